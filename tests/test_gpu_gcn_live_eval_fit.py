"""GPU suite (-m gpu): the replayed validation and ``fit(..., vertex_limit=V)`` with a GCN on the bounded kernels
(``transforms="tile"``), after tests/test_gpu_gat_live_eval_fit.py."""
import pytest
import torch

from test_gpu_eval_step import _loss_bound
from test_gpu_fit import _task

pytestmark = pytest.mark.gpu

CAP, BS = 64, 128


def _gcn(cuda, p=0.1):
    from bliss_gnn_amd.model import GCN
    torch.manual_seed(0)
    return GCN(24, 16, 4, 3, torch.relu, p, transforms="tile").to(cuda).bfloat16()


def _setup(cuda, name, fan):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    g, tr, va, te = _task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    return g, fit.make_sampler(name, fan), _gcn(cuda), tr, va, te


def _trained(cuda, name, fan):
    from bliss_gnn_amd.train import BatchLoader, TrainStep
    g, s, m, tr, va, te = _setup(cuda, name, fan)
    step = TrainStep(g, s, m, lr=0.01)
    torch.manual_seed(5)
    loader = BatchLoader(tr, CAP, seed=5).forever()
    for _ in range(3):
        step(next(loader))
    return g, s, m, va[:2 * CAP + 37]


@pytest.mark.parametrize("name,fan", [("labor", [5, 5, 5]), ("poisson-bandit-keyed", [24, 16, 12])])
def test_ragged_split_is_replayed_whole_with_a_gcn(cuda, name, fan):
    """64 + 64 + 37 validation seeds through one captured evaluation step: the eager metric exactly, the same loss."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import GraphedEvalStep, _ce_loss
    gA, sA, mA, va = _trained(cuda, name, fan)
    gB, sB, mB, _ = _trained(cuda, name, fan)
    assert va.numel() % CAP == 37
    es = GraphedEvalStep(gA, sA, mA, CAP, False, batch_capacity=CAP)
    entered = []
    real = es._eager
    es._eager = lambda *a, **kw: (entered.append(1), real(*a, **kw))[1]
    torch.manual_seed(7)
    acc_g, loss_g = es.run(va)
    lf, terms = _ce_loss(), []

    def recording(pred, y):
        loss = lf(pred, y)
        terms.append(float(loss) * pred.shape[0])
        return loss

    torch.manual_seed(7)
    acc_e, loss_e = fit.evaluate(gB, sB, mB, va, CAP, False, recording)
    print(name, acc_g, acc_e, loss_g, loss_e)
    assert es.replays == 3 == len(terms) and not entered and es.fallbacks == 0
    assert acc_g == acc_e
    assert abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
    es.close()


def _measured_k(cuda, name, fan):
    from bliss_gnn_amd.train import BatchLoader
    g, sampler, _, tr, _, _ = _setup(cuda, name, fan)
    torch.manual_seed(11)
    loader = BatchLoader(tr, BS, seed=0).forever()
    ks = [sampler.sample_blocks(g, next(loader))[2][0].num_src_nodes() for _ in range(6)]
    return sum(ks) / len(ks)


def test_fit_under_a_vertex_limit_with_a_gcn(cuda, monkeypatch):
    """Four epochs, capacity 256: the batch size changes at least twice, and every history entry and all parameter bits of the graphed loop are the eager loop's, from ONE
    captured graph."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import GraphedTrainStep
    name, fan = "labor", [5, 5, 5]
    k0 = _measured_k(cuda, name, fan)
    limit = int(k0 / 2)
    captures, real = [], GraphedTrainStep._capture_graph
    monkeypatch.setattr(GraphedTrainStep, "_capture_graph", lambda self, loader: (captures.append(1), real(self, loader))[1])
    out, params = {}, {}
    for kind in ("eager", "graphed"):
        g, sampler, model, tr, va, te = _setup(cuda, name, fan)
        torch.manual_seed(11)
        out[kind] = fit.fit(g, sampler, model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=4, train_step=kind, vertex_limit=limit,
                            batch_capacity=256)
        params[kind] = [p.detach().contiguous().view(torch.int16).clone() for p in model.parameters()]
    he, hg = out["eager"]["history"], out["graphed"]["history"]
    sizes = [h["batch_size"] for h in hg]
    print("K at", BS, "=", k0, "limit", limit, "batch sizes", sizes)
    assert len(he) == len(hg) == 4 and sizes[0] == BS
    assert sum(1 for a, b in zip(sizes, sizes[1:]) if a != b) >= 2, sizes
    for a, b in zip(he, hg):
        for k in ("batch_size", "batch_size_clamped", "input_nodes", "sampled_nodes", "sampled_edges", "train_loss", "val_acc", "val_loss"):
            assert a[k] == b[k], (k, a, b)
    assert all(torch.equal(p, q) for p, q in zip(params["eager"], params["graphed"]))
    assert captures == [1]
