"""GPU suite (-m gpu): ``fit(..., vertex_limit=V)`` (the reference's ``--vertex-limit``) on the learnable task
of tests/test_gpu_fit.py: the batch size falls towards the vertex budget, the eager and the graphed loop take the same decisions
on the same blocks, the graphed loop never re-captures, and ``vertex_limit=-1`` is ``fit`` as it was."""
import pytest
import torch

from test_gpu_fit import _task

pytestmark = pytest.mark.gpu

BS = 128
SAMPLERS = {"poisson-bandit": [64, 32, 16], "labor": [5, 5, 5]}


def _setup(cuda, name, p=0.0):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = _task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    sampler = fit.make_sampler(name, SAMPLERS[name])
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, p).to(cuda).bfloat16()
    return g, sampler, model, tr, va, te


def _measured_k(cuda, name):
    """The mean input-layer size of a few batches at the starting batch size (a sampler of its own)."""
    from bliss_gnn_amd.train import BatchLoader
    g, sampler, _, tr, _, _ = _setup(cuda, name)
    torch.manual_seed(11)
    loader = BatchLoader(tr, BS, seed=0).forever()
    ks = [sampler.sample_blocks(g, next(loader))[2][0].num_src_nodes() for _ in range(6)]
    return sum(ks) / len(ks)


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_batch_size_follows_the_vertex_budget_in_both_loops(cuda, name, monkeypatch):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import GraphedTrainStep
    k0 = _measured_k(cuda, name)
    limit = int(k0 / 2)
    captures, real = [], GraphedTrainStep._capture_graph
    monkeypatch.setattr(GraphedTrainStep, "_capture_graph", lambda self, loader: (captures.append(1), real(self, loader))[1])
    out, params = {}, {}
    for kind in ("eager", "graphed"):
        g, sampler, model, tr, va, te = _setup(cuda, name)
        torch.manual_seed(11)
        out[kind] = fit.fit(g, sampler, model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=4, train_step=kind, vertex_limit=limit,
                            batch_capacity=2 * BS)
        params[kind] = [_bits(q).clone() for q in model.parameters()]
    he, hg = out["eager"]["history"], out["graphed"]["history"]
    sizes = [h["batch_size"] for h in hg]
    print(name, "K at", BS, "=", k0, "limit", limit, "batch sizes", sizes, "input K", [h["input_nodes"]["m"] for h in hg])
    assert len(he) == len(hg) == 4 and sizes[0] == BS
    assert min(sizes[1:3]) < BS                                                 # it falls within the first epochs
    assert all(1 <= b <= 2 * BS for b in sizes)
    assert abs(hg[-1]["input_nodes"]["m"] - limit) < abs(hg[0]["input_nodes"]["m"] - limit)
    assert hg[0]["input_nodes"]["n"] == 1800 // BS
    for a, b in zip(he, hg):                                                    # the same decisions on the same blocks
        for k in ("batch_size", "batch_size_clamped", "input_nodes", "sampled_nodes", "sampled_edges", "train_loss", "val_acc", "val_loss"):
            assert a[k] == b[k], (k, a, b)
    assert out["eager"]["steps"] == out["graphed"]["steps"] == sum(1800 // b for b in sizes)
    assert all(torch.equal(p, q) for p, q in zip(params["eager"], params["graphed"]))
    assert captures == [1]                                                      # one capture serves every batch size


def test_without_a_limit_fit_is_what_it_was(cuda):
    from bliss_gnn_amd import fit
    res = []
    for kw in ({}, dict(vertex_limit=-1, limit_factor=3, batch_capacity=None)):
        for kind in ("eager", "graphed"):
            g, sampler, model, tr, va, te = _setup(cuda, "labor", 0.1)
            torch.manual_seed(11)
            out = fit.fit(g, sampler, model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=2, train_step=kind, **kw)
            res.append((kind, out["history"], out["steps"], out["final"], [_bits(q).clone() for q in model.parameters()]))
    for (k0, h0, s0, f0, p0), (k1, h1, s1, f1, p1) in zip(res[:2], res[2:]):
        assert k0 == k1 and h0 == h1 and s0 == s1 and f0 == f1 and all(torch.equal(a, b) for a, b in zip(p0, p1))
        assert "batch_size" not in h0[0] and "input_nodes" not in h0[0]
    assert "sampled_nodes" not in res[0][1][0] and "sampled_nodes" in res[1][1][0]


def test_graphed_validation_follows_the_batch_size(cuda):
    """eval_step="graphed" under a vertex limit: the replayed validation runs at the current batch size inside the capacity."""
    from bliss_gnn_amd import fit
    limit = int(_measured_k(cuda, "labor") / 2)
    out = {}
    for ev, train in (("eager", "graphed"), ("graphed", "graphed"), ("graphed", "eager")):
        g, sampler, model, tr, va, te = _setup(cuda, "labor")
        torch.manual_seed(11)
        out[ev if train == "graphed" else "eager-train"] = fit.fit(g, sampler, model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=3, train_step=train,
                                                                   eval_step=ev, vertex_limit=limit)["history"]
    for other in ("graphed", "eager-train"):                                    # (the eager train loop with the replayed validation too)
        assert [h["batch_size"] for h in out["eager"]] == [h["batch_size"] for h in out[other]]
        assert [h["val_acc"] for h in out["eager"]] == [h["val_acc"] for h in out[other]]
    assert out["graphed"][-1]["batch_size"] < BS
