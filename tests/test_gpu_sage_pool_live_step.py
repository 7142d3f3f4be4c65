"""GPU suite (-m gpu): a pool GraphSAGE on the tile kernels (``SAGE(..., transforms="tile", aggregator_type="pool")``, DESIGN.md
section 32) under a batch capacity, after tests/test_gpu_gcn_live_step.py with the same graph, sizes and method.  One captured
``GraphedTrainStep(batch_capacity=64)`` driven with 64, 37, 1 and 64 live seeds against eager ``TrainStep`` calls of an identically
seeded tile pool model on the same seeds -- every floating-point buffer the step allocates pre-filled with NaN -- the losses of
all steps, all parameter bits and the bandit sampler's EXP3 rows bit-equal; the replayed validation over a ragged split; a
two-epoch ``fit`` under a vertex limit; the ``"auto"`` pool model still refuses."""
import math

import pytest
import torch

from test_gpu_eval_step import _loss_bound
from test_gpu_gcn_live_step import CAP, CLASSES, FEAT, LIVE, SAMPLERS, _bits, _live_batches, _task

pytestmark = pytest.mark.gpu


def _model(cuda, transforms="tile"):
    from bliss_gnn_amd.model import SAGE
    torch.manual_seed(0)
    m = SAGE(FEAT, 16, CLASSES, 3, torch.relu, 0.1, transforms=transforms, aggregator_type="pool").to(cuda).bfloat16()
    m.train()
    return m


def _build(cuda, name, transforms="tile"):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader
    g, tr = _task(cuda)
    return g, fit.make_sampler(name, SAMPLERS[name]), _model(cuda, transforms), tr, BatchLoader(tr, CAP, seed=5).forever()


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_one_captured_pool_step_serves_every_batch_size(cuda, name, monkeypatch):
    from bliss_gnn_amd.train import GraphedTrainStep, TrainStep
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)                              # the warm-up steps and (recorded) every replay
    g, s, m, tr, loader = _build(cuda, name)
    step = GraphedTrainStep(g, s, m, CAP, lr=0.01, batch_capacity=CAP)
    torch.manual_seed(3)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)                                              # three real steps of 64 seeds
    losses, sizes = [], []
    for seeds in _live_batches(tr):
        losses.append(float(step(seeds)))
        sizes.append(step.last_counts[0].S)
    monkeypatch.undo()
    assert sizes == list(LIVE)

    gB, sB, mB, trB, loaderB = _build(cuda, name)
    eager = TrainStep(gB, sB, mB, lr=0.01)
    torch.manual_seed(3)
    for _ in range(3):
        sB.sample_blocks(gB, next(loaderB))
    for _ in range(3):
        eager(next(loaderB))
    want = [float(eager(seeds)) for seeds in _live_batches(trB)]
    print(name, losses, want)
    assert all(math.isfinite(x) for x in losses) and losses == want
    for (k, p), q in zip(m.named_parameters(), mB.parameters()):
        assert bool(torch.isfinite(p.float()).all()) and torch.equal(_bits(p), _bits(q)), k
    if getattr(s, "_w_pos", None) is not None:                                  # the bandit sampler's EXP3 rows (its reward reads embed_norm)
        assert torch.equal(_bits(s._w_pos), _bits(sB._w_pos))
        assert not torch.equal(_bits(s._w_pos[0]), _bits(torch.ones_like(s._w_pos[0])))
    s.check_errors() if hasattr(s, "check_errors") else None
    ctrs = lambda model: [int(model._dropout_state(l, cuda)[0][0]) for l in range(2)]
    assert ctrs(m) == ctrs(mB) and ctrs(m)[0] > 0                               # the dropout streams advanced alike
    if hasattr(step, "close"):
        step.close()


def _trained(cuda, name):
    from bliss_gnn_amd.train import TrainStep
    g, s, m, tr, loader = _build(cuda, name)
    step = TrainStep(g, s, m, lr=0.01)
    torch.manual_seed(5)
    for _ in range(3):
        step(next(loader))
    gen = torch.Generator().manual_seed(4)
    va = torch.randperm(g.num_nodes(), generator=gen)[:2 * CAP + 37].to(torch.int32).to(cuda)
    return g, s, m, va


def test_ragged_split_is_replayed_whole_with_a_pool_model(cuda):
    """64 + 64 + 37 validation seeds through one captured evaluation step: the eager metric exactly, the same loss."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import GraphedEvalStep, _ce_loss
    gA, sA, mA, va = _trained(cuda, "labor")
    gB, sB, mB, _ = _trained(cuda, "labor")
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
    print(acc_g, acc_e, loss_g, loss_e)
    assert es.replays == 3 == len(terms) and not entered and es.fallbacks == 0
    assert acc_g == acc_e
    assert abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
    es.close()


def test_fit_under_a_vertex_limit_with_a_pool_model(cuda):
    """Two epochs of the graphed loop under a vertex limit, replayed validation: finite losses, every parameter moved."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader
    g, sampler, model, tr, _ = _build(cuda, "labor")
    gen = torch.Generator().manual_seed(6)
    rest = torch.randperm(g.num_nodes(), generator=gen).to(torch.int32).to(cuda)
    va, te = rest[:100], rest[100:200]
    torch.manual_seed(11)
    loader = BatchLoader(tr, CAP, seed=0).forever()
    ks = [sampler.sample_blocks(g, next(loader))[2][0].num_src_nodes() for _ in range(4)]
    before = [p.detach().clone() for p in model.parameters()]
    torch.manual_seed(11)
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=CAP, lr=0.01, max_epochs=2, train_step="graphed", eval_step="graphed",
                  vertex_limit=int(sum(ks) / len(ks) / 2), batch_capacity=2 * CAP)
    hist = out["history"]
    print([(h["batch_size"], h["train_loss"], h["val_loss"]) for h in hist])
    assert len(hist) == 2 and all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in hist)
    for (n, p), q in zip(model.named_parameters(), before):
        assert bool(torch.isfinite(p.float()).all()) and not torch.equal(p, q), n


def test_only_the_tile_pool_model_takes_a_capacity(cuda):
    from bliss_gnn_amd.train import GraphedEvalStep, GraphedTrainStep, _live_refusal
    g, s, tile, tr, _ = _build(cuda, "labor")
    assert _live_refusal(tile) is None
    _, _, auto, _, _ = _build(cuda, "labor", transforms="auto")
    assert "MFMA path" in _live_refusal(auto)
    with pytest.raises(NotImplementedError, match="MFMA path"):
        GraphedTrainStep(g, s, auto, CAP, batch_capacity=CAP)
    with pytest.raises(NotImplementedError, match="MFMA path"):
        GraphedEvalStep(g, s, auto, CAP, batch_capacity=CAP)
    why = _live_refusal(tile.float())
    assert why is not None and "bf16" in why
