"""GPU suite (-m gpu): a GCN on the bounded kernels (``transforms="tile"``) under a batch capacity, after
tests/test_gpu_gat_live_step.py.  ``GCN(24, 16, 4, 3, relu, 0.1)`` has a weight-first (24 -> 16), an aggregate-first (16 -> 16) and a
weight-first (16 -> 4) layer.  One captured ``GraphedTrainStep(batch_capacity=64)`` driven with 64, 37, 1 and 64 live seeds
against eager ``TrainStep`` calls of an identically seeded tile model on the same seeds -- every floating-point buffer the step
allocates pre-filled with NaN -- the losses of all steps, all parameter bits and the bandit sampler's EXP3 rows bit-equal; the
default model still refuses, and so does a tile model in fp32."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

V, E, FEAT, CLASSES, CAP = 500, 6000, 24, 4, 64
SAMPLERS = {"poisson-bandit-keyed": [24, 16, 12], "labor": [5, 5, 5]}
LIVE = (64, 37, 1, 64)


def _task(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=23)                                    # lognormal expected in-degrees
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, FEAT, generator=gen).bfloat16()
    labels = (feats.float() @ torch.randn(FEAT, CLASSES, generator=gen)).argmax(1)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    perm = torch.randperm(V, generator=gen).to(torch.int32).to(cuda)
    return g, perm[:360]


def _build(cuda, name, transforms="tile"):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import GCN
    from bliss_gnn_amd.train import BatchLoader
    g, tr = _task(cuda)
    torch.manual_seed(0)
    model = GCN(FEAT, 16, CLASSES, 3, torch.relu, 0.1, transforms=transforms).to(cuda).bfloat16()
    model.train()
    return g, fit.make_sampler(name, SAMPLERS[name]), model, tr, BatchLoader(tr, CAP, seed=5).forever()


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


def _live_batches(tr):
    perm = tr[torch.randperm(tr.numel(), generator=torch.Generator().manual_seed(9)).to(tr.device)]
    out, o = [], 0
    for n in LIVE:
        out.append(perm[o:o + n].clone())
        o += n
    return out


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_one_captured_gcn_step_serves_every_batch_size(cuda, name, monkeypatch):
    from bliss_gnn_amd.train import GraphedTrainStep, TrainStep
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)                              # the warm-up steps and (recorded) every replay
    g, s, m, tr, loader = _build(cuda, name)
    assert [l._in_feats > l._out_feats for l in m.layers] == [True, False, True]
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
    assert [int(l._drop_state(cuda)["ctr"][0]) for l in m.layers[:-1]] == [int(l._drop_state(cuda)["ctr"][0]) for l in mB.layers[:-1]]
    if hasattr(step, "close"):
        step.close()


def test_the_default_gcn_still_refuses_a_capacity(cuda):
    from bliss_gnn_amd.train import GraphedEvalStep, GraphedTrainStep, _live_refusal
    g, s, m, tr, _ = _build(cuda, "labor", transforms="library")
    with pytest.raises(NotImplementedError, match='transforms="tile"'):
        GraphedTrainStep(g, s, m, CAP, batch_capacity=CAP)
    with pytest.raises(NotImplementedError, match="GCN"):
        GraphedEvalStep(g, s, m, CAP, batch_capacity=CAP)
    _, _, tile, _, _ = _build(cuda, "labor")
    assert _live_refusal(tile) is None
    why = _live_refusal(tile.float())
    assert why is not None and "bf16" in why and "GCN layer 0" in why
