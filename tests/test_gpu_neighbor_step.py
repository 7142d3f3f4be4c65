"""GPU suite (-m gpu): the device-side neighbor sampler inside the train steps -- captured into a HIP graph and replayed
(GraphedTrainStep), through ``fit.fit``, and refused by the pipelined loop."""
import math

import numpy as np
import pytest
import torch

import neighbor_ref as ref

pytestmark = pytest.mark.gpu

FAN, BS, DRAW_SEED = [8, 4, 4], 128, 31


def _task(cuda, V=3000, E=40000, F=24, classes=4):
    """(the helper of tests/test_gpu_fit.py)"""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, F, generator=gen).bfloat16()
    labels = (feats.float() @ torch.randn(F, classes, generator=gen)).argmax(1)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    perm = torch.randperm(V, generator=gen).to(torch.int32).to(cuda)
    return g, perm[:1800], perm[1800:2300], perm[2300:]


class Recorded:
    """A loader that remembers the batches it handed out."""

    def __init__(self, ids):
        from bliss_gnn_amd.train import BatchLoader
        self.it, self.seen = BatchLoader(ids, BS, seed=5).forever(), []

    def __iter__(self):
        return self

    def __next__(self):
        self.seen.append(next(self.it))
        return self.seen[-1]


def test_graphed_step_replays_the_neighbor_sampler(cuda):
    """Two identically set up steps, both calibrated with 3 sampler calls.  A: captured (2 warm-up steps, the captured one, then
    17 replays = 20 steps).  B: 20 eager_steps.  Every observable step's sizes are the restatement's for that step's seeds and draw
    step; the last losses are bit-identical; the loss is finite and has fallen."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import GraphedTrainStep

    def build():
        g, tr, _, _ = _task(cuda)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        sampler = fit.NeighborSampler(FAN, seed=DRAW_SEED, draw="device")
        step = GraphedTrainStep(g, sampler, model, BS, lr=0.01)
        loader = Recorded(tr)
        step.calibrate(loader, steps=3)
        return g, sampler, step, loader

    g, s1, graphed, l1 = build()
    ip, ix, ei = g.indptr.cpu().numpy(), g.indices.cpu().numpy(), g.eid.cpu().numpy()
    want = {}

    def check_sizes(step, seeds, draw_step):
        if draw_step not in want:
            lays = ref.sample_blocks(ip, ix, ei, seeds.cpu().numpy(), list(reversed(FAN)), DRAW_SEED, draw_step)
            want[draw_step] = [dict(S=l["S"], E=l["E"], C=l["K"], K=l["K"], B=l["B"]) for l in reversed(lays)]
        assert step.sizes() == want[draw_step], (draw_step, step.sizes(), want[draw_step])

    rng0 = torch.get_rng_state()
    graphed.capture(l1, warmup=2)
    check_sizes(graphed, l1.seen[5], 5)                                          # calibration 0..2, warm-up 3..4, the captured step
    for i in range(17):
        loss1 = graphed(next(l1))
        check_sizes(graphed, l1.seen[-1], 6 + i)
    assert s1.draw_step() == 23 and len(l1.seen) == 23
    assert torch.equal(torch.get_rng_state(), rng0), "the device draw must not touch torch's CPU generator"

    _, s2, twin, l2 = build()
    losses = []
    for i in range(20):
        losses.append(float(twin.eager_step(next(l2))))
        check_sizes(twin, l2.seen[-1], 3 + i)
    assert all(torch.equal(a, b) for a, b in zip(l1.seen, l2.seen))
    print("losses", losses, "graphed", float(loss1))
    assert float(loss1) == losses[-1]
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0]
    for p1, p2 in zip(graphed.model.parameters(), twin.model.parameters()):
        assert torch.equal(p1.view(torch.int16), p2.view(torch.int16))
    graphed.close()


def test_fit_runs_the_device_neighbor_sampler(cuda):
    """The protocol of test_fit_runs_every_sampler_choice (tests/test_gpu_fit.py)."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = _task(cuda)
    sampler = fit.make_sampler("neighbor", [64, 32, 16], draw="device")
    assert sampler.draw == "device"
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
    seen = []
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=128, lr=0.01, max_epochs=4, log=seen.append)
    assert len(out["history"]) == 4 and out["steps"] == 4 * (1800 // 128)
    assert out["history"][-1]["train_loss"] < out["history"][0]["train_loss"]     # it learns
    assert out["best_val_acc"] > 0.3 and set(out["final"]) == {"Train", "Validation", "Test"}
    assert out["final"]["Test"] > 0.3                                             # 4 classes: chance is 0.25
    assert seen == out["history"]


def test_pipelined_step_refuses_the_device_neighbor_sampler(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g, _, _, _ = _task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    with pytest.raises(NotImplementedError):
        PipelinedTrainStep(g, fit.NeighborSampler(FAN, draw="device"), model, BS)
    s = fit.NeighborSampler(FAN, draw="device")
    with pytest.raises(NotImplementedError):                                      # no split enqueue either
        s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), part="main", external_rng=True)
