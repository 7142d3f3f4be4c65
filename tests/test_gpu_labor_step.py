"""GPU suite (-m gpu): the device-side LABOR-0 sampler through ``fit.LaborSampler`` -- three layers against the restatement, the
engine's capacity-regrow loop, captured into a HIP graph and replayed (GraphedTrainStep, GraphedEvalStep), through ``fit.fit``,
and refused by the pipelined loop."""
import math

import numpy as np
import pytest
import torch

import labor_ref as ref
from test_gpu_eval_step import _eager_pass, _loss_bound, _trained
from test_gpu_fit import _task as fit_task
from test_gpu_labor import SEED, graph_np, seeds67

pytestmark = pytest.mark.gpu

FAN, BS, DRAW_SEED = [5, 5, 5], 64, 31


def _assert_blocks(blocks, lays, cuda):
    import bliss_gnn_amd as bg
    t = lambda a: torch.from_numpy(np.asarray(a)).to(cuda)
    for blk, want in zip(reversed(blocks), lays):                                 # sampling order
        c = blk._counts
        assert (c.S, c.E, c.C, c.K, c.B, c.err) == (want["S"], want["E"], want["K"], want["K"], want["B"], 0)
        assert (blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()) == (want["S"], want["K"], want["B"])
        assert torch.equal(blk.indptr, t(want["indptr"])) and torch.equal(blk.src, t(want["src"])) and torch.equal(blk.dst, t(want["dst"]))
        assert torch.equal(blk.pos, t(want["pos"])) and torch.equal(blk.edata[bg.EID], t(want["eid"]))
        assert torch.equal(blk.srcdata[bg.NID], t(want["kept_nid"]))
        ti, te = blk.transposed()
        assert torch.equal(ti, t(want["t_indptr"])) and torch.equal(te[:want["B"]], t(want["t_edge"]))
        assert bool((blk.edata["edge_weights"] == 1).all()) and blk.edata["edge_weights"].dtype == torch.bfloat16
        assert bool((blk._node_prob == 1).all())


def _big_graph(cuda):
    import bliss_gnn_amd as bg
    ip, ix, ei = graph_np()
    return bg.Graph(torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda), torch.from_numpy(ei).to(cuda))


def _assert_engine_clean(eng):
    """Replay hygiene of the engine's own scratch."""
    V = eng.V
    words = -(-(-(-V // 32)) // 1024) * 1024
    assert int(eng._lb_scr[1][:16 + words].abs().sum()) == 0
    for st in eng._sets.values():
        assert bool((st["kept_map"] == -1).all())


@pytest.mark.parametrize("dep", [False, True])
def test_three_layers_are_the_restatements(cuda, dep):
    from bliss_gnn_amd import fit
    g = _big_graph(cuda)
    ip, ix, ei = graph_np()
    s = fit.LaborSampler([10, 3, 3], seed=SEED, layer_dependency=dep)             # input-most first: sampled 3, 3, then 10
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    torch.manual_seed(77)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    for step in range(3):
        assert s.draw_step() == step                                              # one per call
        inp, outp, blocks = s.sample_blocks(g, seeds)
        lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3, 10], SEED, step, layer_dependency=dep)
        _assert_blocks(blocks, lays, cuda)
        assert torch.equal(inp, blocks[0].srcdata["_ID"]) and outp is seeds
    assert s.draw_step() == 3
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    # the same state draws the same blocks
    s.reset_draw(SEED, step=41)
    _, _, again = s.sample_blocks(g, seeds)
    assert s.draw_step() == 42
    _assert_blocks(again, ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3, 10], SEED, 41, layer_dependency=dep), cuda)
    _assert_engine_clean(s._engine)


def test_the_regrow_loop_repeats_the_same_draw_step(cuda):
    """B is not exactly bounded: a call over a capacity is flagged, the step is rewound by one, the capacity grown, the call repeated."""
    from bliss_gnn_amd import fit
    g = _big_graph(cuda)
    ip, ix, ei = graph_np()
    s = fit.LaborSampler([3, 3], seed=SEED)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    s.sample_blocks(g, seeds)
    eng = s._engine
    assert eng.exact_b is False and eng.retries == 0
    eng.caps[0]["B"], eng.caps[1]["B"], eng.caps[1]["K"], eng.ws = 64, 128, 300, None    # below the true B = 232 of the first layer
    _, _, blocks = s.sample_blocks(g, seeds)
    assert eng.retries >= 2 and s.draw_step() == 2
    _assert_blocks(blocks, ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3], SEED, 1), cuda)
    _assert_engine_clean(eng)


# ------------------------------------------------------------------------------------------------- inside the train steps
def _task(cuda, V=2000, E=24000, F=24, classes=4):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, F, generator=gen).bfloat16()
    labels = (feats.float() @ torch.randn(F, classes, generator=gen)).argmax(1)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    perm = torch.randperm(V, generator=gen).to(torch.int32).to(cuda)
    return g, perm[:1200]


def test_graphed_step_replays_the_labor_sampler(cuda):
    """Two identically set up sampler / model pairs on the same loader.  A: GraphedTrainStep -- calibrate 3 (sampler calls that
    train nothing), warm-up 2, the captured step, 7 replays = 10 trained steps.  B: the same 3 sampler calls, then 10 eager
    TrainStep calls.  The losses of the replayed steps, the parameters and the sizes are bit-identical; every replayed step's sizes
    are the restatement's for its seeds and draw step; the step counter ends at calibration + 10."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep

    def build():
        g, tr = _task(cuda)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        return g, fit.LaborSampler(FAN, seed=DRAW_SEED), model, BatchLoader(tr, BS, seed=5).forever()

    g1, s1, m1, l1 = build()
    ip, ix, ei = g1.indptr.cpu().numpy(), g1.indices.cpu().numpy(), g1.eid.cpu().numpy()
    graphed = GraphedTrainStep(g1, s1, m1, BS, lr=0.01)
    rng0 = torch.get_rng_state()
    graphed.calibrate(l1, steps=3)
    graphed.capture(l1, warmup=2)
    assert s1.draw_step() == 6
    losses1 = []
    for i in range(7):
        seeds = next(l1)
        losses1.append(float(graphed(seeds)))
        lays = ref.sample_blocks(ip, ix, ei, seeds.cpu().numpy(), list(reversed(FAN)), DRAW_SEED, 6 + i)
        assert graphed.sizes() == [dict(S=l["S"], E=l["E"], C=l["K"], K=l["K"], B=l["B"]) for l in reversed(lays)], i
    assert s1.draw_step() == 3 + 10
    assert torch.equal(torch.get_rng_state(), rng0), "the device draw must not touch torch's CPU generator"

    g2, s2, m2, l2 = build()
    eager = TrainStep(g2, s2, m2, lr=0.01)
    for _ in range(3):
        s2.sample_blocks(g2, next(l2))
    losses2 = [float(eager(next(l2))) for _ in range(10)]
    assert s2.draw_step() == 13 and torch.equal(torch.get_rng_state(), rng0)
    print("graphed", losses1, "eager", losses2)
    assert losses1 == losses2[3:]
    assert math.isfinite(losses2[-1]) and losses2[-1] < losses2[0]
    sizes2 = [dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in eager.last["mfgs"]]
    assert graphed.sizes() == sizes2
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p1.view(torch.int16), p2.view(torch.int16))
    graphed.close()
    _assert_engine_clean(s1._engine)


def test_replayed_validation_is_the_eager_one(cuda):
    """The assertions of tests/test_gpu_eval_step.py::test_replayed_validation_is_the_eager_one, for ``make_sampler("labor")``."""
    from bliss_gnn_amd.train import GraphedEvalStep
    gA, sA, mA, va = _trained(cuda, "labor", "device", False)
    gB, sB, mB, _ = _trained(cuda, "labor", "device", False)
    assert type(sA).__name__ == "LaborSampler"
    assert all(torch.equal(p, q) for p, q in zip(mA.parameters(), mB.parameters()))
    es = GraphedEvalStep(gA, sA, mA, 128, False)
    for rep in range(2):                                                          # the second pass reuses the graph
        mA.train(); mB.train()
        torch.manual_seed(7 + rep)
        acc_g, loss_g = es.run(va)
        rng_g = torch.get_rng_state()
        torch.manual_seed(7 + rep)
        acc_e, loss_e, counts, terms = _eager_pass(gB, sB, mB, va, False)
        print(rep, acc_g, acc_e, loss_g, loss_e, es.last_counts, counts, _loss_bound(terms, va.numel()))
        assert len(terms) == 4 and va.numel() == 500
        assert es.last_counts == counts                                           # the host counts of the concatenated predictions
        assert acc_g == acc_e                                                     # equal as floats
        assert abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
        assert torch.equal(rng_g, torch.get_rng_state())
        assert sA.draw_step() == sB.draw_step()
        assert mA.training and mB.training
    assert es.captures == 1 and es.fallbacks == 0
    es.close()


def test_fit_runs_the_labor_sampler(cuda):
    """The protocol and acceptance criterion of test_fit_runs_every_sampler_choice (tests/test_gpu_fit.py)."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = fit_task(cuda)
    sampler = fit.make_sampler("labor", [64, 32, 16])
    assert type(sampler) is fit.LaborSampler
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
    seen = []
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=128, lr=0.01, max_epochs=4, log=seen.append)
    assert len(out["history"]) == 4 and out["steps"] == 4 * (1800 // 128)
    assert out["history"][-1]["train_loss"] < out["history"][0]["train_loss"]     # it learns
    assert out["best_val_acc"] > 0.3 and set(out["final"]) == {"Train", "Validation", "Test"}
    assert out["final"]["Test"] > 0.3                                             # 4 classes: chance is 0.25
    assert seen == out["history"]


def test_pipelined_step_refuses_the_labor_sampler(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g, _ = _task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    with pytest.raises(NotImplementedError):
        PipelinedTrainStep(g, fit.LaborSampler(FAN), model, BS)
    s = fit.LaborSampler(FAN)
    with pytest.raises(NotImplementedError):                                      # no split enqueue either
        s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), part="main", external_rng=True)
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), chain_rng=True)
