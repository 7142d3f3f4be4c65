"""GPU suite (-m gpu): the device-side LABOR-i sampler through ``fit.ImportanceLaborSampler`` -- three layers against the
restatement, the engine's capacity-regrow loop, captured into a HIP graph and replayed (GraphedTrainStep, GraphedEvalStep), through
``fit.fit`` by its sampler name, refused by the pipelined loop, and a SAGE layer over its non-unit weights."""
import math

import numpy as np
import pytest
import torch

import labor_is_ref as ref
from test_gpu_eval_step import _eager_pass, _loss_bound, _trained
from test_gpu_fit import _task as fit_task
from test_gpu_labor import SEED, graph_np, seeds67
from test_gpu_labor_is import bits
from test_gpu_labor_step import _big_graph, _task

pytestmark = pytest.mark.gpu

FAN, BS, DRAW_SEED = [5, 5, 5], 64, 31


def _assert_blocks(blocks, lays, cuda):
    import bliss_gnn_amd as bg
    t = lambda a: torch.from_numpy(np.asarray(a)).to(cuda)
    for blk, want in zip(reversed(blocks), lays):                                 # sampling order
        c, B = blk._counts, want["B"]
        assert (c.S, c.E, c.C, c.K, c.B, c.err) == (want["S"], want["E"], want["K"], want["K"], B, 0)
        assert (blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()) == (want["S"], want["K"], B)
        assert torch.equal(blk.indptr, t(want["indptr"])) and torch.equal(blk.src, t(want["src"])) and torch.equal(blk.dst, t(want["dst"]))
        assert torch.equal(blk.pos, t(want["pos"])) and torch.equal(blk.edata[bg.EID], t(want["eid"]))
        assert torch.equal(blk.srcdata[bg.NID], t(want["kept_nid"]))
        ti, te = blk.transposed()
        assert torch.equal(ti, t(want["t_indptr"])) and torch.equal(te[:B], t(want["t_edge"]))
        w = blk.edata["edge_weights"]
        assert w.dtype == torch.bfloat16 and w.numel() == B
        assert int((bits(w) - t(ref.bf16_of_f64(want["edge_weights"]).astype(np.int32))).abs().max()) <= 1      # one bf16 ulp
        assert torch.equal(bits(blk._q[:B]), t(want["q_ij"].astype(np.int32)))
        assert bool((blk._node_prob == 1).all())


def _assert_engine_clean(eng):
    """Replay hygiene of the engine's own scratch: tickets, bitmap, both importance buffers, kept_map."""
    V = eng.V
    words = -(-(-(-V // 32)) // 1024) * 1024
    scr = eng._li_scr[2]
    assert int(scr[:16 + words].abs().sum()) == 0
    o = 16 + words + words // 1024
    assert int((scr[o:o + 2 * V] != 0).sum()) == 0
    for st in eng._sets.values():
        assert bool((st["kept_map"] == -1).all())


@pytest.mark.parametrize("dep", [False, True])
def test_three_layers_are_the_restatements(cuda, dep):
    from bliss_gnn_amd import fit
    g = _big_graph(cuda)
    ip, ix, ei = graph_np()
    s = fit.ImportanceLaborSampler([10, 3, 3], iterations=2, seed=SEED, layer_dependency=dep)   # input-most first: sampled 3, 3, then 10
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    torch.manual_seed(77)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    for step in range(2):
        assert s.draw_step() == step                                              # one per call
        inp, outp, blocks = s.sample_blocks(g, seeds)
        lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3, 10], SEED, step, 2, layer_dependency=dep)
        _assert_blocks(blocks, lays, cuda)
        assert torch.equal(inp, blocks[0].srcdata["_ID"]) and outp is seeds
        assert any(bool((b.edata["edge_weights"] != 1).any()) for b in blocks)    # (Hajek weights, not LABOR-0's units)
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    s.reset_draw(SEED, step=41)                                                   # the same state draws the same blocks
    _, _, again = s.sample_blocks(g, seeds)
    assert s.draw_step() == 42
    _assert_blocks(again, ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3, 10], SEED, 41, 2, layer_dependency=dep), cuda)
    _assert_engine_clean(s._engine)
    assert s._engine._lb_scr is None                                              # (csrc/labor.hip was not run)


def test_zero_iterations_run_these_kernels_and_draw_labor_0(cuda):
    from bliss_gnn_amd import fit
    g = _big_graph(cuda)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    s0, s = fit.LaborSampler([3, 3], seed=SEED), fit.ImportanceLaborSampler([3, 3], iterations=0, seed=SEED)
    _, _, want = s0.sample_blocks(g, seeds)
    _, _, got = s.sample_blocks(g, seeds)
    for a, b in zip(got, want):
        for name in ("indptr", "src", "dst", "pos"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert torch.equal(a.srcdata["_ID"], b.srcdata["_ID"]) and bool((a.edata["edge_weights"] == 1).all())
    assert s._engine._lb_scr is None and s._engine._li_scr is not None and s0._engine._li_scr is None


def test_the_regrow_loop_repeats_the_same_draw_step(cuda):
    """B is not exactly bounded: a call over a capacity is flagged, the step is rewound by one, the capacity (and the scratch that
    is sized by it) grown, the call repeated."""
    from bliss_gnn_amd import fit
    g = _big_graph(cuda)
    ip, ix, ei = graph_np()
    s = fit.ImportanceLaborSampler([3, 3], iterations=1, seed=SEED)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    s.sample_blocks(g, seeds)
    eng = s._engine
    assert eng.exact_b is False and eng.retries == 0
    eng.caps[0]["B"], eng.caps[1]["B"], eng.caps[1]["K"], eng.ws = 64, 128, 300, None    # below the true B of the first layer
    _, _, blocks = s.sample_blocks(g, seeds)
    assert eng.retries >= 2 and s.draw_step() == 2
    lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3], SEED, 1, 1)
    assert lays[0]["B"] > 64
    _assert_blocks(blocks, lays, cuda)
    _assert_engine_clean(eng)


# ------------------------------------------------------------------------------------------------- inside the train steps
def test_graphed_step_replays_the_sampler(cuda):
    """tests/test_gpu_labor_step.py's twin experiment: A = GraphedTrainStep (calibrate 3, warm-up 2, the captured step, 7 replays),
    B = the same 3 sampler calls, then 10 eager TrainStep calls.  Losses of the replayed steps, parameters and sizes are
    bit-identical; every replayed step's sizes are the restatement's for its seeds and draw step."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep

    def build():
        g, tr = _task(cuda)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        return g, fit.ImportanceLaborSampler(FAN, iterations=2, seed=DRAW_SEED), model, BatchLoader(tr, BS, seed=5).forever()

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
        lays = ref.sample_blocks(ip, ix, ei, seeds.cpu().numpy(), list(reversed(FAN)), DRAW_SEED, 6 + i, 2)
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
    """The assertions of tests/test_gpu_eval_step.py::test_replayed_validation_is_the_eager_one, for ``make_sampler("labor-2")``."""
    from bliss_gnn_amd.train import GraphedEvalStep
    gA, sA, mA, va = _trained(cuda, "labor-2", "device", False)
    gB, sB, mB, _ = _trained(cuda, "labor-2", "device", False)
    assert type(sA).__name__ == "ImportanceLaborSampler" and sA.iterations == 2
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


def test_fit_runs_the_sampler_by_name(cuda):
    """The protocol and acceptance criterion of tests/test_gpu_labor_step.py::test_fit_runs_the_labor_sampler."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = fit_task(cuda)
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
    sampler = fit.make_sampler("labor-2", [64, 32, 16])
    assert type(sampler) is fit.ImportanceLaborSampler and sampler.iterations == 2
    seen = []
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=128, lr=0.01, max_epochs=4, log=seen.append)
    assert len(out["history"]) == 4 and out["steps"] == 4 * (1800 // 128)
    assert out["history"][-1]["train_loss"] < out["history"][0]["train_loss"]     # it learns
    assert out["best_val_acc"] > 0.3 and set(out["final"]) == {"Train", "Validation", "Test"}
    assert out["final"]["Test"] > 0.3                                             # 4 classes: chance is 0.25
    assert seen == out["history"]


def test_pipelined_step_refuses_the_sampler(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g, _ = _task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    with pytest.raises(NotImplementedError):
        PipelinedTrainStep(g, fit.ImportanceLaborSampler(FAN, iterations=1), model, BS)
    s = fit.ImportanceLaborSampler(FAN, iterations=1)
    with pytest.raises(NotImplementedError):                                      # no split enqueue either
        s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), part="main", external_rng=True)
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), chain_rng=True)


def test_sage_forward_and_backward_over_non_unit_weights_and_an_empty_column(cuda):
    """A block with columns that keep nothing and Hajek weights != 1: the mean aggregation and its gradient against an fp32
    evaluation of out[s] = (1 / k_s) sum_e w_e h[src_e] on the same bf16 inputs.  The kernel accumulates in fp32 and rounds once
    to bf16: half a bf16 ulp of the result (2^-9 relative, taken as 2^-8) plus 2^-20 of the sum of the terms' magnitudes for the
    fp32 accumulation in another order."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.nn import SAGEConv, weighted_aggregate
    g = _big_graph(cuda)
    ip, ix, ei = graph_np()
    want = ref.sample_layer(ip, ix, ei, np.array(seeds67()), 1, SEED, 0, 0, 2)
    deg = np.diff(ip)[np.array(seeds67())]
    k = np.diff(want["indptr"])
    rows = np.nonzero((k == 0) & (deg > 1))[0]
    assert len(rows) > 0                                                          # columns above the fanout that keep nothing
    s = fit.ImportanceLaborSampler([1], iterations=2, seed=SEED)
    _, _, blocks = s.sample_blocks(g, torch.tensor(seeds67(), dtype=torch.int32, device=cuda))
    blk = blocks[0]
    _assert_blocks(blocks, [want], cuda)
    w = blk.edata["edge_weights"]
    assert bool((w != 1).any())
    torch.manual_seed(3)
    h = torch.randn(blk.num_src_nodes(), 16, device=cuda).bfloat16().requires_grad_(True)
    agg = weighted_aggregate(blk, h, w, mean=True)
    go = torch.randn(67, 16, device=cuda).bfloat16()
    agg.backward(go)
    src, dst = blk.src.long(), blk.dst.long()
    kk = torch.from_numpy(np.maximum(k, 1)).to(cuda).float()
    terms = w.float()[:, None] * h.detach().float()[src] / kk[dst][:, None]
    ref_out = torch.zeros(67, 16, device=cuda).index_add_(0, dst, terms)
    mag = torch.zeros(67, 16, device=cuda).index_add_(0, dst, terms.abs())
    assert bool(((agg.float() - ref_out).abs() <= 2.0 ** -8 * ref_out.abs() + 2.0 ** -20 * mag).all())
    r = torch.from_numpy(rows).to(cuda)
    assert bool((agg[r] == 0).all())
    gterms = w.float()[:, None] * go.float()[dst] / kk[dst][:, None]
    ref_g = torch.zeros(blk.num_src_nodes(), 16, device=cuda).index_add_(0, src, gterms)
    gmag = torch.zeros(blk.num_src_nodes(), 16, device=cuda).index_add_(0, src, gterms.abs())
    assert bool(((h.grad.float() - ref_g).abs() <= 2.0 ** -8 * ref_g.abs() + 2.0 ** -20 * gmag).all())
    conv = SAGEConv(16, 24, "mean").to(cuda).bfloat16()
    out = conv(blk, h.detach(), w)
    assert out.shape == (67, 24) and bool(torch.isfinite(out.float()).all())
    assert torch.equal(out[r], conv.fc_self(h.detach()[:67])[r])                  # the neighbour term of an empty column is zero
