"""GPU suite (-m gpu): the weighted LABOR samplers (fit.WeightedLaborSampler, fit.BanditLaborSampler) as a
sampler loop against the oracle's EXP3 update and the restatement's draw, through the engine's capacity-regrow loop, inside the
train steps -- captured into a HIP graph and replayed --, in a replayed validation pass, through ``fit.fit`` with both train
steps, and refused by the pipelined loop."""
import math

import numpy as np
import pytest
import torch

import wlabor_ref as ref
from conftest import bf16_bits
from oracle import bliss_oracle as bo
from test_gpu_eval_step import _eager_pass, _loss_bound, _trained
from test_gpu_fit import _task as fit_task
from test_gpu_labor import SEED, graph_np, seeds67
from test_gpu_labor_step import _big_graph
from test_gpu_wlabor import bits

pytestmark = pytest.mark.gpu

FAN, BS, DRAW_SEED = [8, 4, 4], 128, 31


def _oblock(blk):
    import bliss_gnn_amd as bg
    c = lambda t: t.cpu().long()
    return bo.OBlock(blk.num_src_nodes(), blk.num_dst_nodes(), c(blk.indptr), c(blk.src), c(blk.dst), c(blk.edata[bg.EID]),
                     blk.edata["edge_weights"].cpu(), blk.edata["q_ij"].cpu(), torch.ones(blk.num_src_nodes()).bfloat16(),
                     c(blk.srcdata["_ID"]), c(blk.dstdata["_ID"]))


def _assert_block(blk, want, cuda):
    import bliss_gnn_amd as bg
    t = lambda a: torch.from_numpy(np.asarray(a)).to(cuda)
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
    assert int((bits(w) - t(ref.bf16_of_f64(want["edge_weights"]).astype(np.int32))).abs().max()) <= 1          # one bf16 ulp
    assert torch.equal(bits(blk.edata["q_ij"]), t(want["q_ij"].astype(np.int32)))
    assert blk.edata["p_ij"].numel() == B and torch.equal(bits(blk.edata["p_ij"]), t(want["p_ij"].astype(np.int32)))


def _assert_engine_clean(eng):
    """Replay hygiene of the engine's own scratch: tickets, the pending-error word, bitmap, kept_map."""
    words = -(-(-(-eng.V // 32)) // 1024) * 1024
    assert int(eng._wl_scr[2][:16 + words].abs().sum()) == 0
    assert eng._lb_scr is None and eng._li_scr is None and eng._wn_scr is None    # (only csrc/labor_w.hip ran)
    for st in eng._sets.values():
        assert bool((st["kept_map"] == -1).all())


@pytest.mark.parametrize("model", ["sage", "gat"])
def test_sampler_loop_against_the_oracles_exp3(cuda, model):
    """Two steps: the blocks are the restatement's draw over exp3_edge_prob on the CURRENT rows (so the sampler reads what the
    update wrote), rewards and exp3_weights are the oracle's bit for bit."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(3000, 50000, seed=3)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda))
    g.edata["w"] = bg.normalized_edata(g)
    og = bo.CSC(ip, ix, ei)
    edge_w = bo.normalized_edata(og)
    fan, eta = [5, 3], 0.4
    s = fit.BanditLaborSampler(fan, eta=eta, model=model, seed=DRAW_SEED)
    gen = torch.Generator().manual_seed(4)
    o_w = torch.ones(2, og.num_edges, dtype=torch.bfloat16)
    ipn, ixn, ein = ip.numpy(), ix.numpy(), ei.numpy()
    shrunk = False
    for step in range(2):
        seeds = torch.randperm(3000, generator=gen)[:40].to(torch.int32)
        _, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        assert s.draw_step() == step + 1
        o_blocks, cur = [None, None], seeds.long()
        for n, b in enumerate(reversed(range(2))):                                # sampling order: block 1 first
            blk = blocks[b]
            assert torch.equal(blk.dstdata["_ID"].cpu().long(), cur)
            fr = bo.expand_frontier(og, cur)
            q, _ = bo.exp3_edge_prob(og, fr, o_w[b], eta)
            q_pos = np.full(og.num_edges, np.nan, dtype=np.float32)
            q_pos[fr.pos.numpy()] = q.float().numpy()
            want = ref.sample_layer(ipn, ixn, ein, cur.numpy(), fan[b], DRAW_SEED, step, n, q_pos)
            _assert_block(blk, want, cuda)                                        # (q_ij = the oracle's exp3_edge_prob on the kept edges)
            assert bool((blk.srcdata["node_prob"] == 1).all())
            deg = ipn[cur.numpy() + 1] - ipn[cur.numpy()]
            shrunk |= bool((np.diff(want["indptr"])[deg > fan[b]] != fan[b]).any())   # (a column keeps fanout edges in expectation only)
            o_blocks[b] = _oblock(blk)
            cur = o_blocks[b].src_nid
        en, aij = [], []
        for blk, ob in zip(blocks, o_blocks):
            e_ = (torch.rand(ob.n_src, generator=gen) * 20).bfloat16()
            blk.srcdata["embed_norm"] = e_.to(cuda)
            en.append(e_)
            if model == "gat":
                a_ = torch.rand(ob.eid.numel(), generator=gen).bfloat16()
                blk.edata["a_ij"] = a_.to(cuda)
                aij.append(a_)
        s.exp3(blocks, g)
        s.check_errors()
        o_w, traces = bo.exp3(og, o_blocks, o_w, edge_w, en, a_ij=aij if model == "gat" else None)
        for blk, tr in zip(blocks, traces):
            assert np.array_equal(bf16_bits(blk.edata["rewards"]), bf16_bits(tr["rewards"]))
        assert np.array_equal(bf16_bits(s.exp3_weights), bf16_bits(o_w))
    assert shrunk and not torch.equal(o_w, torch.ones_like(o_w))                  # (the second step drew from updated rows)
    _assert_engine_clean(s._engine)


def _ones_rows(ip, n_layers, eta):
    """The restatement's q of the untouched EXP3 rows (all ones), per layer, as functions of the layer's seeds."""
    w = np.ones(int(ip[-1]), dtype=np.float32)
    return [lambda seeds: ref.exp3_q_pos(ip, np.asarray(seeds, dtype=np.int64), w, eta)] * n_layers


def test_the_regrow_loop_repeats_the_same_draw_step(cuda):
    """B is not exactly bounded: a call over a capacity is flagged, the step is rewound by one, the capacity (and the scratch and
    p_ij buffer that are sized by it) grown, the call repeated."""
    from bliss_gnn_amd import fit
    g = _big_graph(cuda)
    ip, ix, ei = graph_np()
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    for dep in (False, True):
        s = fit.BanditLaborSampler([3, 3], eta=0.4, seed=SEED, layer_dependency=dep)
        _, _, blocks = s.sample_blocks(g, seeds)
        lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3], SEED, 0, _ones_rows(ip, 2, 0.4), layer_dependency=dep)
        for blk, want in zip(reversed(blocks), lays):
            _assert_block(blk, want, cuda)
        eng = s._engine
        assert eng.exact_b is False and eng.retries == 0
        eng.caps[0]["B"], eng.caps[1]["B"], eng.caps[1]["K"], eng.ws = 64, 128, 300, None    # below the true B of the first layer
        _, _, blocks = s.sample_blocks(g, seeds)
        assert eng.retries >= 2 and s.draw_step() == 2
        lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [3, 3], SEED, 1, _ones_rows(ip, 2, 0.4), layer_dependency=dep)
        assert lays[0]["B"] > 64
        for blk, want in zip(reversed(blocks), lays):
            _assert_block(blk, want, cuda)
        _assert_engine_clean(eng)


def test_prob_by_edge_id_reaches_the_kernel_by_position(cuda):
    """``WeightedLaborSampler``: q_ij is the given probability, p_ij the inclusion probability, an edge with probability 0 is never
    kept in a column that is not kept whole, and the blocks are the restatement's."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    g, tr, _, _ = fit_task(cuda)
    E = g.num_edges()
    p = torch.rand(E, generator=torch.Generator().manual_seed(8)).bfloat16()
    p[torch.randperm(E, generator=torch.Generator().manual_seed(9))[:E // 3]] = 0.0
    g.edata["p"] = p.to(cuda)
    sw = fit.WeightedLaborSampler([4, 4], "p", seed=DRAW_SEED)
    s0 = fit.LaborSampler([4, 4], seed=DRAW_SEED)
    _, _, bw = sw.sample_blocks(g, tr[:BS])
    _, _, b0 = s0.sample_blocks(g, tr[:BS])
    assert "p_ij" not in b0[-1].edata and not torch.equal(bw[-1].pos, b0[-1].pos)
    ip, ix, ei = g.indptr.cpu().numpy(), g.indices.cpu().numpy(), g.eid.cpu().numpy()
    q_pos = g.by_position(g.edata["p"]).float().cpu().numpy()
    lays = ref.sample_blocks(ip, ix, ei, tr[:BS].cpu().numpy(), [4, 4], DRAW_SEED, 0, [q_pos, q_pos])
    for blk, want in zip(reversed(bw), lays):
        _assert_block(blk, want, cuda)
        assert torch.equal(blk.edata["q_ij"].view(torch.int16), g.edata["p"][blk.edata[bg.EID].long()].view(torch.int16))
        deg = torch.from_numpy(np.diff(ip)).to(cuda)[blk.dstdata["_ID"].long()]
        whole = (deg <= 4)[blk.dst.long()]
        assert bool((blk.edata["q_ij"][~whole] > 0).all()) and bool((blk.edata["p_ij"][whole] == 1).all())
        assert bool((blk.edata["p_ij"][~whole] > 0).all()) and bool((blk.edata["edge_weights"][whole] == 1).all())
    assert any(bool((b.edata["edge_weights"] != 1).any()) for b in bw)            # (Hajek weights, not LABOR-0's units)
    sw.check_errors()


# ------------------------------------------------------------------------------------------------- inside the train steps
def _step_task(cuda):
    import bliss_gnn_amd as bg
    g, tr, va, _ = fit_task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    return g, tr, va


def test_graphed_step_replays_the_bandit_sampler(cuda):
    """tests/test_gpu_wneighbor_step.py's arrangement with an eager twin: A = GraphedTrainStep (calibrate 3, warm-up 2, the captured
    step, 6 replays), B = the same 3 sampler calls, then 9 eager TrainStep calls from the same seeds and draw state.  The losses of
    the replayed steps, the parameters, the sizes and the EXP3 rows are bit-identical; the draw step advances by one per replay."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep

    def build():
        g, tr, va = _step_task(cuda)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        return g, fit.BanditLaborSampler(FAN, eta=0.4, seed=DRAW_SEED), model, BatchLoader(tr, BS, seed=5).forever(), va

    g1, s1, m1, l1, va = build()
    graphed = GraphedTrainStep(g1, s1, m1, BS, lr=0.01)
    rng0 = torch.get_rng_state()
    graphed.calibrate(l1, steps=3)
    graphed.capture(l1, warmup=2)
    assert s1.draw_step() == 6
    losses1 = []
    for i in range(6):
        losses1.append(float(graphed(next(l1))))
        assert s1.draw_step() == 7 + i                                            # one per replay
    s1.check_errors()
    assert torch.equal(torch.get_rng_state(), rng0), "the device draw must not touch torch's CPU generator"

    g2, s2, m2, l2, _ = build()
    eager = TrainStep(g2, s2, m2, lr=0.01)
    for _ in range(3):
        s2.sample_blocks(g2, next(l2))
    losses2 = [float(eager(next(l2))) for _ in range(9)]
    s2.check_errors()
    assert s2.draw_step() == 12 and torch.equal(torch.get_rng_state(), rng0)
    print("graphed", losses1, "eager", losses2)
    assert losses1 == losses2[3:]
    assert math.isfinite(losses2[-1]) and losses2[-1] < losses2[0]
    sizes2 = [dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in eager.last["mfgs"]]
    assert graphed.sizes() == sizes2
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p1.view(torch.int16), p2.view(torch.int16))
    w1 = s1.exp3_weights
    assert torch.equal(w1.view(torch.int16), s2.exp3_weights.view(torch.int16))
    assert not torch.equal(w1, torch.ones_like(w1))                               # (the bandit update ran inside the graph)
    graphed.close()
    _assert_engine_clean(s1._engine)


def test_replayed_validation_is_the_eager_one(cuda):
    """The assertions of tests/test_gpu_eval_step.py::test_replayed_validation_is_the_eager_one, for ``make_sampler("labor-exp3")``:
    the replayed pass draws with the sampler and leaves the EXP3 rows alone."""
    from bliss_gnn_amd.train import GraphedEvalStep
    gA, sA, mA, va = _trained(cuda, "labor-exp3", "device", False)
    gB, sB, mB, _ = _trained(cuda, "labor-exp3", "device", False)
    assert type(sA).__name__ == "BanditLaborSampler"
    assert all(torch.equal(p, q) for p, q in zip(mA.parameters(), mB.parameters()))
    es = GraphedEvalStep(gA, sA, mA, 128, False)
    for rep in range(2):                                                          # the second pass reuses the graph
        rows = sA._w_pos.clone()
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
        assert torch.equal(rows.view(torch.int16), sA._w_pos.view(torch.int16))
        assert torch.equal(sA._w_pos.view(torch.int16), sB._w_pos.view(torch.int16))
    assert es.captures == 1 and es.fallbacks == 0
    es.close()


def test_fit_graphed_is_fit_eager_bit_for_bit(cuda):
    """tests/test_gpu_fit_graphed.py's comparison for ``"labor-exp3"`` over two epochs."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    out, state = {}, {}
    for kind in ("eager", "graphed"):
        g, tr, va, te = fit_task(cuda)
        g.edata["w"] = bg.normalized_edata(g)
        sampler = fit.make_sampler("labor-exp3", [5, 5, 5], eta=0.4)
        assert type(sampler) is fit.BanditLaborSampler
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
        torch.manual_seed(11)
        out[kind] = fit.fit(g, sampler, model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=2, eval_step="eager", train_metric=True,
                            train_step=kind)
        sampler.check_errors()
        state[kind] = dict(params=[q.detach().contiguous().view(torch.int16).clone() for q in model.parameters()],
                           rng=torch.get_rng_state(), draw=sampler.draw_step(), exp3=sampler._w_pos.view(torch.int16).clone())
    e, gr = out["eager"], out["graphed"]
    print([h["train_loss"] for h in gr["history"]], [h["train_loss"] for h in e["history"]], gr["history"][-1]["sampled_nodes"])
    assert len(gr["history"]) == len(e["history"]) == 2 and gr["steps"] == e["steps"] == 2 * 14
    for hg, he in zip(gr["history"], e["history"]):
        for k in ("epoch", "train_loss", "val_acc", "val_loss", "lr", "train_acc"):
            assert hg[k] == he[k], (k, hg, he)
    assert gr["best_val_acc"] == e["best_val_acc"] and gr["final"] == e["final"]
    sg, se = state["graphed"], state["eager"]
    assert all(torch.equal(a, b) for a, b in zip(sg["params"], se["params"]))
    assert torch.equal(sg["rng"], se["rng"]) and sg["draw"] == se["draw"]
    assert torch.equal(sg["exp3"], se["exp3"]) and not bool((sg["exp3"] == sg["exp3"].flatten()[0]).all())      # the rows moved


def test_pipelined_step_refuses_the_samplers(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g, _, _ = _step_task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    for s in (fit.BanditLaborSampler(FAN), fit.WeightedLaborSampler(FAN, "w")):
        with pytest.raises(NotImplementedError):
            PipelinedTrainStep(g, s, model, BS)
        with pytest.raises(NotImplementedError):                                  # no split enqueue either
            s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), part="main", external_rng=True)
        with pytest.raises(NotImplementedError):
            s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), chain_rng=True)
