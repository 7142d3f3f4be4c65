"""GPU suite (-m gpu): the node-wise bandit sampler (fit.BanditNeighborSampler) as a sampler loop against the
oracle's EXP3 update, inside the train steps -- captured into a HIP graph and replayed --, through ``fit.fit``, and refused by the
pipelined loop; ``NeighborSampler(draw="device", prob=...)`` beside it."""
import math

import numpy as np
import pytest
import torch

import wneighbor_ref as ref
from conftest import bf16_bits
from oracle import bliss_oracle as bo
from test_gpu_fit import _task as fit_task

pytestmark = pytest.mark.gpu

FAN, BS, DRAW_SEED = [8, 4, 4], 128, 31


def _oblock(blk):
    import bliss_gnn_amd as bg
    c = lambda t: t.cpu().long()
    return bo.OBlock(blk.num_src_nodes(), blk.num_dst_nodes(), c(blk.indptr), c(blk.src), c(blk.dst), c(blk.edata[bg.EID]),
                     blk.edata["edge_weights"].cpu(), blk.edata["q_ij"].cpu(), torch.ones(blk.num_src_nodes()).bfloat16(),
                     c(blk.srcdata["_ID"]), c(blk.dstdata["_ID"]))


@pytest.mark.parametrize("model", ["sage", "gat"])
def test_sampler_loop_against_the_oracles_exp3(cuda, model):
    """Two steps: the blocks' q_ij are exp3_edge_prob on the CURRENT rows (so the sampler reads what the update wrote), rewards and
    exp3_weights are the oracle's bit for bit."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(3000, 50000, seed=3)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda))
    g.edata["w"] = bg.normalized_edata(g)
    og = bo.CSC(ip, ix, ei)
    edge_w = bo.normalized_edata(og)
    fan, eta = [5, 3], 0.4
    s = fit.BanditNeighborSampler(fan, eta=eta, model=model, seed=DRAW_SEED)
    gen = torch.Generator().manual_seed(4)
    o_w = torch.ones(2, og.num_edges, dtype=torch.bfloat16)
    ipn = ip.numpy()
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
            assert np.array_equal(bf16_bits(blk.edata["q_ij"]), bf16_bits(torch.from_numpy(q_pos[blk.pos.cpu().numpy()]).bfloat16()))
            deg = ipn[cur.numpy() + 1] - ipn[cur.numpy()]
            assert np.array_equal(np.diff(blk.indptr.cpu().numpy()), np.minimum(deg, fan[b]))
            assert bool((blk.srcdata["node_prob"] == 1).all())
            # the Hajek weights of these q: each column's sum is its kept count
            w = blk.edata["edge_weights"].float().cpu().numpy()
            for c in range(blk.num_dst_nodes()):
                o, e = int(blk.indptr[c]), int(blk.indptr[c + 1])
                if deg[c] <= fan[b]:
                    assert (w[o:e] == 1).all()
                else:
                    want = ref.hajek_weights(q_pos[blk.pos[o:e].cpu().numpy()], False)
                    assert np.abs(bf16_bits(torch.from_numpy(w[o:e]).bfloat16()).astype(np.int64)
                                  - ref.bf16_bits(want).astype(np.int64)).max() <= 1
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
    assert not torch.equal(o_w, torch.ones_like(o_w))                             # (the second step drew from updated rows)


def _step_task(cuda):
    import bliss_gnn_amd as bg
    g, tr, va, _ = fit_task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    return g, tr, va


def test_graphed_step_replays_the_bandit_sampler(cuda):
    """tests/test_gpu_neighbor_step.py's arrangement with an eager twin: A = GraphedTrainStep (calibrate 3, warm-up 2, the captured
    step, 6 replays), B = the same 3 sampler calls, then 9 eager TrainStep calls from the same seeds and draw state.  The losses of
    the replayed steps, the parameters and the EXP3 rows are bit-identical; the draw step advances by one per replay."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, GraphedEvalStep, GraphedTrainStep, TrainStep

    def build():
        g, tr, va = _step_task(cuda)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        return g, fit.BanditNeighborSampler(FAN, eta=0.4, seed=DRAW_SEED), model, BatchLoader(tr, BS, seed=5).forever(), va

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
    # replay hygiene of the engine's own scratch
    eng = s1._engine
    words = -(-(-(-g1.num_nodes() // 32)) // 1024) * 1024
    assert int(eng._wn_scr[:16 + words].abs().sum()) == 0 and eng._nb_scr is None
    for st in eng._sets.values():
        assert bool((st["kept_map"] == -1).all())
    # a replayed validation pass draws with the sampler and leaves the EXP3 rows alone
    es = GraphedEvalStep(g1, s1, m1, BS, False)
    before, d0 = s1.exp3_weights.clone(), s1.draw_step()
    acc, _ = es.run(va)
    assert 0.0 <= acc <= 1.0 and s1.draw_step() > d0 and es.captures == 1
    assert torch.equal(before.view(torch.int16), s1.exp3_weights.view(torch.int16))
    es.close()


@pytest.mark.parametrize("kind", ["neighbor-exp3", "prob"])
def test_fit_runs_the_weighted_samplers(cuda, kind):
    """tests/test_gpu_fit.py's task and assertions."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = fit_task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    if kind == "neighbor-exp3":
        sampler = fit.make_sampler("neighbor-exp3", [5, 5], eta=0.4)
        assert type(sampler) is fit.BanditNeighborSampler
    else:
        sampler = fit.NeighborSampler([5, 5], draw="device", prob="w")
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 2, torch.relu, 0.1).to(cuda).bfloat16()
    seen = []
    out = fit.fit(g, sampler, model, tr, va, te, batch_size=128, lr=0.01, max_epochs=4, log=seen.append)
    assert len(out["history"]) == 4 and out["steps"] == 4 * (1800 // 128)
    assert out["history"][-1]["train_loss"] < out["history"][0]["train_loss"]     # it learns
    assert out["best_val_acc"] > 0.3 and set(out["final"]) == {"Train", "Validation", "Test"}
    assert out["final"]["Test"] > 0.3                                             # 4 classes: chance is 0.25
    assert seen == out["history"]
    sampler.check_errors()
    if kind == "neighbor-exp3":
        w = sampler.exp3_weights
        assert w.shape == (2, g.num_edges()) and not torch.equal(w, torch.ones_like(w))


def test_prob_changes_the_draw_and_carries_q(cuda):
    """``prob`` by EDGE ID reaches the kernel by position: an edge with probability 0 is never drawn from a column that has enough
    positive ones, q_ij is the given probability, and the blocks differ from the uniform draw's."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    g, tr, _, _ = fit_task(cuda)
    E = g.num_edges()
    p = torch.rand(E, generator=torch.Generator().manual_seed(8)).bfloat16()
    p[torch.randperm(E, generator=torch.Generator().manual_seed(9))[:E // 3]] = 0.0
    g.edata["p"] = p.to(cuda)
    sw = fit.NeighborSampler([4, 4], seed=DRAW_SEED, draw="device", prob="p")
    su = fit.NeighborSampler([4, 4], seed=DRAW_SEED, draw="device")
    _, _, bw = sw.sample_blocks(g, tr[:BS])
    _, _, bu = su.sample_blocks(g, tr[:BS])
    assert bool((bu[-1].edata["edge_weights"] == 1).all())
    assert not torch.equal(bw[-1].pos, bu[-1].pos)
    for blk in bw:
        q = blk.edata["q_ij"]
        assert torch.equal(q.view(torch.int16), g.edata["p"][blk.edata[bg.EID].long()].view(torch.int16))
        dst = blk.dstdata["_ID"].long()
        p_pos = g.by_position(g.edata["p"])
        n_pos = torch.zeros(dst.numel(), dtype=torch.int64, device=cuda)
        for c in range(dst.numel()):
            n_pos[c] = int((p_pos[int(g.indptr[dst[c]]):int(g.indptr[dst[c] + 1])] > 0).sum())
        zero_kept = torch.zeros(dst.numel(), dtype=torch.int64, device=cuda).index_add_(0, blk.dst.long(), (q == 0).long())
        kept = blk.indptr[1:].long() - blk.indptr[:-1].long()
        assert bool((zero_kept == (kept - torch.minimum(kept, n_pos))).all())     # zeros only as fillers


def test_pipelined_step_and_the_host_draw_refuse(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g, _, _ = _step_task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    for s in (fit.BanditNeighborSampler(FAN), fit.NeighborSampler(FAN, draw="device", prob="w")):
        with pytest.raises(NotImplementedError):
            PipelinedTrainStep(g, s, model, BS)
        with pytest.raises(NotImplementedError):                                  # no split enqueue either
            s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), part="main", external_rng=True)
        with pytest.raises(NotImplementedError):
            s.sample_blocks_static(g, torch.arange(BS, dtype=torch.int32, device=cuda), chain_rng=True)
    with pytest.raises(NotImplementedError):
        fit.NeighborSampler(FAN, draw="host", prob="w")
