"""GPU suite (-m gpu): the multinomial samplers with ``draw="device"`` through the classes -- against the oracle driven in the
same mode (the drawn set restated from the traced keys by tests/mn_draw_ref.py), replayed from a HIP graph against the eager
step, and the refusals of what the device draw does not cover."""
import numpy as np
import pytest
import torch

import mn_draw_ref as ref
from conftest import bf16_bits

pytestmark = pytest.mark.gpu

V, E, GSEED, BS, FAN = 6000, 100000, 51, 48, [300, 150, 80]
DRAW_SEED = 977


@pytest.fixture(scope="module")
def graph_cpu():
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=GSEED)
    feats = torch.randn(V, 32, generator=torch.Generator().manual_seed(2)).bfloat16()
    labels = torch.randint(0, 4, (V,), generator=torch.Generator().manual_seed(3))
    return ip, ix, ei, feats, labels


def _graph(graph_cpu, cuda):
    import bliss_gnn_amd as bg
    ip, ix, ei, feats, labels = graph_cpu
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    return g


def _sampler(kind, **kw):
    import bliss_gnn_amd as bg
    if kind == "bandit":
        s = bg.BanditLadiesSampler(FAN, eta=0.1, node_embedding="features", **kw)
    else:
        s = bg.LadiesSampler(FAN, importance_sampling=kind == "ladies", **kw)
    if kw.get("draw") == "device":
        s.reset_draw(seed=DRAW_SEED)
    return s


def _ulp_apart(a, b):
    return np.abs(a.view(np.uint32).astype(np.int64) - b.view(np.uint32).astype(np.int64)).max(initial=0)


@pytest.mark.parametrize("kind", ["bandit", "ladies", "ladies_uniform"])
def test_device_draw_matches_the_oracle_in_the_same_mode(cuda, graph_cpu, kind):
    """Two steps with draw="device".  Per layer the keys restated from the ORACLE's p and candidate ids are within one ulp of the
    traced device keys; the oracle's expand_frontier / importance / generate_block, driven with chosen = select(traced keys, k),
    give bit-identical blocks (and, for the bandit, EXP3 weights after exp3)."""
    import bliss_gnn_amd as bg
    from oracle import bliss_oracle as bo
    ip, ix, ei = graph_cpu[:3]
    g = _graph(graph_cpu, cuda)
    og = bo.CSC(ip, ix, ei)
    edge_w = bo.normalized_edata(og)
    bandit, imp = kind == "bandit", kind != "ladies_uniform"
    s = _sampler(kind, draw="device")
    o_w = torch.ones(len(FAN), og.num_edges, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(8)
    for step in range(2):
        seeds = torch.arange(30 * step, 30 * step + BS, dtype=torch.int32)
        _, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        assert s.draw_step() == step + 1
        o_blocks, seed_nodes = [], seeds.to(torch.int64)
        for n, block_id in enumerate(reversed(range(len(FAN)))):
            blk = blocks[block_id]
            fr = bo.expand_frontier(og, seed_nodes)
            if bandit:
                W, _ = bo.exp3_edge_prob(og, fr, o_w[block_id], 0.1)
                p, _ = bo.bandit_node_importance(fr, W, imp)
            else:
                W = edge_w[fr.eid]
                p, _ = bo.ladies_node_importance(fr, W, imp)
            tr = blk._trace
            assert np.array_equal(tr["cand_nid"].cpu().numpy(), fr.nid.numpy().astype(np.int32))
            assert np.array_equal(bf16_bits(tr["p"]), bf16_bits(p.bfloat16()))
            dev_keys = tr["keys"].cpu().numpy()
            want = ref.keys(p.bfloat16(), fr.nid.numpy(), DRAW_SEED, step, n)
            assert np.array_equal(np.isposinf(dev_keys), np.isposinf(want)) and _ulp_apart(dev_keys, want) <= 1
            chosen = torch.from_numpy(ref.select(dev_keys, FAN[block_id]))
            ob = bo.generate_block(og, fr, chosen, p, W, hajek=bandit)
            assert np.array_equal(ob.indptr.numpy(), blk.indptr.cpu().numpy())
            assert np.array_equal(ob.src.numpy(), blk.src.cpu().numpy()) and np.array_equal(ob.dst.numpy(), blk.dst.cpu().numpy())
            assert np.array_equal(ob.eid.numpy(), blk.edata[bg.EID].cpu().numpy())
            assert np.array_equal(ob.src_nid.numpy(), blk.srcdata[bg.NID].cpu().numpy())
            assert np.array_equal(bf16_bits(ob.edge_weights), bf16_bits(blk.edata["edge_weights"]))
            if bandit:
                assert np.array_equal(bf16_bits(ob.q_ij), bf16_bits(blk.edata["q_ij"]))
                assert np.array_equal(bf16_bits(ob.node_prob), bf16_bits(blk.srcdata["node_prob"]))
            seed_nodes = ob.src_nid
            o_blocks.insert(0, ob)
        if bandit:
            en = []
            for b, ob in zip(blocks, o_blocks):
                e_ = (torch.rand(ob.n_src, generator=gen) * 20).bfloat16()
                b.srcdata["embed_norm"] = e_.to(cuda)
                en.append(e_)
            s.exp3(blocks, g)
            s.check_errors()
            o_w, _ = bo.exp3(og, o_blocks, o_w, edge_w, en)
            assert np.array_equal(bf16_bits(s.exp3_weights), bf16_bits(o_w))


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_static_blocks_match_the_exact_size_path(cuda, graph_cpu, kind):
    """sample_blocks_static with the device draw: the capacity-padded blocks, trimmed, are the blocks of sample_blocks for the
    same draw state; the K capacity is the exact bound fanout + S."""
    import bliss_gnn_amd as bg
    g3, g4 = _graph(graph_cpu, cuda), _graph(graph_cpu, cuda)
    s3, s4 = _sampler(kind, draw="device"), _sampler(kind, draw="device")
    seeds = torch.arange(100, 100 + BS, dtype=torch.int32, device=cuda)
    s4.sample_blocks(g4, seeds)                                  # binds the engine, learns default capacities
    s4.reset_draw(seed=DRAW_SEED, step=0)
    _, _, exact = s3.sample_blocks(g3, seeds)
    _, _, padded = s4.sample_blocks_static(g4, seeds)
    torch.cuda.synchronize()
    cnts = s4.finish_static()
    assert s3.draw_step() == s4.draw_step() == 1
    caps = s4._engine.caps
    for n, c in enumerate(caps):
        assert c["K"] >= min(V, FAN[len(FAN) - 1 - n] + c["S"])
    for be, bp, c in zip(exact, padded, reversed(cnts)):
        K, B, S = c.K, c.B, c.S
        assert (S, K, B) == (be.num_dst_nodes(), be.num_src_nodes(), be.num_edges())
        assert torch.equal(bp.indptr[:S + 1], be.indptr) and torch.equal(bp.src[:B], be.src) and torch.equal(bp.dst[:B], be.dst)
        assert torch.equal(bp.srcdata[bg.NID][:K], be.srcdata[bg.NID])
        assert torch.equal(bp.edata["edge_weights"][:B].view(torch.int16), be.edata["edge_weights"].view(torch.int16))


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_graphed_step_matches_the_eager_step(cuda, graph_cpu, kind):
    """Two identically seeded sampler / model pairs.  A: TrainStep with draw="device".  B: GraphedTrainStep on the same loader with
    the same number of sampler calls (calibrate 3, warm-up 2, capture, 4 replays = 10).  Loss, parameters and EXP3 weights are
    bit-identical afterwards, draw_step() is the number of sampler calls on both sides, torch's generator is untouched, and
    finish_static never reports a capacity error (it would raise)."""
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep
    ids = torch.arange(V, dtype=torch.int32, device=cuda)

    def build():
        g = _graph(graph_cpu, cuda)
        s = _sampler(kind, draw="device")
        torch.manual_seed(0)
        model = SAGE(32, 16, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        return g, s, model

    g1, s1, m1 = build()
    eager = TrainStep(g1, s1, m1)
    l1 = BatchLoader(ids, BS, seed=5).forever()
    g2, s2, m2 = build()
    graphed = GraphedTrainStep(g2, s2, m2, BS)
    l2 = BatchLoader(ids, BS, seed=5).forever()
    torch.manual_seed(9)
    rng0 = torch.get_rng_state()
    graphed.calibrate(l2, steps=3)
    graphed.capture(l2, warmup=2)
    for _ in range(4):
        loss2 = graphed(next(l2))
    assert torch.equal(torch.get_rng_state(), rng0), "the device draw must not touch torch's CPU generator (graphed step)"
    for _ in range(3):                                           # the calibration's sampler calls train nothing
        s1.sample_blocks(g1, next(l1))
    for _ in range(7):
        loss1 = eager(next(l1))
    assert torch.equal(torch.get_rng_state(), rng0), "the device draw must not touch torch's CPU generator (eager step)"
    assert s1.draw_step() == s2.draw_step() == 10
    sizes1 = [(b._counts.S, b._counts.E, b._counts.C, b._counts.K, b._counts.B) for b in reversed(eager.last["mfgs"])]
    sizes2 = [(c.S, c.E, c.C, c.K, c.B) for c in graphed.last_counts]
    print("sizes eager", sizes1, "graphed", sizes2, "loss", float(loss1), float(loss2))
    assert sizes1 == sizes2
    assert float(loss1) == float(loss2)
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p1.view(torch.int16), p2.view(torch.int16))
    if kind == "bandit":
        s1.check_errors(); s2.check_errors()
        assert torch.equal(s1.exp3_weights.view(torch.int16), s2.exp3_weights.view(torch.int16))
    graphed.close()


def test_device_draw_leaves_the_torch_generator_alone(cuda, graph_cpu):
    from bliss_gnn_amd import NID
    g = _graph(graph_cpu, cuda)
    s = _sampler("bandit", draw="device")
    torch.manual_seed(123)
    before = torch.get_rng_state()
    seeds = torch.arange(BS, dtype=torch.int32, device=cuda)
    _, _, b1 = s.sample_blocks(g, seeds)
    assert torch.equal(torch.get_rng_state(), before)
    # the draw is a function of (seed, step): the same state draws the same blocks, the next step others
    _, _, b2 = s.sample_blocks(g, seeds)
    s.reset_draw(seed=DRAW_SEED, step=0)
    _, _, b3 = s.sample_blocks(g, seeds)
    assert torch.equal(b1[0].srcdata[NID], b3[0].srcdata[NID]) and not torch.equal(b1[0].srcdata[NID], b2[0].srcdata[NID])
    # seed=None: torch.initial_seed() at first use
    s.reset_draw()
    torch.manual_seed(DRAW_SEED)
    _, _, b4 = s.sample_blocks(g, seeds)
    assert torch.equal(b1[0].srcdata[NID], b4[0].srcdata[NID]) and s.draw_step() == 1


def test_refusals(cuda, graph_cpu):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import PipelinedTrainStep
    g = _graph(graph_cpu, cuda)
    seeds = torch.arange(BS, dtype=torch.int32, device=cuda)
    for kind in ("bandit", "ladies"):
        s = _sampler(kind)                                       # default draw: the host's torch.multinomial, no static variant
        assert s.draw == "host"
        s.sample_blocks(g, seeds)
        with pytest.raises(NotImplementedError):
            s.sample_blocks_static(g, seeds)
    with pytest.raises(NotImplementedError):
        bg.BanditLadiesSampler(FAN, replace=True, draw="device")
    with pytest.raises(NotImplementedError):
        bg.LadiesSampler(FAN, replace=True, draw="device")
    with pytest.raises(ValueError):
        bg.LadiesSampler(FAN, draw="gpu")
    s = fit.make_sampler("bandit", FAN, draw="device")
    assert isinstance(s, bg.BanditLadiesSampler) and s.draw == "device"
    assert fit.make_sampler("ladies", FAN, draw="device").draw == "device" and fit.make_sampler("ladies", FAN).draw == "host"
    model = SAGE(32, 16, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    with pytest.raises(NotImplementedError):
        PipelinedTrainStep(g, s, model, BS)
    # the split / external-generator enqueue of the pipelined loop does not exist for the device draw
    s.sample_blocks(g, seeds)
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, seeds, external_rng=True)
