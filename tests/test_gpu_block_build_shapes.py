"""GPU suite (-m gpu): the block build (csrc/sampler.hip: k_block_pass1 -> k_block_scans -> k_block_pass2 -> k_tr_sort_lists) at its
edge shapes and on multigraphs, through the public samplers, over the fixtures of tests/block_build_ref.py (whose content
tests/test_block_build_ref.py pins on the CPU):

  * the block's arrays and counts against the oracle, bit for bit;
  * the sampler-built by-source index (Block._transposed, what every backward pass gathers through) against its definition,
    the stable argsort of src -- compared on the host BEFORE any kernel consumes it;
  * by-source lists on both sides of the 64-edge switch of k_tr_sort_lists, lists with parallel edges on either path, seed
    counts around the bitmap's word (32) and group (2048) edges, a second layer whose seed capacity is not its seed count,
    frontier lengths around the block passes' chunk (1024) and span (256), everything kept (four trips of pass 1's loop) and
    a sparse planted draw (one trip, empty spans), empty columns;
  * the static path and a captured graph, alternating two seed lists so that a slot left from the previous run shows;
  * the split enqueue of PipelinedTrainStep (the sort behind k_cleanup and the ready flag);
  * SpMM and GATv2 forward / backward over the 134-edge list with its parallel edges, per element against fp64."""
import numpy as np
import pytest
import torch

import block_build_ref as bb
import mn_draw_ref
from bounds import SPMM_K, assert_within, check_gat_layer, spmm_terms

pytestmark = pytest.mark.gpu


def _bg():
    import bliss_gnn_amd as bg
    return bg


def _graph(case, dev, ndata=None):
    bg = _bg()
    og = case.og
    g = bg.Graph(og.indptr.to(dev), og.indices.to(dev), og.eid.to(dev), ndata=ndata)
    g.edata["w"] = bg.normalized_edata(g)
    return g


def _sampler(kind, fanouts, **kw):
    bg = _bg()
    if kind == "bandit":
        return bg.PoissonBanditLadiesSampler(fanouts, eta=bb.ETA, **kw)
    return bg.PoissonLadiesSampler(fanouts, **kw)


def _bits(t):
    t = t.detach().cpu()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _check_index(ti, te, src, K, B, want, what):
    """Host-side, before anything consumes the index: t_indptr[:K + 1] and t_edge[:B] are exactly the expectation."""
    w_ip, w_e = want
    assert w_e.numel() == B and w_ip.numel() == K + 1, what
    got_ip, got_e = ti[:K + 1].cpu().long(), te[:B].cpu().long()
    assert torch.equal(got_ip, w_ip), what + ": t_indptr"
    bad = (got_e != w_e).nonzero().flatten()
    assert bad.numel() == 0, "%s: %d of %d t_edge slots differ from the stable argsort of src, first at %d" % (what, bad.numel(), B, int(bad[0]))


def _check_block(b, ob, want, bandit, what):
    bg = _bg()
    c = b._counts
    assert c.err == 0, what
    assert (c.S, c.E, c.C, c.K, c.B) == (ob.n_dst, ob.trace["E"], ob.trace["cand_nid"].numel(), ob.n_src, ob.src.numel()), what
    assert c.c == ob.trace["c"], what
    assert torch.equal(b.indptr.cpu().long(), ob.indptr), what
    assert torch.equal(b.src.cpu().long(), ob.src) and torch.equal(b.dst.cpu().long(), ob.dst), what
    assert torch.equal(b.edata[bg.EID].cpu().long(), ob.eid), what
    assert torch.equal(b.srcdata[bg.NID].cpu().long(), ob.src_nid), what
    assert torch.equal(_bits(b.edata["edge_weights"]), _bits(ob.edge_weights)), what
    if bandit:
        assert torch.equal(_bits(b.edata["q_ij"]), _bits(ob.q_ij)), what
        assert torch.equal(_bits(b.srcdata["node_prob"]), _bits(ob.node_prob)), what
    assert b._transposed is not None, "the sampler builds the index of every layer with a seed capacity <= 32768"
    _check_index(b._transposed[0], b._transposed[1], b.src, c.K, c.B, want, what)


def _sample_and_check(key, kind, dev):
    case = bb.CASES[key]()
    g = _graph(case, dev)
    s = _sampler(kind, case.fanouts)
    torch.manual_seed(0)
    inp, _, blocks = s.sample_blocks(g, case.seeds.to(dev), uniforms=case.uniforms)
    s.check_errors()
    o_inp, _, o_blocks = bb.oracle_blocks(key, kind)
    assert torch.equal(inp.cpu().long(), o_inp)
    assert len(blocks) == len(o_blocks)
    for l, (b, ob, want) in enumerate(zip(blocks, o_blocks, bb.expected_of(key, kind))):
        _check_block(b, ob, want, kind == "bandit", "%s %s block %d" % (key, kind, l))
    return g, s, blocks


@pytest.mark.parametrize("key", bb.ALL_KEPT)
def test_everything_kept_bandit(cuda, key):
    """PoissonBanditLadiesSampler with fanout >= C (the all_one route, deterministic): list lengths 1 .. 130 and the lists with
    parallel edges ('lists'), S = 31 .. 4100 ('S<n>'), frontiers of 255 .. 1025 edges ('E<n>': every full span compacts 256
    kept edges), empty columns first / middle / last ('empty')."""
    _sample_and_check(key, "bandit", cuda)


@pytest.mark.parametrize("key", ["lists", "S33", "S2049", "E1024", "empty"])
def test_everything_kept_ladies(cuda, key):
    """PoissonLadiesSampler: k_block_pass1<false> / k_block_pass2<false> over the same shapes."""
    _sample_and_check(key, "ladies", cuda)


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_sparse_planted_draw(cuda, kind):
    """Planted uniforms (0.0 for the special sources, 1.0 for the hub column's cold sources, seeded random numbers for the
    rest; the oracle gets the same vector): about 5 % of the frontier kept, one trip of pass 1's loop, whole spans empty."""
    _sample_and_check("sparse", kind, cuda)


def test_two_layers(cuda):
    """[f, f]: the second-sampled layer's seeds are the first one's kept nodes, its seed capacity (which sizes the bitmap of
    k_tr_sort_lists) is the first layer's kept CAPACITY; a source that is no candidate of the first layer reaches 70 of them,
    one twice."""
    _, s, blocks = _sample_and_check("two_layer", "bandit", cuda)
    caps = s._engine.caps
    assert caps[1]["S"] == caps[0]["K"] and caps[1]["S"] != blocks[0]._counts.S


@pytest.mark.parametrize("key", ["lists", "sparse"])
def test_atomic_candidate_passes(cuda, monkeypatch, key):
    """BLISS_BINS=0: no per-seed coefficients (seed_coef is null), the block passes compute edge_q instead of edge_q_pre."""
    monkeypatch.setenv("BLISS_BINS", "0")
    _, s, _ = _sample_and_check(key, "bandit", cuda)
    assert s._engine.n_bins == 0


def test_multinomial_device_draw(cuda):
    """BanditLadiesSampler(draw='device') with fanout < C on the 'lists' graph: the same bliss_build_block, with undrawn seeds
    present as sources without edges.  The oracle's generate_block is driven with the set the traced device keys select
    (tests/mn_draw_ref.py, like tests/test_gpu_mn_sampler.py)."""
    from oracle import bliss_oracle as bo
    bg = _bg()
    case = bb.lists_case()
    fan, seed = 200, 977
    g = _graph(case, cuda)
    s = bg.BanditLadiesSampler([fan], eta=bb.ETA, draw="device")
    s.reset_draw(seed=seed)
    _, _, (blk,) = s.sample_blocks(g, case.seeds.to(cuda))
    s.check_errors()
    og = case.og
    fr = bo.expand_frontier(og, case.seeds.long())
    W, _ = bo.exp3_edge_prob(og, fr, torch.ones(og.num_edges, dtype=torch.bfloat16), bb.ETA)
    p, _ = bo.bandit_node_importance(fr, W, True)
    assert fr.nid.numel() > fan
    assert np.array_equal(blk._trace["cand_nid"].cpu().numpy(), fr.nid.numpy().astype(np.int32))
    chosen = torch.from_numpy(mn_draw_ref.select(blk._trace["keys"].cpu().numpy(), fan))
    ob = bo.generate_block(og, fr, chosen, p, W, hajek=True)
    ob.trace.update(E=fr.pos.numel(), cand_nid=fr.nid, c=blk._counts.c)
    # what the case is about: undrawn seeds (sources without edges) and long lists with parallel edges are in this block
    out_deg = torch.bincount(ob.src, minlength=ob.n_src)
    assert int((out_deg[:ob.n_dst] == 0).sum()) >= 1
    long_par = 0
    for nm in bb.LONG_PARALLEL:
        e, d = bb.source_list(ob, case.specials[nm][0])
        long_par += int(e.numel() > 64 and d.unique().numel() < d.numel())
    assert long_par >= 2
    _check_block(blk, ob, bb.expected_index(ob.src, ob.n_src), True, "multinomial lists")


def test_static_path_and_graph_replay(cuda):
    """The 'lists' multigraph through sample_blocks_static three times and from one captured graph three times, alternating
    the seed list with its reverse (same sizes, another index): t_indptr and t_edge of EVERY run equal that run's expectation
    -- equal to each other would not do, a slot left from the previous run must show -- and src / dst the oracle's."""
    keys = ["lists", "lists_alt"]
    case = bb.lists_case()
    g = _graph(case, cuda)
    s = _sampler("bandit", case.fanouts)
    seeds = [bb.CASES[k]().seeds.to(cuda) for k in keys]
    torch.manual_seed(9)
    s.sample_blocks(g, seeds[0])                                     # binds the engine, learns the capacities
    eng = s._engine
    buf = seeds[0].clone()

    def run(i, launch):
        buf.copy_(seeds[i % 2])
        torch.manual_seed(9)
        eng.stage_rng_from_torch()
        blocks = launch()
        torch.cuda.synchronize()
        cnts = s.finish_static()
        o_blocks, want = bb.oracle_blocks(keys[i % 2])[2], bb.expected_of(keys[i % 2])
        for b, c, ob, w in zip(reversed(blocks), cnts, reversed(o_blocks), reversed(want)):
            what = "static run %d (%s)" % (i, keys[i % 2])
            assert c.err == 0 and (c.S, c.K, c.B) == (ob.n_dst, ob.n_src, ob.src.numel()), what
            assert torch.equal(b.src[:c.B].cpu().long(), ob.src) and torch.equal(b.dst[:c.B].cpu().long(), ob.dst), what
            _check_index(b._transposed[0], b._transposed[1], b.src, c.K, c.B, w, what)

    for i in range(3):
        run(i, lambda: s.sample_blocks_static(g, buf)[2])
    torch.manual_seed(9)
    eng.stage_rng_from_torch()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = s.sample_blocks_static(g, buf)[2]

    def replay():
        graph.replay()
        return captured
    for i in range(3, 6):
        run(i, replay)


def test_pipelined_split_enqueue(cuda):
    """PipelinedTrainStep on the two-layer multigraph: with device flags (the default) the input layer's block is enqueued as
    the 'last_block' part -- k_tr_sort_lists with do_cleanup = 0, behind k_cleanup and the ready flag.  The index of both
    slots' blocks is the stable argsort of their src, and equals the one of the one-stream sampler on the same seeds."""
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, PipelinedTrainStep
    case = bb.two_layer_case()
    V, S = case.V, case.seeds.numel()
    feats = torch.randn(V, 16, generator=torch.Generator().manual_seed(2)).bfloat16()
    labels = torch.randint(0, 3, (V,), generator=torch.Generator().manual_seed(3))
    g = _graph(case, cuda, ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    s = _sampler("bandit", case.fanouts)
    torch.manual_seed(0)
    model = SAGE(16, 8, 3, 2, torch.relu, 0.0).to(cuda).bfloat16()
    step = PipelinedTrainStep(g, s, model, S)
    loader = BatchLoader(case.seeds.to(cuda), S, seed=5).forever()      # every batch: the fixture's seeds in another order
    torch.manual_seed(9)
    step.calibrate(loader, steps=2)
    step.capture(loader, warmup=1)
    assert step._defer_block0 or not step.use_flags                     # flags usable => the split route was taken
    print("ROUTE pipelined use_flags=%s last_block_part=%s" % (step.use_flags, step._defer_block0))
    step(loader)
    torch.cuda.synchronize()
    s.check_errors()
    g1 = _graph(case, cuda)
    s1 = _sampler("bandit", case.fanouts)
    deep = case.info["deep"]
    for slot in (0, 1):
        seeds = step.seeds2[slot].clone()
        assert sorted(seeds.tolist()) == sorted(case.seeds.tolist())
        torch.manual_seed(1)
        _, _, one_stream = s1.sample_blocks(g1, seeds)
        cnts = step.last_counts2[1 - slot]                               # [slot 1's, slot 0's], each in sampling order
        for l, (b, b1, c) in enumerate(zip(step.mfgs[slot], one_stream, reversed(cnts))):
            what = "pipelined slot %d block %d" % (slot, l)
            assert c.err == 0 and (c.S, c.K, c.B) == (b1._counts.S, b1._counts.K, b1._counts.B), what
            src = b.src[:c.B].cpu().long()
            assert torch.equal(src, b1.src.cpu().long()) and torch.equal(b.dst[:c.B], b1.dst), what
            _check_index(b._transposed[0], b._transposed[1], b.src, c.K, c.B, bb.expected_index(src, c.K), what)
            assert torch.equal(b._transposed[0][:c.K + 1], b1._transposed[0]) and torch.equal(b._transposed[1][:c.B], b1._transposed[1][:c.B])
        b0, c0 = step.mfgs[slot][0], cnts[-1]                            # the planted 71-edge list with its repeat is in the input block
        loc = int((b0.srcdata[_bg().NID][:c0.K] == deep).nonzero())
        d = b0.dst[:c0.B][b0.src[:c0.B] == loc]
        assert d.numel() == 71 and d.unique().numel() == 70
    step.drain()
    step.close()


@pytest.fixture(scope="module")
def lists_block(cuda):
    """The all-kept 'lists' block; its arrays and its index are checked against the oracle on the host first, so that no
    consumer below is launched on a wrong index."""
    _, _, (blk,) = _sample_and_check("lists", "bandit", cuda)
    return blk


def test_spmm_over_parallel_edges(cuda, lists_block):
    """weighted_aggregate forward and backward on the block with the 134-edge source (four of its destinations twice): per
    element against fp64 built from the ORACLE's src / dst -- a parallel edge contributes twice to both -- with the project's
    SPMM_K, which holds for rows up to 16 384 edges."""
    from bliss_gnn_amd.nn import weighted_aggregate
    blk = lists_block
    ob = bb.oracle_blocks("lists")[2][0]
    K, S, B = ob.n_src, ob.n_dst, ob.src.numel()
    assert int(torch.bincount(ob.src).max()) >= 134
    src, dst = ob.src.to(cuda), ob.dst.to(cuda)
    gen = torch.Generator().manual_seed(4)
    w = blk.edata["edge_weights"]
    for dim, mean, wt in ((41, True, True), (64, False, True), (64, True, False)):
        h = torch.randn(K, dim, generator=gen).bfloat16().to(cuda).requires_grad_(True)
        gout = torch.randn(S, dim, generator=gen).bfloat16().to(cuda)
        out = weighted_aggregate(blk, h, w if wt else None, mean=mean)
        out.backward(gout)
        ref, mag = spmm_terms(src, dst, S, h.detach(), w if wt else None, mean)
        rb, mb = spmm_terms(src, dst, S, gout, w if wt else None, mean, by_src=True, n_out=K)
        case = "lists d%d %s %s" % (dim, "mean" if mean else "sum", "w" if wt else "1")
        r1 = assert_within(out, ref, mag, *SPMM_K["bf16"], "spmm out " + case)
        r2 = assert_within(h.grad, rb, mb, *SPMM_K["bf16"], "spmm d h " + case)
        print("RATIO %s out %.3f dh %.3f" % (case, r1, r2))


@pytest.mark.parametrize("mode", ["1", "0"])
def test_gat_over_parallel_edges(cuda, monkeypatch, lists_block, mode):
    """One GATv2Conv forward and backward on the same block, fused (BLISS_GAT_FUSED=1) and separate (0) kernels, through
    bounds.check_gat_layer (fp64 autograd over the block's src / dst, which the fixture has already compared with the
    oracle's)."""
    from bliss_gnn_amd.nn import GATv2Conv
    blk = lists_block
    fin, H, D = 40, 4, 16
    K = blk.num_src_nodes()
    monkeypatch.setenv("BLISS_GAT_FUSED", mode)
    torch.manual_seed(5)
    layer = GATv2Conv(fin, D, H, 0.0, 0.0, 0.2, False, None, bias=False, share_weights=True, allow_zero_in_degree=True).to(cuda).bfloat16()
    h = (torch.randn(K, fin, generator=torch.Generator().manual_seed(6)) * 0.5).bfloat16().to(cuda).requires_grad_(True)
    cap = {}

    def keep(m, i, o):
        cap["feat"] = o
        o.retain_grad()
    hook = layer.fc_src.register_forward_hook(keep)
    out, e = layer(blk, h, get_attention=True)
    hook.remove()
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).bfloat16().to(cuda)
    (out * gout).float().sum().backward()
    r = check_gat_layer(layer, blk, h, out, e, gout, cap["feat"].detach(), cap["feat"].grad, "lists gat mode %s" % mode)
    print("RATIO lists-gat-mode%s %s" % (mode, " ".join("%s %.3f" % kv for kv in r.items())))
