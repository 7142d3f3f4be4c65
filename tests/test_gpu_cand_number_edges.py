"""GPU suite (-m gpu): k_bitmap_tiles, k_cand_number and the Poisson scale fused into it (csrc/sampler.hip) on crafted graphs,
through the public samplers, one sampling layer each, against bo.sample_blocks_bandit and bo.sample_blocks_ladies bit for bit:

  chunk edges   the seeds' columns have all-distinct sources, so that C is exactly 1024, 1025, 64 * 1024 + 1, 65 * 1024 + 1;
  tile edges    a frontier of 270 270 positions whose first appearances include positions 131 071 | 131 072 and 262 143 | 262 144,
                the edges of k_bitmap_tiles' tiles (4096 words x 32 bits); 131 071 is also the last bit of its bitmap word;
  high / zero   a CSC without self loops: one source is the only in-neighbour of five seeds (p = sqrt(5) >= 2: the global-atomic
                histogram branch of k_cand_number), another one's fraction is below 2^-22 (p == 0: the LDS counter of bin 0);
  capacity      the engine's cap_c shrunk below C: k_cand_number's overflow branch, the engine's answer to bit 2.

Every case runs with BLISS_FUSE_SCALE=1 (the scale by k_cand_number's last workgroup), BLISS_FUSE_SCALE=0 (k_poisson_scale as a
launch of its own) and BLISS_BINS=0 (k_cand_finalize): all three must give the oracle's c, iters, all_one, p and blocks."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUTES = [("BLISS_FUSE_SCALE", "1"), ("BLISS_FUSE_SCALE", "0"), ("BLISS_BINS", "0")]
TILE_BITS = 4096 * 32


def _distinct_columns(C, S=16):
    """S seeds whose columns hold C - S distinct non-seed sources in all (+ the self loops): exactly C candidates."""
    from oracle import bliss_oracle as bo
    gen = torch.Generator().manual_seed(C)
    V = C + 100
    cuts = torch.sort(torch.randperm(C - S - 1, generator=gen)[:S - 1] + 1).values
    deg = torch.diff(torch.cat([torch.tensor([0]), cuts, torch.tensor([C - S])]))
    src = torch.randperm(V - S, generator=gen)[:C - S] + S
    dst = torch.repeat_interleave(torch.arange(S), deg)
    og = bo.prepare_graph(src, dst, V)
    return og, torch.randperm(S, generator=gen).to(torch.int32), 0.1, dict(C=C)


def _tile_edges():
    """270 seeds with 1000 listed sources each (column = 1001 frontier positions, the self loop last), sources drawn from a pool of
    100 000 nodes so that about a third of the positions are first appearances; fresh nodes planted on the tile-edge positions."""
    from oracle import bliss_oracle as bo
    gen = torch.Generator().manual_seed(77)
    S, D, POOL = 270, 1000, 100000
    src = torch.stack([torch.randperm(POOL, generator=gen)[:D] + S for _ in range(S)])
    marks = [TILE_BITS - 1, TILE_BITS, 2 * TILE_BITS - 1, 2 * TILE_BITS]
    for i, fp in enumerate(marks):
        col, k = divmod(fp, D + 1)
        assert k < D                                                    # not the self loop
        src[col, k] = S + POOL + i
    og = bo.prepare_graph(src.flatten(), torch.repeat_interleave(torch.arange(S), D), S + POOL + len(marks))
    return og, torch.arange(S, dtype=torch.int32), 0.1, dict(first=marks)


def _high_and_zero():
    from oracle import bliss_oracle as bo
    gen = torch.Generator().manual_seed(5)
    V, S, H, Z = 3000, 40, 2999, 2998
    cols = [torch.tensor([H])] * 5
    for i in range(5, S):
        cols.append(torch.randperm(2950, generator=gen)[:8 + i] + S)
    cols[5][3] = Z
    indptr = torch.zeros(V + 1, dtype=torch.int64)
    indptr[1:S + 1] = torch.cumsum(torch.tensor([c.numel() for c in cols]), 0)
    indptr[S + 1:] = indptr[S]
    indices = torch.cat(cols).to(torch.int32)
    og = bo.CSC(indptr, indices, torch.randperm(indices.numel(), generator=gen).to(torch.int32))
    return og, torch.arange(S, dtype=torch.int32), 2.0 ** -24, dict(tiny_pos=int(indptr[5]) + 3, patterns=True)


CASES = {"C1024": lambda: _distinct_columns(1024), "C1025": lambda: _distinct_columns(1025),
         "C65537": lambda: _distinct_columns(64 * 1024 + 1), "C66561": lambda: _distinct_columns(65 * 1024 + 1),
         "tiles": _tile_edges, "high_zero": _high_and_zero}


@functools.lru_cache(maxsize=None)
def _problem(name):
    """-> graph, seeds, eta, fanout, EXP3 row (by edge id), the oracle's block; the case's own claims asserted on the trace."""
    from oracle import bliss_oracle as bo
    og, seeds, eta, info = CASES[name]()
    gen = torch.Generator().manual_seed(3)
    E = og.num_edges
    w = 0.25 + 0.75 * torch.rand(E, generator=gen)                       # by CSC position
    if "tiny_pos" in info:
        w[info["tiny_pos"]] *= 2.0 ** -50
    w_e = torch.empty(E)
    w_e[og.eid.long()] = w
    rows = w_e.bfloat16()[None]
    fr = bo.expand_frontier(og, seeds)
    fan = int(fr.nid.numel()) // 3
    torch.manual_seed(9)
    o_inp, _, (ob,) = bo.sample_blocks_bandit(og, seeds, [fan], rows, eta)
    C = int(ob.trace["cand_nid"].numel())
    if "C" in info:
        assert C == info["C"]
    if "first" in info:
        src_l, S = ob.trace["src_l"].numpy(), seeds.numel()
        _, first = np.unique(src_l[src_l >= S], return_index=True)
        first = set(np.nonzero(src_l >= S)[0][first].tolist())
        assert all(fp in first for fp in info["first"]) and ob.trace["E"] > 2 * TILE_BITS
    if "patterns" in info:
        bits = ob.trace["p"].view(torch.int16).to(torch.int32) & 0xFFFF
        assert int(bits[seeds.numel():].min()) == 0 and int(bits.max()) >= 0x4000 and int(bits.max()) < 0x7F80
    assert ob.trace["iters"] > 1
    return og, seeds, eta, fan, rows, o_inp, ob


def _bits(t):
    return t.cpu().view(torch.int16) if t.dtype == torch.bfloat16 else t.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_candidate_numbering_and_fused_scale_match_the_oracle_on_every_route(cuda, monkeypatch, name):
    import bliss_gnn_amd as bg
    og, seeds, eta, fan, rows, o_inp, ob = _problem(name)
    g = bg.Graph(og.indptr.to(cuda), og.indices.to(cuda), og.eid.to(cuda))
    g.edata["w"] = bg.normalized_edata(g)
    C = int(ob.trace["cand_nid"].numel())
    for var, val in ROUTES:
        monkeypatch.delenv("BLISS_FUSE_SCALE", raising=False)
        monkeypatch.delenv("BLISS_BINS", raising=False)
        monkeypatch.setenv(var, val)
        s = bg.PoissonBanditLadiesSampler([fan], eta=eta)
        s._bind(g)
        s.exp3_weights = rows.to(cuda)
        eng = s._engine
        assert eng.fuse_scale == (var != "BLISS_FUSE_SCALE" or val == "1") and (eng.n_bins == 0) == (var == "BLISS_BINS")
        torch.manual_seed(9)
        inp, _, (b,) = s.sample_blocks(g, seeds.to(cuda))
        s.check_errors()
        k = b._counts
        assert (k.C, k.err) == (C, 0), (var, val, k.C, k.err)                                    # C first, then the rest
        assert (k.E, k.K, k.c, k.iters, k.all_one) == (ob.trace["E"], ob.n_src, ob.trace["c"], ob.trace["iters"], 0), (var, val)
        assert torch.equal(inp.cpu().long(), o_inp)
        assert torch.equal(b._trace["cand_nid"].cpu().long(), ob.trace["cand_nid"]), (var, val)
        assert torch.equal(_bits(b._trace["p"]), _bits(ob.trace["p"])), (var, val)
        assert torch.equal(b.src.cpu().long(), ob.src) and torch.equal(b.dst.cpu().long(), ob.dst), (var, val)
        for mine, ref in ((b.edata["edge_weights"], ob.edge_weights), (b.edata["q_ij"], ob.q_ij), (b.srcdata["node_prob"], ob.node_prob)):
            assert torch.equal(_bits(mine), _bits(ref)), (var, val)
        assert int(eng.hist.abs().sum()) == 0 and int(eng.fs_ticket) == 0, (var, val)


@functools.lru_cache(maxsize=None)
def _ladies_problem(name):
    """-> graph, seeds, fanout, g.edata['w'] (by edge id), the oracle's block.  w = 1 / in-degree; on the graph without self loops
    the planted edge carries 2^-23 instead, so that its source's sum of squares is below the accumulator's unit: p == 0."""
    from oracle import bliss_oracle as bo
    og, seeds, _, info = CASES[name]()
    fan = int(bo.expand_frontier(og, seeds).nid.numel()) // 3
    edge_w = bo.normalized_edata(og).clone()
    if "tiny_pos" in info:
        edge_w[int(og.eid[info["tiny_pos"]])] = 2.0 ** -23
    torch.manual_seed(9)
    o_inp, _, (ob,) = bo.sample_blocks_ladies(og, seeds, [fan], edge_w)
    if "patterns" in info:                                              # five columns of one edge, w = 1 each: p = sqrt(5)
        bits = ob.trace["p"].bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF
        assert int(bits[seeds.numel():].min()) == 0 and 0x4000 <= int(bits.max()) < 0x7F80
    return og, seeds, fan, edge_w, o_inp, ob


@pytest.mark.parametrize("name", list(CASES))
def test_ladies_importances_match_the_oracle_on_every_route(cuda, monkeypatch, name):
    """The LADIES mode of the same kernels (p = sqrt(sum w^2)) against bo.sample_blocks_ladies."""
    import bliss_gnn_amd as bg
    og, seeds, fan, edge_w, o_inp, ob = _ladies_problem(name)
    g = bg.Graph(og.indptr.to(cuda), og.indices.to(cuda), og.eid.to(cuda))
    g.edata["w"] = edge_w.to(cuda)
    for var, val in ROUTES:
        monkeypatch.delenv("BLISS_FUSE_SCALE", raising=False)
        monkeypatch.delenv("BLISS_BINS", raising=False)
        monkeypatch.setenv(var, val)
        s = bg.PoissonLadiesSampler([fan])
        torch.manual_seed(9)
        inp, _, (b,) = s.sample_blocks(g, seeds.to(cuda))
        s.check_errors()
        k = b._counts
        assert (k.C, k.err) == (int(ob.trace["cand_nid"].numel()), 0), (var, val, k.C, k.err)
        assert (k.E, k.K, k.c, k.iters, k.all_one) == (ob.trace["E"], ob.n_src, ob.trace["c"], ob.trace["iters"], 0), (var, val)
        assert torch.equal(inp.cpu().long(), o_inp)
        assert torch.equal(b._trace["cand_nid"].cpu().long(), ob.trace["cand_nid"]), (var, val)
        assert torch.equal(_bits(b._trace["p"].bfloat16()), _bits(ob.trace["p"].bfloat16())), (var, val)
        assert torch.equal(b.src.cpu().long(), ob.src) and torch.equal(b.dst.cpu().long(), ob.dst), (var, val)
        assert torch.equal(_bits(b.edata["edge_weights"]), _bits(ob.edge_weights)), (var, val)
        assert int(s._engine.hist.abs().sum()) == 0 and int(s._engine.fs_ticket) == 0, (var, val)


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_candidate_capacity_below_the_candidate_count_is_reported_and_leaves_the_maps_clean(cuda, monkeypatch, fuse):
    """The engine gives every layer cap_c = |V|; here it is shrunk to 600 under a layer of 1025 candidates.  k_bin_reduce then
    cuts its touched list in no particular order, and k_cand_number must not number what is left (holes below cap_c would be
    indexed into the node maps by the select, the block passes and the cleanup): it flags bit 2 and keeps the 16 seeds only.
    The engine answers bit 2 by repeating the call on the atomic passes (k_chunk_scan's clamp: the first 600 candidates, in
    order), is flagged again and reports.  Both dense maps are clean afterwards; with the capacity back, a new sampler on the
    same graph gives the oracle's block."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import _engine
    monkeypatch.delenv("BLISS_BINS", raising=False)
    monkeypatch.setenv("BLISS_FUSE_SCALE", fuse)
    og, seeds, eta, fan, rows, o_inp, ob = _problem("C1025")
    g = bg.Graph(og.indptr.to(cuda), og.indices.to(cuda), og.eid.to(cuda))
    g.edata["w"] = bg.normalized_edata(g)

    def sampler():
        s = bg.PoissonBanditLadiesSampler([fan], eta=eta)
        s._bind(g)
        s.exp3_weights = rows.to(cuda)
        return s

    s = sampler()
    torch.manual_seed(9)
    s.sample_blocks(g, seeds.to(cuda))                                   # learns the capacities
    eng = s._engine
    assert eng.n_bins > 0 and eng.caps[0]["C"] == og.num_nodes
    eng.caps[0]["C"], eng.ws = 600, None
    attempts, grow = [], eng._grow

    def recording_grow(errs):
        c = _engine._parse_counts(eng.counts_host, 1)[0][0]
        attempts.append((eng.n_bins > 0, c.S, c.C, c.K, c.err))
        grow(errs)

    monkeypatch.setattr(eng, "_grow", recording_grow)
    torch.manual_seed(9)
    with pytest.raises(RuntimeError, match="candidate capacity exceeded"):
        s.sample_blocks(g, seeds.to(cuda))
    S = int(seeds.numel())
    assert attempts == [(True, S, S, S, 2)]                              # the binned attempt: seeds only, all kept (C <= fanout)
    last = _engine._parse_counts(eng.counts_host, 1)[0][0]
    assert eng.n_bins == 0 and (last.S, last.C, last.err & 2) == (S, 600, 2)      # the atomic attempt: the clamp
    for i in eng._sets:
        assert bool((eng._sets[i]["local_id"] == -1).all()) and bool((eng._sets[i]["kept_map"] == -1).all())
    assert int(eng.hist.abs().sum()) == 0 and int(eng.fs_ticket) == 0
    s2 = sampler()
    torch.manual_seed(9)
    inp, _, (b,) = s2.sample_blocks(g, seeds.to(cuda))
    s2.check_errors()
    assert (b._counts.C, b._counts.K, b._counts.c, b._counts.err) == (1025, ob.n_src, ob.trace["c"], 0)
    assert torch.equal(b._trace["cand_nid"].cpu().long(), ob.trace["cand_nid"]) and torch.equal(b.src.cpu().long(), ob.src)
    assert torch.equal(_bits(b.srcdata["node_prob"]), _bits(ob.node_prob))
