"""GPU suite (-m gpu): k_col_sums (csrc/sampler.hip) at every column length where it takes another path -- one wave per column
up to 1024 edges, one workgroup per longer column with the first 8192 edges in registers, the classes of k_seg_scan's list
(over 1024 / over 4096 edges), the tails beyond the registers -- and on both arithmetic paths: the branch-free sums of plain
terms and the generic converters (terms below the accumulator's unit, below its 40-bit second accumulator, all-tiny columns).
Everything goes through the public sampler and is compared with the oracle bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

V = 40000
DEGS = [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 8191, 8192, 8193, 16384, 16385, 24577, 33000]
NS = len(DEGS)                   # nodes 0 .. NS-1 are the seeds with these in-degrees
N_SEEDS = 64
FAN, ETA = [3000, 1500], 0.1


def _bg():
    import bliss_gnn_amd as bg
    return bg


@functools.lru_cache(maxsize=None)
def _problem():
    """The graph (host CSC), the seed list and the two sets of EXP3 rows (by edge id)."""
    from oracle import bliss_oracle as bo
    gen = torch.Generator().manual_seed(123)
    src, dst = [], []
    for node, deg in enumerate(DEGS):                                   # distinct sources per seed column (+ the self loop)
        src.append(torch.randperm(V - NS, generator=gen)[:deg - 1] + NS)
        dst.append(torch.full((deg - 1,), node))
    for node, deg in enumerate(DEGS):                                   # the hubs appear thousands of times as sources
        if deg >= 8192:
            src.append(torch.full((2000,), node))
            dst.append(torch.randint(NS, V, (2000,), generator=gen))
    src.append(torch.randint(0, V, (300000,), generator=gen))
    dst.append(torch.randint(NS, V, (300000,), generator=gen))
    og = bo.prepare_graph(torch.cat(src), torch.cat(dst), V)
    assert [int(og.indptr[i + 1] - og.indptr[i]) for i in range(NS)] == DEGS
    seeds = torch.cat([torch.arange(NS), torch.randperm(V - NS, generator=gen)[:N_SEEDS - NS] + NS]).to(torch.int32)
    E = og.num_edges
    ones = torch.ones(len(FAN), E, dtype=torch.bfloat16)
    # mixed rows, built by CSC position: weights in [0.25, 1) (plain terms), one edge in ten 2^-50 lower (the generic
    # converters in many short columns), then the special columns
    w = 0.25 + 0.75 * torch.rand(E, generator=gen)
    w = torch.where(torch.rand(E, generator=gen) < 0.1, w * 2.0 ** -50, w)
    col = lambda d: int(og.indptr[DEGS.index(d)])
    w[col(1024):col(1024) + 1024] = 0.25 + 0.75 * torch.rand(1024, generator=gen)
    w[col(1024) + 0] = 2.0 ** -50                  # one-wave path, first register slot: below the accumulator's unit
    w[col(1024) + 1000] = 2.0 ** -100              # ... last register slot: below the second accumulator too (sticky)
    w[col(4097):col(4097) + 4097] = 0.25 + 0.75 * torch.rand(4097, generator=gen)
    w[col(4097) + 7] = 2.0 ** -100                 # one-workgroup path, first register slot
    w[col(8192):col(8192) + 8192] = 0.25 + 0.75 * torch.rand(8192, generator=gen)
    w[col(8192) + 8100] = 2.0 ** -50               # ... last register slot
    w[col(16385):col(16385) + 16385] = 0.25 + 0.75 * torch.rand(16385, generator=gen)
    w[col(16385) + 9000] = 2.0 ** -100             # a hub: in the second 8192 edges
    w[col(24577):col(24577) + 24577] = (0.25 + 0.75 * torch.rand(24577, generator=gen)) * 2.0 ** -12
    w[col(24577) + 24576] = 0.75                   # a hub whose largest weight is its very last edge
    for d in (65, 4096):                           # columns whose weights are ALL tiny: the sum is far below 2^-40
        w[col(d):col(d) + d] = (0.25 + 0.75 * torch.rand(d, generator=gen)) * 2.0 ** -90
    w_e = torch.empty(E)
    w_e[og.eid.long()] = w                         # by edge id, like the reference's attribute
    mixed = torch.stack([w_e, w_e]).bfloat16()
    return og, seeds, dict(ones=ones, mixed=mixed)


@functools.lru_cache(maxsize=None)
def _oracle(rows):
    from oracle import bliss_oracle as bo
    og, seeds, w = _problem()
    torch.manual_seed(9)
    o_inp, _, o_blocks = bo.sample_blocks_bandit(og, seeds, FAN, w[rows], ETA)
    return o_inp, o_blocks


def _sampler(cuda, rows):
    bg = _bg()
    og, seeds, w = _problem()
    g = bg.Graph(og.indptr.to(cuda), og.indices.to(cuda), og.eid.to(cuda))
    g.edata["w"] = bg.normalized_edata(g)
    s = bg.PoissonBanditLadiesSampler(FAN, eta=ETA)
    if rows != "ones":
        s._bind(g)
        s.exp3_weights = w[rows].to(cuda)
    return g, s, seeds.to(cuda)


def _bits(t):
    return t.cpu().view(torch.int16) if t.dtype == torch.bfloat16 else t.cpu()


def _seed_coef(eng, n, S):
    """(bf16 bits of sum_j w_ij, bf16 bits of sum_k q_ik) per seed of sampling layer n, from the engine's per-seed scratch."""
    cs = eng.caps[n]["S"]
    x = eng.ws[n].seed_acc.view(torch.int64)[6 * cs: 6 * cs + S].cpu()
    return x & 0xFFFF, (x >> 16) & 0xFFFF


def _check_against_oracle(sampler, inp, blocks, rows):
    o_inp, o_blocks = _oracle(rows)
    assert torch.equal(inp.cpu().long(), o_inp)
    for n, (b, ob) in enumerate(zip(reversed(blocks), reversed(o_blocks))):      # sampling order
        assert b._counts.E == ob.trace["E"] and b._counts.c == ob.trace["c"] and b._counts.err == 0
        assert torch.equal(b._trace["cand_nid"].cpu().long(), ob.trace["cand_nid"])
        assert torch.equal(_bits(b._trace["p"]), _bits(ob.trace["p"]))
        assert torch.equal(b.src.cpu().long(), ob.src) and torch.equal(b.dst.cpu().long(), ob.dst)
        for mine, ref in ((b.edata["edge_weights"], ob.edge_weights), (b.edata["q_ij"], ob.q_ij), (b.srcdata["node_prob"], ob.node_prob)):
            assert torch.equal(_bits(mine), _bits(ref))
        # the column sums themselves: numerics.exact_segment_sum_rel / exact_segment_sum of the oracle, rounded once
        S = ob.trace["w_sum"].numel()
        wsum, qsum = _seed_coef(sampler._engine, n, S)
        assert torch.equal(wsum, _bits(ob.trace["w_sum"]).long() & 0xFFFF), n
        assert torch.equal(qsum, _bits(ob.trace["q_sum"]).long() & 0xFFFF), n


@pytest.mark.parametrize("rows", ["ones", "mixed"])
def test_column_lengths_match_oracle(cuda, rows):
    """ones: EXP3 rows of ones (every term plain).  mixed: rows that put waves and workgroups on both arithmetic paths (see
    _problem).  Candidates, p, blocks, edge weights, q_ij, node_prob and the per-seed sums' bits equal the oracle's."""
    g, s, seeds = _sampler(cuda, rows)
    torch.manual_seed(9)
    inp, _, blocks = s.sample_blocks(g, seeds)
    s.check_errors()
    _check_against_oracle(s, inp, blocks, rows)


def _snapshot(s, blocks, cnts):
    """What one static call left: per layer (sampling order) the live block fields and the per-seed sums."""
    bg = _bg()
    out = []
    for n, (b, c) in enumerate(zip(reversed(blocks), cnts)):
        assert c.err == 0
        cs = s._engine.caps[n]["S"]
        acc = s._engine.ws[n].seed_acc.view(torch.int64)
        out.append(dict(sizes=(c.S, c.E, c.C, c.K, c.B), src=b.src[:c.B].clone(), dst=b.dst[:c.B].clone(),
                        nid=b.srcdata[bg.NID][:c.K].clone(), ew=_bits(b._edge_weights[:c.B]).clone(), q=_bits(b._q[:c.B]).clone(),
                        prob=_bits(b._node_prob[:c.K]).clone(), acc_w=acc[:c.S].clone(), acc_q=acc[cs:cs + c.S].clone(),
                        coef=acc[6 * cs:6 * cs + c.S].clone()))
    return out


def _same(a, b):
    for la, lb in zip(a, b):
        assert la["sizes"] == lb["sizes"]
        for k in la:
            if k != "sizes":
                assert torch.equal(la[k].cpu(), lb[k].cpu()), k


def test_replays_leave_the_same_bits(cuda):
    """The same batch three times in a row through the static path and three times from a captured graph: every run leaves the
    bits of the eager call (a ticket, count or accumulator left dirty by one launch would show in the next)."""
    bg = _bg()
    g, s, seeds = _sampler(cuda, "mixed")
    torch.manual_seed(9)
    inp, _, eager = s.sample_blocks(g, seeds)                         # binds the engine, learns the capacities
    _check_against_oracle(s, inp, eager, "mixed")
    eng = s._engine

    def static_once(launch):
        torch.manual_seed(9)
        eng.stage_rng_from_torch()
        blocks = launch()
        torch.cuda.synchronize()
        return _snapshot(s, blocks, s.finish_static())

    runs = [static_once(lambda: s.sample_blocks_static(g, seeds)[2]) for _ in range(3)]
    for n, (r, be) in enumerate(zip(runs[0], reversed(eager))):
        assert r["sizes"][3:] == (be.num_src_nodes(), be.num_edges())
        assert torch.equal(r["src"], be.src) and torch.equal(r["dst"], be.dst) and torch.equal(r["nid"], be.srcdata[bg.NID])
        assert torch.equal(r["ew"], _bits(be.edata["edge_weights"])) and torch.equal(r["q"], _bits(be.edata["q_ij"]))
        assert torch.equal(r["prob"], _bits(be.srcdata["node_prob"]))
    for r in runs[1:]:
        _same(runs[0], r)
    torch.manual_seed(9)
    eng.stage_rng_from_torch()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = s.sample_blocks_static(g, seeds)[2]
    for _ in range(3):
        def replay():
            graph.replay()
            return captured
        _same(runs[0], static_once(replay))


def test_sharded_caller_with_hub_seeds(cuda):
    """One layer through BLISS_MODE_PARTIALS (shard.py: the sharded caller of the same launch) on a world of one rank, the hubs
    among the seeds: the by-source partial sums equal the oracle's exact Q.44 accumulators, the per-seed sums its bf16 sums."""
    from bliss_gnn_amd import shard as sh
    from oracle import numerics as nx
    og, seeds, w = _problem()
    _, o_blocks = _oracle("mixed")
    ob = o_blocks[-1]                                                  # sampling layer 0: the seeds' own columns
    shard = sh.GraphShard.from_global(og.indptr, og.indices, og.eid, torch.tensor([0, V]), 0, device=cuda)
    ops = sh._HipShardOps(shard, len(FAN), ETA)
    ops.w_pos = w["mixed"][:, og.eid.long()].contiguous().to(cuda)      # by CSC position
    ops.set_caps(N_SEEDS, list(reversed(FAN)))
    ids, sums = ops.frontier_partials(0, len(FAN) - 1, seeds.to(cuda))
    q, q_sum = ob.trace["q"], ob.trace["q_sum"]
    r = q / q_sum[ob.trace["dst_l"]]
    _, acc = nx.exact_segment_sum(r ** 2, ob.trace["src_l"], ob.trace["cand_nid"].numel(), nx.FRAC_SRC)
    want = dict(zip(ob.trace["cand_nid"].tolist(), acc.tolist()))
    got = dict(zip(ids.cpu().tolist(), sums.cpu().tolist()))
    assert len(got) == ids.numel() and got == want
    wsum, qsum = _seed_coef(ops.eng, 0, N_SEEDS)
    assert torch.equal(wsum, _bits(ob.trace["w_sum"]).long() & 0xFFFF)
    assert torch.equal(qsum, _bits(q_sum).long() & 0xFFFF)
