"""GPU suite (-m gpu): the node-wise draw WITH replacement (csrc/replace_draw.hip) against the CPU restatement
of its rule (tests/replace_ref.py).  The rule is integers only: every block array, the picks, the sources, the by-source index, the
counts and q_ij are compared with equality; the weights (an fp64 sum) within one bf16 ulp and section 17's column-sum bound.

Graphs: ``chung_lu_csc(4000, 200000, seed=9)`` and a hand-built multigraph (1400 nodes) whose first nodes have in-degrees 0, 1, 2, 63,
64, 65, 255, 256, 257 and 1025 (the draw kernel's chunk table holds 1024 prefixes: the last one is the first column with a chunk of two),
then a column of six parallel edges, a column with a self loop, the bad-value column and an all-zero column."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import replace_ref as ref
import wneighbor_ref as wref
from block_invariants import check_index
from bounds import SPMM_K, assert_within, spmm_terms
from test_gpu_neighbor import GUARD, SEED, Layer
from test_replace_ref import CASES, check_counts

pytestmark = pytest.mark.gpu

DEG_H = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 6, 5, 8, 8]
HUB_H, PAR, LOOP, BAD, ZERO = 9, 10, 11, 12, 13
BAD_VALUES = [0, 3, np.nan, 1, -2, np.inf, 2, 0]
V_H = 1400
FANOUTS = [1, 3, 64, 257, 1024, -1]
SIZES = [1, 31, 300]
M64 = ref.M64


@functools.lru_cache(maxsize=None)
def graph_np(name):
    """(indptr int64, indices int32, eid int32, bf16 bit patterns of the raw probabilities by CSC position)."""
    if name == "cl":
        from bliss_gnn_amd.synth import chung_lu_csc
        ip, ix, ei = (t.numpy() for t in chung_lu_csc(4000, 200000, seed=9))
        ip, ix, ei = ip.astype(np.int64), ix.astype(np.int32), ei.astype(np.int32)
    else:
        rng = np.random.default_rng(31)
        deg = np.concatenate([np.array(DEG_H), rng.integers(0, 13, V_H - len(DEG_H))])
        ip = np.zeros(V_H + 1, dtype=np.int64)
        ip[1:] = np.cumsum(deg)
        ix = rng.integers(0, V_H, int(ip[-1])).astype(np.int32)
        ix[ip[PAR]:ip[PAR + 1]] = 700                                            # six parallel edges
        ix[ip[LOOP]] = LOOP                                                      # a self loop
        ix[ip[HUB_H] + 5] = 3                                                    # a seed that is a source of another seed
        ei = rng.permutation(int(ip[-1])).astype(np.int32)
    E = int(ip[-1])
    rng = np.random.default_rng(32)
    q = wref.rbf(np.exp2(rng.uniform(-6, 3, E)).astype(np.float32))
    q[rng.permutation(E)[:E // 9]] = 0.0
    if name == "hand":
        q[ip[BAD]:ip[BAD + 1]] = BAD_VALUES
        q[ip[ZERO]:ip[ZERO + 1]] = 0.0
        q[ip[HUB_H] + 17], q[ip[HUB_H] + 900] = np.nan, -2.0
    return ip, ix, ei, wref.bf16_bits(q)


@functools.lru_cache(maxsize=None)
def seeds_of(name, S):
    ip = graph_np(name)[0]
    V = len(ip) - 1
    hub = int(np.argmax(np.diff(ip)))
    if S == 1:
        return (hub,)
    first = list(range(len(DEG_H))) if name == "hand" else [hub]
    rest = [int(v) for v in np.random.default_rng(33 + S).permutation(V) if int(v) not in first][:S - len(first)]
    return tuple(np.random.default_rng(34).permutation(np.array(first + rest)).tolist())


@functools.lru_cache(maxsize=None)
def want_layer(name, S, fanout, weighted, step=0, layer=0):
    ip, ix, ei, pb = graph_np(name)
    return ref.sample_layer(ip, ix, ei, np.array(seeds_of(name, S)), fanout, SEED, step, layer, prob_bits=pb if weighted else None)


def bits_dev(b, dev):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).to(dev).view(torch.bfloat16)


@pytest.fixture(scope="module")
def graphs_dev(cuda):
    out = {}
    for name in ("hand", "cl"):
        ip, ix, ei, pb = graph_np(name)
        out[name] = (torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda), torch.from_numpy(ei).to(cuda), bits_dev(pb, cuda))
    return out


class RLayer(Layer):
    """Hand-allocated buffers of direct bliss_neighbor_replace_layer calls; every output array is followed by guard words and the
    weight / q_ij arrays are NaN before every call."""

    def __init__(self, dev, graph_dev, cap_s, cap_k, cap_b):
        super().__init__(dev, graph_dev[:3], cap_s, cap_k, cap_b)
        V = int(self.ip.numel()) - 1
        self.num_nodes, self.g.num_nodes = V, V
        self.kept_map = torch.full((V,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(self.lib.lib.bliss_neighbor_replace_scratch_bytes(V, cap_s)) // 4, dtype=torch.int32, device=dev)
        self.picks = torch.full((cap_b + GUARD,), -7, dtype=torch.int32, device=dev)

    def __call__(self, seeds, fanout, prob=None, step=0, layer=0, bump=0, r_ov=None, n_seeds_dev=None, set_step=True, picks=True,
                 transpose=True, sync=True):
        _lib = self.lib
        if set_step:
            self.step.fill_(step)
        self.w[:self.cap_b] = float("nan")
        self.q[:self.cap_b] = float("nan")
        n_seeds = -1 if n_seeds_dev is not None else int(seeds.numel())
        cnt_ptr = self.counts.data_ptr()
        ws = _lib.LayerWs(cnt_ptr, self.seg_ptr.data_ptr(), 0, 0, 0, 0, 0, 0, self.kept_nid.data_ptr(), 0, 0, 0, 0, self.cap_k)
        ws.kept_map = self.kept_map.data_ptr()
        out = _lib.BlockOut(self.indptr.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), self.pos.data_ptr(), self.eid.data_ptr(),
                            self.w.data_ptr(), self.q.data_ptr(), 0, 0, 0, self.cap_b)
        st = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib.bliss_neighbor_replace_layer(C.byref(self.g), seeds.data_ptr(), n_seeds, 0 if n_seeds_dev is None else n_seeds_dev,
                                                   self.cap_s, fanout, 0 if r_ov is None else r_ov.data_ptr(), SEED,
                                                   self.step.data_ptr(), layer, bump, 0 if prob is None else prob.data_ptr(),
                                                   self.picks.data_ptr() if picks else 0, C.byref(ws), C.byref(out),
                                                   self.scratch.data_ptr(), st)
        assert rc == 0, rc
        if transpose:
            rc = _lib.lib.bliss_block_transpose(self.src.data_ptr(), cnt_ptr + 16, self.cap_b, self.cap_b, self.cap_k,
                                                self.t_indptr.data_ptr(), self.t_edge.data_ptr(), self.tr_temp.data_ptr(), self.tr_bytes, st)
            assert rc == 0, rc
        if not sync:
            return None
        torch.cuda.synchronize()
        return _lib.LayerCounts.from_buffer_copy(self.counts[:10].cpu().numpy().tobytes())

    def assert_guards(self):
        super().assert_guards()
        assert bool((self.picks[self.cap_b:] == -7).all()), "guard words after picks_out were overwritten"

    def assert_clean(self):
        words = -(-(-(-self.num_nodes // 32)) // 1024) * 1024
        assert bool((self.kept_map == -1).all()), "kept_map is not clean"
        assert int(self.scratch[:16 + words].abs().sum()) == 0, "tickets / bitmap are not zero"

    def got(self, c):
        n = lambda t: t.cpu().numpy()
        S, K, B = c.S, c.K, c.B
        return dict(S=S, E=c.E, K=K, B=B, indptr=n(self.indptr[:S + 1]), pos=n(self.pos[:B]), dst=n(self.dst[:B]), eid=n(self.eid[:B]),
                    src=n(self.src[:B]), kept_nid=n(self.kept_nid[:K]), t_indptr=n(self.t_indptr[:K + 1]), t_edge=n(self.t_edge[:B]),
                    q_ij=n(self.q[:B].view(torch.int16)).view(np.uint16), weights=n(self.w[:B].float()), picks=n(self.picks[:B]))

    def assert_equals(self, c, want):
        assert (c.C, c.err) == (c.K, 0), (c.C, c.K, c.err)
        ref.compare(self.got(c), want)                                           # (a weight left NaN fails its `> 0`)
        assert int(self.indptr[c.S:self.cap_s + 1].min()) == int(self.indptr[c.S:self.cap_s + 1].max()) == c.B   # padded rows are empty
        assert bool((self.kept_nid[c.K:self.cap_k] == 0).all())                  # capacity padding: a valid node id
        assert bool(torch.isnan(self.w[c.B:self.cap_b].float()).all()) and bool(torch.isnan(self.q[c.B:self.cap_b].float()).all())
        self.assert_guards()
        self.assert_clean()


def make_layer(cuda, graphs_dev, name, S, fanout):
    E = int(graphs_dev[name][1].numel())
    V = int(graphs_dev[name][0].numel()) - 1
    return RLayer(cuda, graphs_dev[name], S + 3, V, S * fanout if fanout > 0 else E)


@pytest.mark.parametrize("fanout", FANOUTS + [65])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "raw"])
def test_layer_equals_the_restatement(cuda, graphs_dev, fanout, weighted):
    """Both graphs, S = 1, 31, 300: every output array.  Fanout 64 is the widest one-wave uniform draw, 65 the first on a workgroup."""
    for name in ("hand", "cl"):
        prob = graphs_dev[name][3] if weighted else None
        for S in SIZES:
            lay = make_layer(cuda, graphs_dev, name, S, fanout)
            seeds = torch.tensor(seeds_of(name, S), dtype=torch.int32, device=cuda)
            c = lay(seeds, fanout, prob)
            want = want_layer(name, S, fanout, weighted)
            lay.assert_equals(c, want)
            if fanout > 0:                                                       # k_s = fanout also when d <= fanout; B known up front
                deg = np.diff(graph_np(name)[0])[list(seeds_of(name, S))]
                assert np.array_equal(np.diff(want["indptr"]), np.where(deg > 0, fanout, 0)) and c.B == fanout * int((deg > 0).sum())
            if S == 31 and fanout == 3:
                c = lay(seeds, fanout, prob, step=5, layer=2)                    # another step and layer, the same scratch
                lay.assert_equals(c, want_layer(name, S, fanout, weighted, 5, 2))
    if weighted and fanout == 64:
        want = want_layer("hand", 31, 64, True)
        s = seeds_of("hand", 31).index(BAD)
        o, e = want["indptr"][s], want["indptr"][s + 1]
        assert set(want["picks"][o:e].tolist()) == {1, 3, 6}                      # only the three positive finite entries
        s = seeds_of("hand", 31).index(ZERO)
        o, e = want["indptr"][s], want["indptr"][s + 1]
        assert bool(want["fallback"][s]) and bool((want["weights"][o:e] == 1).all()) and len(set(want["picks"][o:e].tolist())) > 3


def test_second_layer_reads_its_seed_count_from_the_device(cuda, graphs_dev):
    ip, ix, ei, pb = graph_np("hand")
    lays = ref.sample_blocks(ip, ix, ei, np.array(seeds_of("hand", 31)[:9]), [5, 3], SEED, 4, prob_bits=pb)
    prob = graphs_dev["hand"][3]
    first = RLayer(cuda, graphs_dev["hand"], 16, 64, 9 * 5)
    c0 = first(torch.tensor(seeds_of("hand", 31)[:9], dtype=torch.int32, device=cuda), 5, prob, step=4, layer=0)
    first.assert_equals(c0, lays[0])
    second = RLayer(cuda, graphs_dev["hand"], 64, 64 * 4, 64 * 3)
    c1 = second(first.kept_nid[:64], 3, prob, step=4, layer=1, bump=1, n_seeds_dev=first.counts.data_ptr() + 12)
    second.assert_equals(c1, lays[1])
    assert int(second.step.item()) == 5                                          # bumped once, by one workgroup


def test_a_seed_id_out_of_range_is_an_empty_column(cuda, graphs_dev):
    ip, ix, ei, pb = graph_np("hand")
    ids = list(seeds_of("hand", 31)[:20])
    lay = RLayer(cuda, graphs_dev["hand"], 32, V_H, 32 * 7)
    for prob in (None, graphs_dev["hand"][3]):
        for bad in (V_H, -1, 2 ** 31 - 1):
            mixed = ids[:9] + [bad] + ids[9:]
            c = lay(torch.tensor(mixed, dtype=torch.int32, device=cuda), 7, prob, step=1)
            assert c.err == 2 and c.S == 21                                      # BLISS_ERR_CAP_CAND
            want = ref.sample_layer(ip, ix, ei, np.array(mixed), 7, SEED, 1, 0, prob_bits=None if prob is None else pb)
            row = lay.indptr[:22].cpu().numpy()
            assert row[10] == row[9] and np.array_equal(row, want["indptr"])
            assert np.array_equal(lay.pos[:c.B].cpu().numpy(), want["pos"]) and np.array_equal(lay.src[:c.B].cpu().numpy(), want["src"])
            lay.assert_guards()
            lay.assert_clean()
        c = lay(torch.tensor(ids, dtype=torch.int32, device=cuda), 7, prob, step=1)     # and the next call is whole
        lay.assert_equals(c, ref.sample_layer(ip, ix, ei, np.array(ids), 7, SEED, 1, 0, prob_bits=None if prob is None else pb))


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "raw"])
def test_planted_variates(cuda, graphs_dev, weighted):
    """r = 0, r = 2^64 - 1, and the two variates around a prefix boundary: the smallest r whose t equals the prefix, and r - 1."""
    ip, ix, ei, pb = graph_np("hand")
    seeds = seeds_of("hand", 31)
    f = 4
    r = np.zeros(31 * f, dtype=np.uint64)
    on_boundary = 0
    for s, v in enumerate(seeds):
        a, d = int(ip[v]), int(ip[v + 1] - ip[v])
        w = ref.fixed_weights(pb[a:a + d]) if weighted and d else None
        W = sum(w) if w else 0
        if W:
            i = next(i for i in range(d // 2, d + d // 2) if w[i % d]) % d       # an entry of positive weight
            prefix, tot = sum(w[:i + 1]), W
        else:
            prefix, tot = d // 2, max(d, 1)
        rb = -((-prefix << 64) // tot)                                           # ceil(prefix * 2^64 / tot)
        if 0 < prefix < tot:
            assert (rb * tot) >> 64 == prefix and ((rb - 1) * tot) >> 64 == prefix - 1
            on_boundary += 1
        r[s * f:s * f + f] = [0, M64, min(rb, M64), max(rb - 1, 0)]
    assert on_boundary >= 15
    lay = make_layer(cuda, graphs_dev, "hand", 31, f)
    prob = graphs_dev["hand"][3] if weighted else None
    c = lay(torch.tensor(seeds, dtype=torch.int32, device=cuda), f, prob, r_ov=torch.from_numpy(r.view(np.int64)).to(cuda))
    want = ref.sample_layer(ip, ix, ei, np.array(seeds), f, SEED, 0, 0, prob_bits=pb if weighted else None, r_override=r.tolist())
    lay.assert_equals(c, want)
    s = seeds.index(HUB_H)
    pk = want["picks"][want["indptr"][s]:want["indptr"][s + 1]].tolist()
    if not weighted:
        assert pk == [0, 1025 // 2 - 1, 1025 // 2, 1024]
    else:
        w = ref.fixed_weights(pb[int(ip[HUB_H]):int(ip[HUB_H + 1])])
        assert pk[0] == min(i for i in range(1025) if w[i]) and pk[3] == max(i for i in range(1025) if w[i]) and pk[2] > pk[1]


def test_capacity_overflows_raise_their_bit_and_leave_the_scratch_idle(cuda, graphs_dev):
    prob = graphs_dev["hand"][3]
    seeds = torch.tensor(seeds_of("hand", 31), dtype=torch.int32, device=cuda)
    want = want_layer("hand", 31, 64, True)
    V = V_H
    from bliss_gnn_amd import _lib
    shared = torch.zeros(int(_lib.lib.bliss_neighbor_replace_scratch_bytes(V, 31)) // 4, dtype=torch.int32, device=cuda)
    for cap_s, cap_k, cap_b, bit in ((31, want["K"] - 1, want["B"], 4), (31, want["K"], want["B"] - 1, 8), (30, want["K"], want["B"], 64)):
        short = RLayer(cuda, graphs_dev["hand"], cap_s, cap_k, cap_b)
        short.scratch = shared
        c = short(seeds, 64, prob)
        assert c.err & bit, (c.err, bit)
        assert c.K <= cap_k and c.B <= cap_b and c.S <= cap_s
        short.assert_guards()
        short.assert_clean()
        check_index(short.src.cpu(), short.t_indptr.cpu(), short.t_edge.cpu(), c.K, c.B, cap_k)       # clamped, and still walkable
        roomy = RLayer(cuda, graphs_dev["hand"], 31, want["K"], want["B"])       # the exact capacities hold everything
        roomy.scratch, roomy.kept_map = shared, short.kept_map
        roomy.assert_equals(roomy(seeds, 64, prob), want)


def test_replay_and_the_step_bump(cuda, graphs_dev):
    prob = graphs_dev["cl"][3]
    seeds = torch.tensor(seeds_of("cl", 300), dtype=torch.int32, device=cuda)
    for p, f in ((prob, 3), (None, 3), (None, 257)):                              # (each of the three draw kernels takes its ticket)
        lay = make_layer(cuda, graphs_dev, "cl", 300, f)
        snaps = []
        for _ in range(2):                                                       # the step rewound: the same draw on the same scratch
            c = lay(seeds, f, p, step=9, layer=1, bump=0)
            assert int(lay.step.item()) == 9
            snaps.append(lay.got(c))
        for name in snaps[0]:
            assert np.array_equal(np.asarray(snaps[0][name]), np.asarray(snaps[1][name])), name
        c = lay(seeds, f, p, step=9, layer=1, bump=1)
        assert int(lay.step.item()) == 10                                        # once per call, by one workgroup
        assert np.array_equal(lay.got(c)["pos"], snaps[0]["pos"])                # (the call itself drew with step 9)
        c = lay(seeds, f, p, layer=1, bump=1, set_step=False)
        assert int(lay.step.item()) == 11
        lay.assert_equals(c, want_layer("cl", 300, f, p is not None, 10, 1))
        assert not np.array_equal(lay.got(c)["pos"], snaps[0]["pos"])


@pytest.mark.parametrize("name", ["uniform-8", "weighted-1..8"])
def test_pick_counts_on_the_device(cuda, name):
    """Node 7 with eight in-edges, fanout 3, draw steps 0 .. 2047 counted by the device's own step counter: the pick counts are
    the restatement's, so within 5 sigma of the multinomial expectation."""
    ident, q, m, f = CASES[name]
    ip = torch.tensor([0] * (ident + 1) + [m, m], dtype=torch.int64, device=cuda)            # node `ident` holds the column
    ix = torch.arange(m, dtype=torch.int32, device=cuda) % 6
    lay = RLayer(cuda, (ip, ix, torch.arange(m, dtype=torch.int32, device=cuda)), 1, 8, f)
    prob = None if q is None else bits_dev(wref.bf16_bits(np.asarray(q, dtype=np.float32)), cuda)
    seeds = torch.tensor([ident], dtype=torch.int32, device=cuda)
    hits = torch.zeros(m, dtype=torch.int64, device=cuda)
    errs = torch.zeros(1, dtype=torch.int32, device=cuda)
    one = torch.ones(f, dtype=torch.int64, device=cuda)
    for t in range(2048):
        lay(seeds, f, prob, layer=1, bump=1, set_step=t == 0, picks=False, transpose=False, sync=False)
        hits.index_add_(0, lay.pos[:f].long(), one)
        errs |= lay.counts[5:6] | (lay.counts[4:5] != f).int()
    torch.cuda.synchronize()
    assert int(lay.step.item()) == 2048 and int(errs.item()) == 0
    from test_replace_ref import case_counts
    assert np.array_equal(hits.cpu().numpy(), case_counts(name, 2048))
    check_counts(hits.cpu().numpy(), name, 2048)


@pytest.fixture(scope="module")
def repeat_block(cuda):
    """One layer of NeighborSampler(draw="device", replace=True, prob="w") over the hand graph's first 31 seeds, fanout 7: columns
    of one, two and six edges hold repeated edges.  Checked against the restatement before any consumer runs on it."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.fit import NeighborSampler
    ip, ix, ei, pb = graph_np("hand")
    g = bg.Graph(torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda), torch.from_numpy(ei).to(cuda))
    w_eid = torch.empty(int(ip[-1]), dtype=torch.bfloat16)
    w_eid[torch.from_numpy(ei).long()] = bits_dev(pb, "cpu")
    g.edata["w"] = w_eid.to(cuda)
    s = NeighborSampler([7], seed=SEED, draw="device", replace=True, prob="w")
    seeds = torch.tensor(seeds_of("hand", 31), dtype=torch.int32, device=cuda)
    _, _, (blk,) = s.sample_blocks(g, seeds)
    want = want_layer("hand", 31, 7, True)
    c = blk._counts
    t_indptr, t_edge = blk.transposed() if blk._transposed is None else blk._transposed
    n = lambda t: t.cpu().numpy()
    got = dict(S=c.S, E=c.E, K=c.K, B=c.B, indptr=n(blk.indptr), pos=n(blk.pos), dst=n(blk.dst), eid=n(blk.edata[bg.EID]), src=n(blk.src),
               kept_nid=n(blk.srcdata[bg.NID]), t_indptr=n(t_indptr[:c.K + 1]), t_edge=n(t_edge[:c.B]),
               q_ij=n(blk.edata["q_ij"].view(torch.int16)).view(np.uint16), weights=n(blk.edata["edge_weights"].float()),
               picks=want["picks"])                                              # (no picks_out in a product path)
    ref.compare(got, want)
    assert s.draw_step() == 1
    return blk, want


def test_transpose_of_a_block_with_repeated_edges(cuda, repeat_block):
    """bliss_block_transpose on repeated edges: the stable argsort of src (equal (src, dst) pairs keep their edge order)."""
    blk, want = repeat_block
    pairs = np.stack([want["src"], want["dst"]], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                            # the block does hold the same edge twice
    t_indptr, t_edge = blk._transposed
    order = torch.argsort(blk.src.long(), stable=True)
    assert torch.equal(t_edge[:want["B"]].long(), order)
    assert torch.equal(t_indptr[:want["K"] + 1].long().cpu(), torch.from_numpy(np.searchsorted(want["src"][order.cpu().numpy()],
                                                                                              np.arange(want["K"] + 1))))


def test_spmm_over_repeated_edges(cuda, repeat_block):
    """weighted_aggregate forward and backward on that block: per element against fp64 from the RESTATEMENT's src / dst -- a repeated
    edge contributes once per repeat to both -- within the project's SPMM_K."""
    from bliss_gnn_amd.nn import weighted_aggregate
    blk, want = repeat_block
    K, S = want["K"], want["S"]
    src, dst = torch.from_numpy(want["src"]).long().to(cuda), torch.from_numpy(want["dst"]).long().to(cuda)
    gen = torch.Generator().manual_seed(4)
    w = blk.edata["edge_weights"]
    for dim, mean, wt in ((41, True, True), (64, False, True), (64, True, False)):
        h = torch.randn(K, dim, generator=gen).bfloat16().to(cuda).requires_grad_(True)
        gout = torch.randn(S, dim, generator=gen).bfloat16().to(cuda)
        out = weighted_aggregate(blk, h, w if wt else None, mean=mean)
        out.backward(gout)
        rf, mag = spmm_terms(src, dst, S, h.detach(), w if wt else None, mean)
        rb, mb = spmm_terms(src, dst, S, gout, w if wt else None, mean, by_src=True, n_out=K)
        case = "repeats d%d %s %s" % (dim, "mean" if mean else "sum", "w" if wt else "1")
        r1 = assert_within(out, rf, mag, *SPMM_K["bf16"], "spmm out " + case)
        r2 = assert_within(h.grad, rb, mb, *SPMM_K["bf16"], "spmm d h " + case)
        print("RATIO %s out %.3f dh %.3f" % (case, r1, r2))
