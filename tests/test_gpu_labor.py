"""GPU suite (-m gpu): the device-side LABOR-0 sampler (csrc/labor.hip) against the CPU restatement of its rule
(tests/labor_ref.py), array for array with torch.equal -- the rule is integers only, so there is no tolerance anywhere.

The graph is hand-built, 32 * 1024 + 37 nodes (the source bitmap spans two 1024-word tiles): its first nodes have in-degrees 0, 1,
2, 3, 4, 10, 11 (fanout and fanout + 1 for every fanout of the cases below), 255, 256, 257, 1000 and 5000 (the writing kernel's
256-edge chunks are met from both sides), the other nodes 0..12; edge ids are a permutation; columns hold the same source more than
once, also across chunks; seeds are sources of other seeds; and node ids 31, 32, 32767, 32768 and V - 1 are sources."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import labor_ref as ref
from block_invariants import check_index
from test_labor_ref import check_inclusion, inclusion_counts, stat_graph

pytestmark = pytest.mark.gpu

V = 32 * 1024 + 37
DEG = [0, 1, 2, 3, 4, 10, 11, 255, 256, 257, 1000, 5000]
HUB = 11                                                                       # the column of degree 5000
EDGE_IDS = [31, 32, 32767, 32768, V - 1]                                       # bitmap word / tile boundaries
SEED = 1234
GUARD = 8


@functools.lru_cache(maxsize=None)
def graph_np():
    rng = np.random.default_rng(11)
    deg = np.concatenate([np.array(DEG), rng.integers(0, 13, V - len(DEG))])
    indptr = np.zeros(V + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.integers(0, V, int(indptr[-1]))
    indices[indptr[2]:indptr[3]] = [32, 32768]
    indices[indptr[3]:indptr[4]] = [31, 32767, V - 1]
    indices[indptr[4]:indptr[4] + 2] = 20000                                    # a multi-edge: two of node 4's in-edges from 20000
    indices[indptr[5]] = HUB                                                    # seeds that are sources of other seeds
    indices[indptr[5] + 1:indptr[5] + 6] = EDGE_IDS
    a = indptr[HUB]
    indices[a + 3] = 5
    indices[a + 4] = HUB                                                        # and a self-loop
    indices[[a + 7, a + 300, a + 2000]] = 20001                                 # a multi-edge over three chunks of the hub
    indices[a + 10:a + 15] = EDGE_IDS
    eid = rng.permutation(int(indptr[-1]))
    return indptr, indices.astype(np.int32), eid.astype(np.int32)


@functools.lru_cache(maxsize=None)
def seeds_all():
    """1025 distinct seeds, most of them short columns; the first 67 hold every special column."""
    pool = np.setdiff1d(np.arange(len(DEG), V), np.array(EDGE_IDS + [20000, 20001]))
    rest = np.random.default_rng(12).permutation(pool)[:1025 - len(DEG)]
    head = np.random.default_rng(13).permutation(np.concatenate([np.arange(len(DEG)), rest[:67 - len(DEG)]]))
    return tuple(np.concatenate([head, rest[67 - len(DEG):]]).tolist())


def seeds67():
    return seeds_all()[:67]


@functools.lru_cache(maxsize=None)
def ref_layer(seeds, fanout, step, layer):
    ip, ix, ei = graph_np()
    return ref.sample_layer(ip, ix, ei, np.array(seeds, dtype=np.int64), fanout, SEED, step, layer)


@pytest.fixture(scope="module")
def graph_dev(cuda):
    ip, ix, ei = graph_np()
    return torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda), torch.from_numpy(ei).to(cuda)


class Layer:
    """Hand-allocated buffers of direct bliss_labor_layer calls; every output array is followed by guard words."""

    def __init__(self, dev, graph_dev, cap_s, cap_k, cap_b, num_nodes=V):
        from bliss_gnn_amd import _lib
        self.lib, self.dev, self.V = _lib, dev, num_nodes
        self.ip, self.ix, self.ei = graph_dev
        self.cap_s, self.cap_k, self.cap_b = cap_s, cap_k, cap_b
        self.g = _lib.Graph(self.ip.data_ptr(), self.ix.data_ptr(), self.ei.data_ptr(), num_nodes, int(self.ix.numel()))
        self.counts = torch.zeros(20, dtype=torch.int32, device=dev)
        self.fill()
        self.kept_map = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(_lib.lib.bliss_labor_scratch_bytes(num_nodes, cap_s)) // 4, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.tr_bytes = int(_lib.lib.bliss_block_transpose_temp_bytes(cap_b, cap_k))
        self.tr_temp = torch.empty(max(self.tr_bytes, 1), dtype=torch.uint8, device=dev)

    def fill(self):
        dev, cap_s, cap_k, cap_b = self.dev, self.cap_s, self.cap_k, self.cap_b
        i32 = lambda n: torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev)
        self.seg_ptr, self.indptr = i32(cap_s + 1), i32(cap_s + 1)
        self.src, self.dst, self.pos, self.eid = i32(cap_b), i32(cap_b), i32(cap_b), i32(cap_b)
        self.w = torch.full((cap_b + GUARD,), -7.0, dtype=torch.bfloat16, device=dev)
        self.q = torch.full((cap_b + GUARD,), -7.0, dtype=torch.bfloat16, device=dev)
        self.kept_nid = i32(cap_k)
        self.t_indptr, self.t_edge = i32(cap_k + 1), i32(max(cap_b, 1))

    def __call__(self, seeds, fanout, step=0, layer=0, bump=0, ov=None, n_seeds_dev=None, set_step=True, dep=0, cap_b=None):
        _lib = self.lib
        if set_step:
            self.step.fill_(step)
        cap_b = self.cap_b if cap_b is None else cap_b
        n_seeds = -1 if n_seeds_dev is not None else int(seeds.numel())
        cnt_ptr = self.counts.data_ptr()
        ws = _lib.LayerWs(cnt_ptr, self.seg_ptr.data_ptr(), 0, 0, 0, 0, 0, 0, self.kept_nid.data_ptr(), 0, 0, 0, 0, self.cap_k)
        ws.kept_map = self.kept_map.data_ptr()
        out = _lib.BlockOut(self.indptr.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), self.pos.data_ptr(), self.eid.data_ptr(),
                            self.w.data_ptr(), self.q.data_ptr(), 0, 0, 0, cap_b)
        st = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib.bliss_labor_layer(C.byref(self.g), seeds.data_ptr(), n_seeds, 0 if n_seeds_dev is None else n_seeds_dev,
                                        self.cap_s, fanout, 0 if ov is None else ov.data_ptr(), SEED, self.step.data_ptr(), layer,
                                        bump, dep, C.byref(ws), C.byref(out), self.scratch.data_ptr(), st)
        assert rc == 0, rc
        rc = _lib.lib.bliss_block_transpose(self.src.data_ptr(), cnt_ptr + 16, self.cap_b, self.cap_b, self.cap_k,
                                            self.t_indptr.data_ptr(), self.t_edge.data_ptr(), self.tr_temp.data_ptr(), self.tr_bytes, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return _lib.LayerCounts.from_buffer_copy(self.counts[:10].cpu().numpy().tobytes())

    def assert_guards(self, cap_b=None):
        cap_b = self.cap_b if cap_b is None else cap_b
        for name, n in (("seg_ptr", self.cap_s + 1), ("indptr", self.cap_s + 1), ("src", cap_b), ("dst", cap_b),
                        ("pos", cap_b), ("eid", cap_b), ("kept_nid", self.cap_k), ("w", cap_b), ("q", cap_b)):
            assert bool((getattr(self, name)[n:] == -7).all()), "words behind the capacity of %s were overwritten" % name

    def assert_clean(self):
        """What a replay relies on: kept_map all -1, tickets and bitmap all zero."""
        words = -(-(-(-self.V // 32)) // 1024) * 1024
        assert bool((self.kept_map == -1).all()), "kept_map is not clean"
        assert int(self.scratch[:16 + words].abs().sum()) == 0, "tickets / bitmap are not zero"

    def assert_equals(self, c, want):
        dev = self.dev
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
        S, K, B = want["S"], want["K"], want["B"]
        assert (c.S, c.E, c.C, c.K, c.B, c.err) == (S, want["E"], K, K, B, 0), (c.S, c.E, c.C, c.K, c.B, c.err, S, want["E"], K, B)
        assert torch.equal(self.indptr[:S + 1], t(want["indptr"]))
        assert bool((self.indptr[S:self.cap_s + 1] == B).all())                  # the padded rows are empty
        for name in ("pos", "dst", "eid", "src"):
            assert torch.equal(getattr(self, name)[:B], t(want[name])), name
        assert torch.equal(self.kept_nid[:K], t(want["kept_nid"]))
        assert bool((self.kept_nid[K:self.cap_k] == 0).all())
        assert torch.equal(self.t_indptr[:K + 1], t(want["t_indptr"])) and torch.equal(self.t_edge[:B], t(want["t_edge"]))
        assert bool((self.w[:B] == 1).all()) and bool((self.q[:B] == 1).all())
        seg = np.zeros(S + 1, dtype=np.int64)
        ip = self.ip.cpu().numpy()
        nid = np.asarray(want["kept_nid"][:S], dtype=np.int64)
        seg[1:] = np.cumsum(ip[nid + 1] - ip[nid])
        assert torch.equal(self.seg_ptr[:S + 1], t(seg.astype(np.int32)))
        self.assert_guards()
        self.assert_clean()


def _dev(a, cuda, dtype=torch.int32):
    return torch.tensor(list(a), dtype=dtype, device=cuda)


@pytest.fixture(scope="module")
def layer67(cuda, graph_dev):
    return Layer(cuda, graph_dev, 80, 8000, 8000)


@pytest.mark.parametrize("fanout", [-1, 1, 3, 10])
def test_one_layer_of_67_seeds_and_of_one(cuda, graph_dev, layer67, fanout):
    seeds = _dev(seeds67(), cuda)
    for step, layer in ((0, 0), (5, 2)):
        want = ref_layer(seeds67(), fanout, step, layer)
        assert want["B"] < 8000 and want["K"] < 8000
        layer67.assert_equals(layer67(seeds, fanout, step=step, layer=layer), want)
    c = layer67(seeds, fanout, step=0, layer=0)                                  # again on the same scratch: nothing was left behind
    layer67.assert_equals(c, ref_layer(seeds67(), fanout, 0, 0))
    want = ref_layer((HUB,), fanout, 3, 1)                                       # S = 1: the hub alone, exact capacities
    one = Layer(cuda, graph_dev, 1, want["K"], max(want["B"], 1))
    one.assert_equals(one(_dev([HUB], cuda), fanout, step=3, layer=1), want)
    if fanout < 0:
        assert want["B"] == 5000


def test_layer_dependency_flag_draws_with_layer_zero(cuda, layer67):
    seeds = _dev(seeds67(), cuda)
    layer67.assert_equals(layer67(seeds, 3, step=5, layer=2, dep=1), ref_layer(seeds67(), 3, 5, 0))
    assert not np.array_equal(ref_layer(seeds67(), 3, 5, 0)["pos"], ref_layer(seeds67(), 3, 5, 2)["pos"])


@pytest.mark.parametrize("S", [1, 1023, 1024, 1025])
def test_scan_trips(cuda, graph_dev, S):
    seeds = seeds_all()[:S]
    want = ref_layer(seeds, 3, 2, 1)
    lay = Layer(cuda, graph_dev, S, want["K"], max(want["B"], 1))                 # exact capacities
    lay.assert_equals(lay(_dev(seeds, cuda), 3, step=2, layer=1), want)


@pytest.mark.parametrize("count", [0, 1, 67])
def test_seed_count_read_on_the_device(cuda, graph_dev, count):
    seeds = seeds67()[:count]
    want = ref_layer(seeds, 3, 4, 0)
    lay = Layer(cuda, graph_dev, 67, 8000, 8000)
    n_dev = _dev([-5, count, -5], cuda)
    c = lay(_dev(seeds67(), cuda), 3, step=4, layer=0, bump=1, n_seeds_dev=n_dev.data_ptr() + 4)
    lay.assert_equals(c, want)
    assert int(lay.step.item()) == 5                                              # bumped once, by one workgroup
    if count == 0:
        assert (c.S, c.K, c.B) == (0, 0, 0)


def test_second_layer_reads_its_seeds_from_the_first(cuda, graph_dev):
    ip, ix, ei = graph_np()
    lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()[:9]), [3, 3], SEED, 4)
    first = Layer(cuda, graph_dev, 16, 200, 400)
    first.assert_equals(first(_dev(seeds67()[:9], cuda), 3, step=4, layer=0), lays[0])
    second = Layer(cuda, graph_dev, 200, 2000, 2000)
    # the seeds are the first layer's kept nodes (capacity-padded), their number is the K of its counts record
    c1 = second(first.kept_nid[:200], 3, step=4, layer=1, bump=1, n_seeds_dev=first.counts.data_ptr() + 12)
    second.assert_equals(c1, lays[1])
    assert int(second.step.item()) == 5


def test_planted_keys(cuda, graph_dev, layer67):
    ip, ix, ei = graph_np()
    seeds, sl = _dev(seeds67(), cuda), list(seeds67())
    six, ten, hub = sl.index(6), sl.index(10), sl.index(HUB)
    a = int(ip[HUB])
    full, none, pair = ix[ip[6]:ip[7]], ix[ip[10]:ip[11]], ix[a + 20:a + 22]
    assert not np.isin(none, full).any() and pair[0] != pair[1] and not np.isin(pair, np.concatenate([full, none])).any()
    ov = np.random.default_rng(14).integers(0, 2 ** 32, V, dtype=np.uint64).astype(np.uint32)
    ov[full] = 0                                                                  # the column of degree 11 keeps everything
    ov[none] = 0xFFFFFFFF                                                         # the column of degree 1000 keeps NOTHING
    thr = ref.threshold(3, 5000)
    ov[pair[0]], ov[pair[1]] = thr - 1, thr                                       # the strict threshold, in the hub
    want = ref.sample_layer(ip, ix, ei, np.array(sl), 3, SEED, 0, 0, keys_override=ov)
    assert want["indptr"][six + 1] - want["indptr"][six] == 11
    assert want["indptr"][ten + 1] == want["indptr"][ten] and ten + 1 < 67        # indptr repeats ...
    layer67.assert_equals(layer67(seeds, 3, ov=torch.from_numpy(ov.view(np.int32)).to(cuda)), want)    # ... the next column lands right
    kept = set(layer67.pos[want["indptr"][hub]:want["indptr"][hub + 1]].cpu().tolist())
    assert a + 20 in kept and a + 21 not in kept


def test_edge_capacity_below_the_true_count(cuda, graph_dev):
    """Bounds handling: the bit is raised, nothing is written behind the capacity, and the scratch is left clean."""
    want = ref_layer(seeds67(), 3, 0, 0)
    seeds = _dev(seeds67(), cuda)
    lay = Layer(cuda, graph_dev, 67, want["K"], want["B"])
    short = want["B"] - 40
    c = lay(seeds, 3, cap_b=short)
    assert c.err == 8 and c.B == short and c.S == 67
    check_index(lay.src.cpu(), lay.t_indptr.cpu(), lay.t_edge.cpu(), c.K, c.B, lay.cap_k)             # clamped, and still walkable
    lay.assert_guards(cap_b=short)                                                # (the words [short, B) of the arrays are guards too)
    lay.assert_clean()
    t = lambda x: torch.from_numpy(np.asarray(x)).to(cuda)
    ncol = int(np.searchsorted(want["indptr"], short, side="right")) - 1          # columns that fit whole are the restatement's
    nb = int(want["indptr"][ncol])
    assert torch.equal(lay.indptr[:ncol + 1], t(want["indptr"][:ncol + 1])) and bool((lay.indptr[ncol + 1:68] <= short).all())
    assert torch.equal(lay.pos[:nb], t(want["pos"][:nb])) and torch.equal(lay.dst[:nb], t(want["dst"][:nb]))
    # no source was marked for an edge that was not written: K counts the seeds and the sources of written edges only
    ip, ix, _ = graph_np()
    written = lay.pos[:short].cpu().numpy()
    assert c.K == len(np.union1d(np.array(seeds67()), ix[written]))
    lay.assert_equals(lay(seeds, 3), want)                                        # the following call, with room: the restatement's
    short_k = Layer(cuda, graph_dev, 67, want["K"] - 1, want["B"])
    c = short_k(seeds, 3)
    assert c.err == 4 and c.K == want["K"] - 1 and c.B == want["B"]
    short_k.assert_guards()
    short_k.assert_clean()
    check_index(short_k.src.cpu(), short_k.t_indptr.cpu(), short_k.t_edge.cpu(), c.K, c.B, short_k.cap_k)     # clamped, and still walkable
    short_s = Layer(cuda, graph_dev, 66, want["K"], want["B"])
    c = short_s(seeds, 3)
    assert c.err & 64 and c.S == 66
    short_s.assert_guards()
    short_s.assert_clean()
    check_index(short_s.src.cpu(), short_s.t_indptr.cpu(), short_s.t_edge.cpu(), c.K, c.B, short_s.cap_k)     # clamped, and still walkable


def test_two_runs_of_twenty_launches_are_bit_equal(cuda, graph_dev, layer67):
    seeds = _dev(seeds67(), cuda)
    runs = []
    for _ in range(2):
        got = []
        for t in range(20):
            c = layer67(seeds, 3, step=100, layer=1, bump=1, set_step=t == 0)
            got.append(torch.cat([layer67.counts[:6], layer67.indptr[:68], layer67.pos[:c.B], layer67.src[:c.B], layer67.eid[:c.B],
                                  layer67.kept_nid[:c.K], layer67.t_edge[:c.B]]).clone())
        assert int(layer67.step.item()) == 120
        runs.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], runs[0][1])                                # (the step does change the draw)
    layer67.assert_equals(layer67(seeds, 3, step=119, layer=1), ref_layer(seeds67(), 3, 119, 1))


def test_inclusion_frequencies_on_the_device(cuda):
    """The column of the CPU statistics test, 2048 draw steps counted by the device's own step counter: the rule is
    deterministic, so the counts are the restatement's integers."""
    ip, ix = stat_graph()
    n = len(ip) - 1
    gd = (torch.from_numpy(ip).to(cuda), torch.from_numpy(ix.astype(np.int32)).to(cuda), torch.arange(8, dtype=torch.int32, device=cuda))
    lay = Layer(cuda, gd, 1, 9, 8, num_nodes=n)
    seeds = torch.zeros(1, dtype=torch.int32, device=cuda)
    hits = torch.zeros(8, dtype=torch.int64, device=cuda)
    one = torch.ones(8, dtype=torch.int64, device=cuda)
    empty = 0
    for t in range(2048):
        c = lay(seeds, 3, layer=1, bump=1, set_step=t == 0)
        assert c.err == 0 and c.K == 1 + c.B
        hits.index_add_(0, lay.pos[:c.B].long(), one[:c.B])
        empty += c.B == 0
    assert int(lay.step.item()) == 2048
    hits = hits.cpu().numpy()
    want_hits, want_empty = inclusion_counts()
    assert np.array_equal(hits, want_hits) and empty == want_empty
    check_inclusion(hits, empty)
    lay.assert_clean()


# ------------------------------------------------------------------------------------------------- through the sampler
def test_sage_forward_over_a_block_with_an_empty_column(cuda, graph_dev):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.nn import SAGEConv, weighted_aggregate
    ip, ix, ei = graph_dev
    g = bg.Graph(ip, ix, ei)
    want = ref_layer(seeds67(), 1, 0, 0)
    deg = np.diff(graph_np()[0])[np.array(seeds67())]
    c = np.diff(want["indptr"])
    rows = np.nonzero((c == 0) & (deg > 1))[0]
    assert len(rows) > 0                                                          # columns above the fanout that keep nothing
    s = fit.LaborSampler([1], seed=SEED)
    _, _, blocks = s.sample_blocks(g, _dev(seeds67(), cuda))
    blk = blocks[0]
    assert torch.equal(blk.indptr, torch.from_numpy(want["indptr"]).to(cuda)) and blk.num_src_nodes() == want["K"]
    torch.manual_seed(3)
    h = torch.randn(blk.num_src_nodes(), 16, device=cuda).bfloat16()
    agg = weighted_aggregate(blk, h, blk.edata["edge_weights"], mean=True)
    assert bool(torch.isfinite(agg.float()).all()) and bool((agg[torch.from_numpy(rows).to(cuda)] == 0).all())
    full = np.nonzero(c > 0)[0]
    assert bool((agg[torch.from_numpy(full).to(cuda)].float().abs().sum(1) > 0).all())
    conv = SAGEConv(16, 24, "mean").to(cuda).bfloat16()
    out = conv(blk, h, blk.edata["edge_weights"])
    assert out.shape == (67, 24) and bool(torch.isfinite(out.float()).all())
    r = torch.from_numpy(rows).to(cuda)
    assert torch.equal(out[r], conv.fc_self(h[:67])[r])                           # the neighbour term of an empty column is zero
