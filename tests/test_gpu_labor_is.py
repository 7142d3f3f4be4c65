"""GPU suite (-m gpu): the device-side LABOR-i sampler (csrc/labor_is.hip) against the CPU restatement of its rule
(tests/labor_is_ref.py), array for array with torch.equal -- the rule is unsigned integers up to the weights, and q_ij is two
defined roundings of an integer.  ``edge_weights`` are fp64 on both sides, summed in different orders and rounded once to bf16:
at most one bf16 ulp per element, and per column |sum W - k| <= k * 2^-8 (half a bf16 ulp per term).

Two graphs: tests/test_gpu_labor.py's (in-degrees 0 .. 5000, the bitmap's tile boundary), and a column-degree graph whose seed
columns have degrees 0, 1, 3, 4, 255, 256, 257 (the wave-per-column bound of the scale solve), 2047, 2048, 2049 (its LDS staging
bound) and 5000, with sources drawn from a small pool so that most are shared between columns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import labor_is_ref as ref
from block_invariants import check_index
import test_labor_is_ref as cpu
from test_gpu_labor import GUARD, HUB, SEED, V, Layer as Layer0, graph_np, seeds67, seeds_all

pytestmark = pytest.mark.gpu

ONE = ref.ONE
CV = 6000                                                                      # nodes of the column-degree graph
CDEG = [0, 1, 3, 4, 255, 256, 257, 2047, 2048, 2049, 5000]


@functools.lru_cache(maxsize=None)
def column_graph_np():
    rng = np.random.default_rng(21)
    deg = np.zeros(CV, dtype=np.int64)
    deg[:len(CDEG)] = CDEG
    deg[len(CDEG):40] = rng.integers(0, 9, 40 - len(CDEG))
    indptr = np.zeros(CV + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.integers(40, 3000, int(indptr[-1]))
    indices[indptr[2]:indptr[3]] = [100, 101, 102]                              # a whole column (d = 3 = fanout) ...
    indices[indptr[3]:indptr[3] + 2] = [100, 5]                                 # ... sharing 100 with a non-whole one; seed 5 is a source
    indices[indptr[4]:indptr[4] + 3] = [200, 101, 200]                          # a multi-edge, and 101 shared with the whole column
    a = indptr[10]
    indices[[a + 7, a + 300, a + 2000]] = 201                                   # a multi-edge over three chunks of the hub
    indices[a + 9] = 4                                                          # seeds that are sources of other seeds
    indices[indptr[8] + 5] = 10
    indices[indptr[7] + 2] = CV - 1
    eid = rng.permutation(int(indptr[-1]))
    return indptr, indices.astype(np.int32), eid.astype(np.int32)


def column_seeds():
    return tuple(np.random.default_rng(22).permutation(40).tolist())


GRAPHS = {"big": graph_np, "col": column_graph_np}


@functools.lru_cache(maxsize=None)
def ref_layer(graph, seeds, fanout, step, layer, iters):
    ip, ix, ei = GRAPHS[graph]()
    return ref.sample_layer(ip, ix, ei, np.array(seeds, dtype=np.int64), fanout, SEED, step, layer, iters)


@pytest.fixture(scope="module")
def graph_dev(cuda):
    return tuple(torch.from_numpy(a).to(cuda) for a in graph_np())


@pytest.fixture(scope="module")
def col_dev(cuda):
    return tuple(torch.from_numpy(a).to(cuda) for a in column_graph_np())


def bits(x):
    return x.view(torch.int16).to(torch.int32) & 0xFFFF


class Layer(Layer0):
    """Hand-allocated buffers of direct bliss_labor_is_layer calls (tests/test_gpu_labor.py's, with this sampler's scratch)."""

    def __init__(self, dev, graph_dev, cap_s, cap_k, cap_b, num_nodes=V):
        super().__init__(dev, graph_dev, cap_s, cap_k, cap_b, num_nodes)
        nbytes = int(self.lib.lib.bliss_labor_is_scratch_bytes(num_nodes, cap_s, cap_b))
        assert nbytes > 0 and nbytes % 16 == 0
        self.scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)

    def __call__(self, seeds, fanout, iters, step=0, layer=0, bump=0, ov=None, n_seeds_dev=None, set_step=True, dep=0, cap_b=None,
                 sync=True):
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
        rc = _lib.lib.bliss_labor_is_layer(C.byref(self.g), seeds.data_ptr(), n_seeds, 0 if n_seeds_dev is None else n_seeds_dev,
                                           self.cap_s, fanout, 0 if ov is None else ov.data_ptr(), SEED, self.step.data_ptr(), layer,
                                           bump, dep, iters, C.byref(ws), C.byref(out), self.scratch.data_ptr(), st)
        assert rc == 0, rc
        rc = _lib.lib.bliss_block_transpose(self.src.data_ptr(), cnt_ptr + 16, self.cap_b, self.cap_b, self.cap_k,
                                            self.t_indptr.data_ptr(), self.t_edge.data_ptr(), self.tr_temp.data_ptr(), self.tr_bytes, st)
        assert rc == 0, rc
        if not sync:
            return None
        torch.cuda.synchronize()
        return _lib.LayerCounts.from_buffer_copy(self.counts[:10].cpu().numpy().tobytes())

    def assert_clean(self):
        """What a replay relies on: kept_map all -1; tickets, bitmap and BOTH importance buffers all zero (read back)."""
        words = -(-(-(-self.V // 32)) // 1024) * 1024
        assert bool((self.kept_map == -1).all()), "kept_map is not clean"
        assert int(self.scratch[:16 + words].abs().sum()) == 0, "tickets / bitmap are not zero"
        o = 16 + words + words // 1024
        assert int((self.scratch[o:o + 2 * self.V] != 0).sum()) == 0, "an importance buffer is not idle"

    def assert_weights(self, want):
        """q_ij bit for bit; edge_weights within one bf16 ulp of the restatement's, each column's summing to its kept count."""
        dev, B, S = self.dev, want["B"], want["S"]
        assert torch.equal(bits(self.q[:B]), torch.from_numpy(want["q_ij"].astype(np.int32)).to(dev))
        got = bits(self.w[:B])
        wb = torch.from_numpy(ref.bf16_of_f64(want["edge_weights"]).astype(np.int32)).to(dev)
        worst = int((got - wb).abs().max()) if B else 0
        assert worst <= 1, "edge_weights differ by %d bf16 ulps" % worst
        whole = torch.from_numpy(want["p_e"] == np.uint64(ONE)).to(dev)
        assert bool((got[whole] == 0x3F80).all())                                # exactly 1 in whole columns
        w = self.w[:B].double().cpu().numpy()
        ip = want["indptr"].astype(np.int64)
        k = np.diff(ip)
        sums = np.add.reduceat(np.concatenate([w, [0.0]]), np.minimum(ip[:-1], B))[:S] * (k > 0) if S else np.zeros(0)
        dev_max = float(np.max(np.abs(sums - k) / np.maximum(k, 1))) if S else 0.0
        assert bool((np.abs(sums - k) <= k * 2.0 ** -8).all()), "a column's weights sum to k (1 + %.3g)" % dev_max

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
        self.assert_weights(want)
        seg = np.zeros(S + 1, dtype=np.int64)
        ip = self.ip.cpu().numpy()
        nid = np.asarray(want["kept_nid"][:S], dtype=np.int64)
        seg[1:] = np.cumsum(ip[nid + 1] - ip[nid])
        assert torch.equal(self.seg_ptr[:S + 1], t(seg.astype(np.int32)))
        self.assert_guards()
        self.assert_clean()

    def snapshot(self, c, S):
        return torch.cat([self.counts[:6], self.indptr[:S + 1], self.pos[:c.B], self.src[:c.B], self.eid[:c.B], self.kept_nid[:c.K],
                          self.t_edge[:c.B], bits(self.w[:c.B]), bits(self.q[:c.B])]).clone()


def _dev(a, cuda, dtype=torch.int32):
    return torch.tensor(list(a), dtype=dtype, device=cuda)


@pytest.fixture(scope="module")
def layer67(cuda, graph_dev):
    return Layer(cuda, graph_dev, 80, 8000, 8000)


@pytest.fixture(scope="module")
def labor0(cuda, graph_dev):
    return Layer0(cuda, graph_dev, 80, 8000, 8000)


# ------------------------------------------------------------------------------------------------- one layer
@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("fanout", [-1, 1, 3, 10])
def test_one_layer_of_67_seeds_and_of_one(cuda, graph_dev, layer67, labor0, fanout, iters):
    seeds = _dev(seeds67(), cuda)
    for step, layer in ((0, 0), (5, 2)):
        want = ref_layer("big", seeds67(), fanout, step, layer, iters)
        assert want["B"] < 8000 and want["K"] < 8000
        layer67.assert_equals(layer67(seeds, fanout, iters, step=step, layer=layer), want)
    c = layer67(seeds, fanout, iters, step=0, layer=0)                           # again on the same scratch: nothing was left behind
    layer67.assert_equals(c, ref_layer("big", seeds67(), fanout, 0, 0, iters))
    if iters == 0:                                                               # LABOR-0 through these kernels: bliss_labor_layer's output
        c0 = labor0(seeds, fanout, step=0, layer=0)
        assert (c0.S, c0.E, c0.K, c0.B, c0.err) == (c.S, c.E, c.K, c.B, c.err)
        for name, n in (("indptr", 81), ("kept_nid", 8000), ("seg_ptr", c.S + 1), ("src", c.B), ("dst", c.B), ("pos", c.B), ("eid", c.B),
                        ("t_indptr", c.K + 1), ("t_edge", c.B)):
            assert torch.equal(getattr(layer67, name)[:n], getattr(labor0, name)[:n]), name
        assert torch.equal(bits(layer67.w[:c.B]), bits(labor0.w[:c.B]))
    want = ref_layer("big", (HUB,), fanout, 3, 1, iters)                         # S = 1: the hub alone, exact capacities
    one = Layer(cuda, graph_dev, 1, want["K"], max(want["B"], 1))
    one.assert_equals(one(_dev([HUB], cuda), fanout, iters, step=3, layer=1), want)
    if iters and fanout > 0:
        assert len(set(ref_layer("big", seeds67(), fanout, 0, 0, iters)["p_e"].tolist())) > 10      # (not LABOR-0's thresholds)


def test_layer_dependency_flag_draws_with_layer_zero(cuda, layer67):
    seeds = _dev(seeds67(), cuda)
    layer67.assert_equals(layer67(seeds, 3, 2, step=5, layer=2, dep=1), ref_layer("big", seeds67(), 3, 5, 0, 2))
    assert not np.array_equal(ref_layer("big", seeds67(), 3, 5, 0, 2)["pos"], ref_layer("big", seeds67(), 3, 5, 2, 2)["pos"])


@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("fanout", [1, 3, 10])
def test_column_degree_graph(cuda, col_dev, fanout, iters):
    ip, ix, _ = column_graph_np()
    sl = list(column_seeds())
    deg = np.diff(ip)[np.array(sl)]
    assert set(CDEG) <= set(deg.tolist()) and 255 == deg[sl.index(4)] and 2048 == deg[sl.index(8)]
    want = ref_layer("col", column_seeds(), fanout, 2, 1, iters)
    lay = Layer(cuda, col_dev, 40, want["K"], max(want["B"], 1), num_nodes=CV)    # exact capacities
    lay.assert_equals(lay(_dev(sl, cuda), fanout, iters, step=2, layer=1), want)
    if fanout == 3 and iters:
        # a source shared by a whole and a non-whole column has importance ONE: its probability there is the column's scale
        o = int(np.cumsum(np.concatenate([[0], deg]))[sl.index(3)])
        assert int(want["p"][o]) == (int(want["c"][sl.index(3)]) * ONE) >> 32 and int(want["p"][o]) > int(want["p"][o + 2])
        # the multi-edge is one source: equal probabilities, kept or dropped as one
        o = int(np.cumsum(np.concatenate([[0], deg]))[sl.index(4)])
        assert int(want["p"][o]) == int(want["p"][o + 2])
        kept = set(want["pos"].tolist())
        assert (int(ip[4]) in kept) == (int(ip[4]) + 2 in kept)


# ------------------------------------------------------------------------------------------------- seed counts and layers
@pytest.mark.parametrize("S", [1, 1023, 1024, 1025])
def test_scan_trips(cuda, graph_dev, S):
    seeds = seeds_all()[:S]
    want = ref_layer("big", seeds, 3, 2, 1, 1)
    lay = Layer(cuda, graph_dev, S, want["K"], max(want["B"], 1))                 # exact capacities
    lay.assert_equals(lay(_dev(seeds, cuda), 3, 1, step=2, layer=1), want)


def test_more_seeds_than_the_grids(cuda, graph_dev):
    """4200 columns: more than the 2048 workgroups of the per-column kernels and the 4 * 1024 columns of one trip of the
    wave-per-column kernels, so every stride loop takes a second trip."""
    rest = np.setdiff1d(np.arange(V), np.array(seeds_all()))
    seeds = tuple(seeds_all()) + tuple(np.random.default_rng(23).permutation(rest)[:4200 - 1025].tolist())
    assert len(set(seeds)) == 4200
    want = ref_layer("big", seeds, 3, 1, 0, 1)
    lay = Layer(cuda, graph_dev, 4200, want["K"], want["B"])
    lay.assert_equals(lay(_dev(seeds, cuda), 3, 1, step=1, layer=0), want)


@pytest.mark.parametrize("count", [0, 1, 67])
def test_seed_count_read_on_the_device(cuda, graph_dev, count):
    seeds = seeds67()[:count]
    want = ref_layer("big", seeds, 3, 4, 0, 2)
    lay = Layer(cuda, graph_dev, 67, 8000, 8000)
    n_dev = _dev([-5, count, -5], cuda)
    c = lay(_dev(seeds67(), cuda), 3, 2, step=4, layer=0, bump=1, n_seeds_dev=n_dev.data_ptr() + 4)
    lay.assert_equals(c, want)
    assert int(lay.step.item()) == 5                                              # bumped once, by one workgroup
    if count == 0:
        assert (c.S, c.K, c.B) == (0, 0, 0)


def test_second_layer_reads_its_seeds_from_the_first(cuda, graph_dev):
    ip, ix, ei = graph_np()
    lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()[:9]), [3, 3], SEED, 4, 2)
    first = Layer(cuda, graph_dev, 16, 200, 400)
    first.assert_equals(first(_dev(seeds67()[:9], cuda), 3, 2, step=4, layer=0), lays[0])
    second = Layer(cuda, graph_dev, 200, 2000, 2000)
    # the seeds are the first layer's kept nodes (capacity-padded), their number is the K of its counts record
    c1 = second(first.kept_nid[:200], 3, 2, step=4, layer=1, bump=1, n_seeds_dev=first.counts.data_ptr() + 12)
    second.assert_equals(c1, lays[1])
    assert int(second.step.item()) == 5


def test_a_seed_id_out_of_range_is_an_empty_column(cuda, graph_dev):
    sl = list(seeds67()[:20])
    bad = sl[:7] + [V + 5] + sl[7:15] + [-3] + sl[15:]
    want = ref_layer("big", tuple(sl), 3, 6, 0, 2)
    lay = Layer(cuda, graph_dev, 32, 2000, 2000)
    c = lay(_dev(bad, cuda), 3, 2, step=6, layer=0)
    assert c.err == 2 and (c.S, c.E, c.B, c.K) == (22, want["E"], want["B"], want["K"] + 2)
    k = np.diff(want["indptr"])
    k = np.concatenate([k[:7], [0], k[7:15], [0], k[15:]])
    assert np.array_equal(np.diff(lay.indptr[:23].cpu().numpy()), k)
    B = want["B"]
    assert torch.equal(lay.pos[:B], torch.from_numpy(want["pos"]).to(cuda))
    ix = torch.from_numpy(graph_np()[1]).to(cuda)
    assert torch.equal(lay.kept_nid[lay.src[:B].long()], ix[lay.pos[:B].long()])
    assert lay.kept_nid[:22].cpu().tolist() == bad
    assert torch.equal(bits(lay.q[:B]), torch.from_numpy(want["q_ij"].astype(np.int32)).to(cuda))
    assert int((bits(lay.w[:B]) - torch.from_numpy(ref.bf16_of_f64(want["edge_weights"]).astype(np.int32)).to(cuda)).abs().max()) <= 1
    lay.assert_guards()
    lay.assert_clean()
    lay.assert_equals(lay(_dev(sl, cuda), 3, 2, step=6, layer=0), want)           # the following call is the restatement's


# ------------------------------------------------------------------------------------------------- planted keys
def test_planted_keys(cuda, graph_dev, layer67):
    ip, ix, ei = graph_np()
    seeds, sl = _dev(seeds67(), cuda), list(seeds67())
    base = ref_layer("big", seeds67(), 3, 0, 0, 2)
    seg = np.concatenate([[0], np.cumsum(np.diff(ip)[np.array(sl)])])
    hub, ten = sl.index(HUB), sl.index(10)
    a = int(ip[HUB])
    full, none, pair = ix[ip[6]:ip[7]], ix[ip[10]:ip[11]], ix[a + 20:a + 22]
    assert not np.isin(none, full).any() and pair[0] != pair[1] and not np.isin(pair, np.concatenate([full, none])).any()
    p_pair = [int(x) for x in base["p"][seg[hub] + 20:seg[hub] + 22]]
    assert all(1 <= x < ONE - 1 for x in p_pair)
    ov = np.random.default_rng(14).integers(0, 2 ** 32, V, dtype=np.uint64).astype(np.uint32)
    ov[full] = 0                                                                  # the column of degree 11 keeps everything (p >= 1)
    ov[none] = 0xFFFFFFFF                                                         # the column of degree 1000 keeps NOTHING (p < ONE)
    ov[pair[0]], ov[pair[1]] = p_pair[0] - 1, p_pair[1]                           # the strict comparison, in the hub
    want = ref.sample_layer(ip, ix, ei, np.array(sl), 3, SEED, 0, 0, 2, keys_override=ov)
    assert np.array_equal(want["p"], base["p"])                                   # (the probabilities do not depend on the keys)
    six = sl.index(6)
    assert want["indptr"][six + 1] - want["indptr"][six] == 11 and want["indptr"][ten + 1] == want["indptr"][ten]
    layer67.assert_equals(layer67(seeds, 3, 2, ov=torch.from_numpy(ov.view(np.int32)).to(cuda)), want)
    kept = set(layer67.pos[want["indptr"][hub]:want["indptr"][hub + 1]].cpu().tolist())
    assert a + 20 in kept and a + 21 not in kept


# ------------------------------------------------------------------------------------------------- state left clean
def test_edge_capacity_below_the_true_count(cuda, graph_dev):
    """Bounds handling: the bit is raised, nothing is written behind the capacity, and every |V|-sized word is left idle."""
    want = ref_layer("big", seeds67(), 3, 0, 0, 2)
    seeds = _dev(seeds67(), cuda)
    lay = Layer(cuda, graph_dev, 67, want["K"], want["B"])
    short = want["B"] - 40
    c = lay(seeds, 3, 2, cap_b=short)
    assert c.err == 8 and c.B == short and c.S == 67
    check_index(lay.src.cpu(), lay.t_indptr.cpu(), lay.t_edge.cpu(), c.K, c.B, lay.cap_k)             # clamped, and still walkable
    lay.assert_guards(cap_b=short)                                                # (the words [short, B) of the arrays are guards too)
    lay.assert_clean()
    t = lambda x: torch.from_numpy(np.asarray(x)).to(cuda)
    ncol = int(np.searchsorted(want["indptr"], short, side="right")) - 1          # columns that fit whole are the restatement's
    nb = int(want["indptr"][ncol])
    assert torch.equal(lay.indptr[:ncol + 1], t(want["indptr"][:ncol + 1])) and bool((lay.indptr[ncol + 1:68] <= short).all())
    assert torch.equal(lay.pos[:nb], t(want["pos"][:nb])) and torch.equal(lay.dst[:nb], t(want["dst"][:nb]))
    assert torch.equal(bits(lay.q[:nb]), t(want["q_ij"][:nb].astype(np.int32)))
    # no source was marked for an edge that was not written: K counts the seeds and the sources of written edges only
    ip, ix, _ = graph_np()
    written = lay.pos[:short].cpu().numpy()
    assert c.K == len(np.union1d(np.array(seeds67()), ix[written]))
    lay.assert_equals(lay(seeds, 3, 2), want)                                     # the following call, with room: the restatement's
    short_k = Layer(cuda, graph_dev, 67, want["K"] - 1, want["B"])
    c = short_k(seeds, 3, 2)
    assert c.err == 4 and c.K == want["K"] - 1 and c.B == want["B"]
    short_k.assert_guards()
    short_k.assert_clean()
    check_index(short_k.src.cpu(), short_k.t_indptr.cpu(), short_k.t_edge.cpu(), c.K, c.B, short_k.cap_k)     # clamped, and still walkable
    short_s = Layer(cuda, graph_dev, 66, want["K"], want["B"])
    c = short_s(seeds, 3, 2)
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
            c = layer67(seeds, 3, 2, step=100, layer=1, bump=1, set_step=t == 0)
            got.append(layer67.snapshot(c, 67))
        assert int(layer67.step.item()) == 120
        runs.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], runs[0][1])                                # (the step does change the draw)
    layer67.assert_equals(layer67(seeds, 3, 2, step=119, layer=1), ref_layer("big", seeds67(), 3, 119, 1, 2))


def test_inclusion_frequencies_on_the_device(cuda):
    """The layer of the CPU statistics test, 2048 draw steps counted by the device's own step counter: the rule is
    deterministic, so the counts are the restatement's integers."""
    ip, ix = cpu.stat_graph()
    n, E = len(ip) - 1, len(ix)
    gd = (torch.from_numpy(ip).to(cuda), torch.from_numpy(ix.astype(np.int32)).to(cuda), torch.arange(E, dtype=torch.int32, device=cuda))
    lay = Layer(cuda, gd, 3, 3 + E, E, num_nodes=n)
    seeds = torch.arange(3, dtype=torch.int32, device=cuda)
    hits = torch.zeros(E, dtype=torch.int64, device=cuda)
    one = torch.ones(E, dtype=torch.int64, device=cuda)
    for t in range(cpu.STAT_STEPS):
        lay(seeds, 3, cpu.STAT_ITERS, layer=cpu.STAT_LAYER, bump=1, set_step=t == 0, sync=False)
        hits.index_add_(0, lay.pos[:E].long().clamp(0, E - 1), one * (torch.arange(E, device=cuda) < lay.counts[4]))
    torch.cuda.synchronize()
    assert int(lay.step.item()) == cpu.STAT_STEPS and int(lay.counts[5]) == 0
    want_hits, p = cpu.inclusion_counts()
    assert np.array_equal(hits.cpu().numpy(), want_hits)
    cpu.check_inclusion(hits.cpu().numpy(), p)
    lay.assert_clean()
