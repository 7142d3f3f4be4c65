"""GPU suite (-m gpu): the weighted device-side LABOR sampler (csrc/labor_w.hip) against the CPU restatement of its rule
(tests/wlabor_ref.py), array for array with torch.equal -- the rule is unsigned integers from the bf16 bits of the edge
probabilities up to the weights; q_ij is the probability itself and p_ij two defined roundings of an integer.  ``edge_weights``
are fp64 on both sides, summed in different orders and rounded once to bf16: at most one bf16 ulp per element, and per column
|sum W - k| <= k * 2^-8 (half a bf16 ulp per term).

Two graphs: tests/test_labor_is_ref.py's 400-node lognormal graph with its 64 seeds (both modes, ``layer_dependency`` on and off),
and a hand-built column graph: d = fanout and fanout + 1, an all-zero column, one dominant edge (the clamp at ONE - 1), negative /
NaN / infinite / subnormal probabilities, a ratio that shifts a weight out (>= 32 bits), a multi-edge, and degrees 256, 257, 2048,
2049 on either side of the two path thresholds of the scale kernel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_wlabor_ref as cpu
import wlabor_ref as ref
from block_invariants import check_index
from test_gpu_labor import SEED, Layer as Layer0
from test_labor_is_ref import lognormal_graph

pytestmark = pytest.mark.gpu

ONE = ref.ONE
ETA = 0.4
F = 3                                                                          # the fanout of the hand-built columns
CV = 3000
CDEG = [3, 4, 8, 8, 8, 6, 8, 256, 257, 2048, 2049, 0]                          # columns 0 .. 11 of the column graph
WHOLE, PLUS1, ZEROS, DOMINANT, SPECIAL, SHIFT, MULTI = range(7)


def rbf(x):
    return ref.wneighbor_ref.rbf(np.asarray(x, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def log_graph():
    indptr, indices, seeds = lognormal_graph()
    E = int(indptr[-1])
    eid = np.random.default_rng(31).permutation(E).astype(np.int32)
    q = cpu.random_q(E)                                                         # raw mode: zeros, a NaN, an infinity, a negative, a subnormal
    w = rbf(np.exp2(np.random.default_rng(3).uniform(-8, 4, E)))                # EXP3 mode: positive weights over twelve octaves
    return indptr, indices.astype(np.int32), eid, tuple(int(s) for s in seeds), q, w


@functools.lru_cache(maxsize=None)
def col_graph():
    rng = np.random.default_rng(41)
    deg = np.zeros(CV, dtype=np.int64)
    deg[:len(CDEG)] = CDEG
    indptr = np.zeros(CV + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    E = int(indptr[-1])
    indices = rng.integers(40, CV, E)
    q = rbf(np.exp2(rng.uniform(-6, 3, E)))
    col = lambda c: slice(int(indptr[c]), int(indptr[c + 1]))
    q[col(ZEROS)] = 0.0
    q[col(DOMINANT)] = [1.0, 1.0, 100.0, 1.0, 1.0, 0.5, 1.0, 1.0]
    q[col(SPECIAL)] = [np.nan, -1.0, np.inf, 2.0 ** -130, 1.0, 0.5, -0.0, 3.0]
    q[col(SHIFT)] = [1.0, 2.0 ** -40, 2.0 ** -30, 2.0 ** -31, 3.0, 2.0]
    a = int(indptr[MULTI])
    indices[[a, a + 2, a + 5]] = 77                                             # a multi-edge: one source, three probabilities
    indices[int(indptr[9]) + 5] = 3                                             # seeds that are sources of other seeds
    indices[int(indptr[8]) + 2] = CV - 1
    indices[int(indptr[PLUS1])] = 77                                            # the multi-edge's source, shared with another column
    eid = rng.permutation(E).astype(np.int32)
    w = rbf(np.exp2(rng.uniform(-8, 4, E)))
    return indptr, indices.astype(np.int32), eid, tuple(range(len(CDEG))), q, w


GRAPHS = {"log": log_graph, "col": col_graph}


@functools.lru_cache(maxsize=None)
def q_pos_of(graph, mode, seeds):
    ip, _, _, _, q, w = GRAPHS[graph]()
    return q if mode == 0 else ref.exp3_q_pos(ip, np.array(seeds, dtype=np.int64), w, ETA)


@functools.lru_cache(maxsize=None)
def ref_layer(graph, mode, seeds, fanout, step, layer):
    ip, ix, ei = GRAPHS[graph]()[:3]
    return ref.sample_layer(ip, ix, ei, np.array(seeds, dtype=np.int64), fanout, SEED, step, layer, q_pos_of(graph, mode, seeds))


def bits(x):
    return x.view(torch.int16).to(torch.int32) & 0xFFFF


class Layer(Layer0):
    """Hand-allocated buffers of direct bliss_wlabor_layer calls (tests/test_gpu_labor.py's, with this sampler's scratch, its
    probability rows and its p_ij output)."""

    def __init__(self, dev, graph, cap_s, cap_k, cap_b):
        ip, ix, ei, _, q, w = GRAPHS[graph]() if isinstance(graph, str) else graph
        gd = (torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), torch.from_numpy(ei).to(dev))
        super().__init__(dev, gd, cap_s, cap_k, cap_b, num_nodes=len(ip) - 1)
        nbytes = int(self.lib.lib.bliss_wlabor_scratch_bytes(self.V, cap_s, cap_b))
        assert nbytes > 0 and nbytes % 16 == 0
        self.scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        self.rows = (torch.from_numpy(q).to(dev).bfloat16(), torch.from_numpy(w).to(dev).bfloat16())
        assert torch.equal(self.rows[0].float().nan_to_num(7.0), torch.from_numpy(q).to(dev).nan_to_num(7.0))     # (bf16 values)
        self.p = torch.full((cap_b + 8,), -7.0, dtype=torch.bfloat16, device=dev)

    def __call__(self, seeds, fanout, mode, step=0, layer=0, bump=0, ov=None, n_seeds_dev=None, set_step=True, dep=0, cap_b=None,
                 sync=True, row=None, n_seeds=None):
        _lib = self.lib
        if set_step:
            self.step.fill_(step)
        cap_b = self.cap_b if cap_b is None else cap_b
        if n_seeds is None:
            n_seeds = -1 if n_seeds_dev is not None else int(seeds.numel())
        cnt_ptr = self.counts.data_ptr()
        ws = _lib.LayerWs(cnt_ptr, self.seg_ptr.data_ptr(), 0, 0, 0, 0, 0, 0, self.kept_nid.data_ptr(), 0, 0, 0, 0, self.cap_k)
        ws.kept_map = self.kept_map.data_ptr()
        out = _lib.BlockOut(self.indptr.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), self.pos.data_ptr(), self.eid.data_ptr(),
                            self.w.data_ptr(), self.q.data_ptr(), 0, 0, 0, cap_b)
        st = torch.cuda.current_stream().cuda_stream
        row = self.rows[mode] if row is None else row
        rc = _lib.lib.bliss_wlabor_layer(C.byref(self.g), seeds.data_ptr(), n_seeds, 0 if n_seeds_dev is None else n_seeds_dev,
                                         self.cap_s, fanout, 0 if ov is None else ov.data_ptr(), SEED, self.step.data_ptr(), layer,
                                         bump, dep, mode, row.data_ptr(), float(np.float32(ETA)), float(np.float32(1.0 - ETA)),
                                         C.byref(ws), C.byref(out), self.p.data_ptr(), self.scratch.data_ptr(), st)
        assert rc == 0, rc
        rc = _lib.lib.bliss_block_transpose(self.src.data_ptr(), cnt_ptr + 16, self.cap_b, self.cap_b, self.cap_k,
                                            self.t_indptr.data_ptr(), self.t_edge.data_ptr(), self.tr_temp.data_ptr(), self.tr_bytes, st)
        assert rc == 0, rc
        if not sync:
            return None
        torch.cuda.synchronize()
        return _lib.LayerCounts.from_buffer_copy(self.counts[:10].cpu().numpy().tobytes())

    def assert_guards(self, cap_b=None):
        super().assert_guards(cap_b)
        assert bool((self.p[self.cap_b if cap_b is None else cap_b:] == -7).all()), "words behind the capacity of p_ij were overwritten"

    def assert_weights(self, want):
        """q_ij and p_ij bit for bit; edge_weights within one bf16 ulp of the restatement's, each column's summing to its kept count."""
        dev, B, S = self.dev, want["B"], want["S"]
        assert torch.equal(bits(self.q[:B]), torch.from_numpy(want["q_ij"].astype(np.int32)).to(dev)), "q_ij"
        assert torch.equal(bits(self.p[:B]), torch.from_numpy(want["p_ij"].astype(np.int32)).to(dev)), "p_ij"
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

    def assert_equals(self, c, want, err=0):
        dev = self.dev
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
        S, K, B = want["S"], want["K"], want["B"]
        assert (c.S, c.E, c.C, c.K, c.B, c.err) == (S, want["E"], K, K, B, err), (c.S, c.E, c.C, c.K, c.B, c.err, S, want["E"], K, B)
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
        self.assert_clean()                                                      # kept_map, tickets, the error word, the bitmap

    def snapshot(self, c, S):
        return torch.cat([self.counts[:6], self.indptr[:S + 1], self.pos[:c.B], self.src[:c.B], self.eid[:c.B], self.kept_nid[:c.K],
                          self.t_edge[:c.B], bits(self.w[:c.B]), bits(self.q[:c.B]), bits(self.p[:c.B])]).clone()


def _dev(a, cuda, dtype=torch.int32):
    return torch.tensor(list(a), dtype=dtype, device=cuda)


@pytest.fixture(scope="module")
def log_layer(cuda):
    return Layer(cuda, "log", 80, 2000, 4000)


@pytest.fixture(scope="module")
def col_layer(cuda):
    return Layer(cuda, "col", 16, 3000, 5000)


# ------------------------------------------------------------------------------------------------- one layer
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fanout", [-1, 1, 3, 10])
def test_lognormal_graph_both_modes(cuda, log_layer, fanout, mode):
    sl = log_graph()[3]
    seeds = _dev(sl, cuda)
    for step, layer, dep in ((0, 0, 0), (5, 2, 0), (5, 2, 1)):
        want = ref_layer("log", mode, sl, fanout, step, 0 if dep else layer)
        assert want["B"] < 4000 and want["K"] < 2000
        log_layer.assert_equals(log_layer(seeds, fanout, mode, step=step, layer=layer, dep=dep), want)
    if fanout == 3:
        assert not np.array_equal(ref_layer("log", mode, sl, 3, 5, 0)["pos"], ref_layer("log", mode, sl, 3, 5, 2)["pos"])
        assert len(set(ref_layer("log", mode, sl, 3, 0, 0)["p_e"].tolist())) > 20        # (not LABOR-0's thresholds)
    want = ref_layer("log", mode, sl[:1], fanout, 3, 1)                          # S = 1, exact capacities
    one = Layer(cuda, "log", 1, want["K"], max(want["B"], 1))
    one.assert_equals(one(_dev(sl[:1], cuda), fanout, mode, step=3, layer=1), want)


@pytest.mark.parametrize("mode", [0, 1])
def test_hand_built_columns(cuda, col_layer, mode):
    ip, ix, _, sl, q, _ = col_graph()
    want = ref_layer("col", mode, sl, F, 2, 1)
    col_layer.assert_equals(col_layer(_dev(sl, cuda), F, mode, step=2, layer=1), want)
    exact = Layer(cuda, "col", len(sl), want["K"], want["B"])                     # exact capacities
    exact.assert_equals(exact(_dev(sl, cuda), F, mode, step=2, layer=1), want)
    if mode:
        return
    c, whole = [int(x) for x in want["c"]], want["whole"]
    p = lambda s: [int(x) for x in want["p"][int(ip[s]):int(ip[s + 1])]]           # (seeds 0 .. 11 in order: frontier = CSC order)
    assert whole[WHOLE] and p(WHOLE) == [ONE] * 3 and not whole[PLUS1] and all(x < ONE for x in p(PLUS1))
    assert c[ZEROS] == ONE - 1 and p(ZEROS) == [0] * 8 and want["indptr"][ZEROS] == want["indptr"][ZEROS + 1]
    assert p(DOMINANT)[2] == ONE - 1 and c[DOMINANT] < ONE - 1                     # clamped, and the others raised to fill the fanout
    assert sum(p(DOMINANT)) > (F << 32) - 256 * 8 and p(DOMINANT)[0] > ONE // 4
    sp = p(SPECIAL)
    assert sp[0] == sp[1] == sp[2] == sp[3] == sp[6] == 0 and all(x > 0 for x in (sp[4], sp[5], sp[7])) and c[SPECIAL] == ONE - 1
    sh = p(SHIFT)
    assert sh[1] == sh[3] == 0 and sh[2] <= 255 and sh[4] == ONE - 1              # 2^-31 of the largest exponent: shifted out
    kept = set(want["pos"].tolist())
    assert not kept & {int(ip[SPECIAL]) + i for i in (0, 1, 2, 3, 6)} and not kept & {int(ip[SHIFT]) + 1, int(ip[SHIFT]) + 3}
    assert [int(d) for d in np.diff(ip)[[7, 8, 9, 10]]] == [256, 257, 2048, 2049] and all(0 < c[s] < ONE - 1 for s in (7, 8, 9, 10))


def test_a_multi_edge_is_one_variate_against_three_probabilities(cuda, col_layer):
    ip, ix, _, sl, q, _ = col_graph()
    a = int(ip[MULTI])
    p = [int(x) for x in ref_layer("col", 0, sl, F, 0, 0)["p"][a:a + 8]]
    order = sorted([(p[0], 0), (p[2], 2), (p[5], 5)])
    assert order[0][0] < order[1][0] < order[2][0] and order[0][0] >= 1
    ov = np.full(CV, 0xFFFFFFFF, dtype=np.uint32)
    ov[77] = order[1][0] - 1                                                      # below the two larger probabilities, not the smallest
    want = ref.sample_layer(ip, ix, col_graph()[2], np.array(sl), F, SEED, 0, 0, q, keys_override=ov)
    kept = want["pos"][want["dst"] == MULTI].tolist()
    assert kept == sorted(a + i for _, i in order[1:])
    col_layer.assert_equals(col_layer(_dev(sl, cuda), F, 0, ov=torch.from_numpy(ov.view(np.int32)).to(cuda)), want)
    ov[77] = order[2][0]                                                          # the strict comparison: key = p is dropped
    want = ref.sample_layer(ip, ix, col_graph()[2], np.array(sl), F, SEED, 0, 0, q, keys_override=ov)
    assert want["pos"][want["dst"] == MULTI].tolist() == [] and a + order[2][1] not in want["pos"].tolist()
    col_layer.assert_equals(col_layer(_dev(sl, cuda), F, 0, ov=torch.from_numpy(ov.view(np.int32)).to(cuda)), want)


# ------------------------------------------------------------------------------------------------- seed counts and layers
@pytest.mark.parametrize("count", [0, 1, 64])
def test_seed_count_read_on_the_device(cuda, count):
    sl = log_graph()[3]
    want = ref_layer("log", 1, sl[:count], 3, 4, 0)
    lay = Layer(cuda, "log", 64, 2000, 4000)
    n_dev = _dev([-5, count, -5], cuda)
    c = lay(_dev(sl, cuda), 3, 1, step=4, layer=0, bump=1, n_seeds_dev=n_dev.data_ptr() + 4)
    lay.assert_equals(c, want)
    assert int(lay.step.item()) == 5                                              # bumped once, by one workgroup
    if count == 0:
        assert (c.S, c.K, c.B) == (0, 0, 0)
        c = lay(_dev(sl, cuda), 3, 0, step=4, n_seeds=0)                          # n_seeds = 0 on the host side
        assert (c.S, c.K, c.B, c.err) == (0, 0, 0, 0)
        lay.assert_clean()


def test_second_layer_reads_its_seeds_from_the_first(cuda):
    ip, ix, ei, sl, q, w = log_graph()
    rows = [lambda s: ref.exp3_q_pos(ip, np.asarray(s, dtype=np.int64), w, ETA)] * 2
    lays = ref.sample_blocks(ip, ix, ei, np.array(sl[:9]), [3, 3], SEED, 4, rows)
    first = Layer(cuda, "log", 16, 200, 400)
    first.assert_equals(first(_dev(sl[:9], cuda), 3, 1, step=4, layer=0), lays[0])
    second = Layer(cuda, "log", 200, 400, 2000)
    c1 = second(first.kept_nid[:200], 3, 1, step=4, layer=1, bump=1, n_seeds_dev=first.counts.data_ptr() + 12)
    second.assert_equals(c1, lays[1])
    assert int(second.step.item()) == 5


def test_a_seed_id_out_of_range_is_an_empty_column(cuda):
    ip, ix, ei, sl, q, w = log_graph()
    sl, V = list(sl[:20]), len(ip) - 1
    bad = sl[:7] + [V + 5] + sl[7:15] + [-3] + sl[15:]
    for mode in (0, 1):
        want = ref_layer("log", mode, tuple(sl), 3, 6, 0)
        lay = Layer(cuda, "log", 32, 2000, 2000)
        c = lay(_dev(bad, cuda), 3, mode, step=6, layer=0)
        assert c.err == 2 and (c.S, c.E, c.B, c.K) == (22, want["E"], want["B"], want["K"] + 2)     # BLISS_ERR_CAP_CAND
        k = np.diff(want["indptr"])
        k = np.concatenate([k[:7], [0], k[7:15], [0], k[15:]])
        assert np.array_equal(np.diff(lay.indptr[:23].cpu().numpy()), k)
        B = want["B"]
        assert torch.equal(lay.pos[:B], torch.from_numpy(want["pos"]).to(cuda))
        assert lay.kept_nid[:22].cpu().tolist() == bad
        assert torch.equal(bits(lay.q[:B]), torch.from_numpy(want["q_ij"].astype(np.int32)).to(cuda))
        assert torch.equal(bits(lay.p[:B]), torch.from_numpy(want["p_ij"].astype(np.int32)).to(cuda))
        lay.assert_guards()
        lay.assert_clean()
        lay.assert_equals(lay(_dev(sl, cuda), 3, mode, step=6, layer=0), want)    # the following call is the restatement's


# ------------------------------------------------------------------------------------------------- state left clean
def test_edge_capacity_below_the_true_count(cuda):
    """Bounds handling: the bit is raised, nothing is written behind the capacity, and every idle scratch word is left zero."""
    sl = log_graph()[3]
    seeds = _dev(sl, cuda)
    for mode in (0, 1):
        want = ref_layer("log", mode, sl, 3, 0, 0)
        lay = Layer(cuda, "log", 64, want["K"], want["B"])
        short = want["B"] - 40
        c = lay(seeds, 3, mode, cap_b=short)
        assert c.err == 8 and c.B == short and c.S == 64
        check_index(lay.src.cpu(), lay.t_indptr.cpu(), lay.t_edge.cpu(), c.K, c.B, lay.cap_k)         # clamped, and still walkable
        lay.assert_guards(cap_b=short)                                            # (the words [short, B) of the arrays are guards too)
        lay.assert_clean()
        t = lambda x: torch.from_numpy(np.asarray(x)).to(cuda)
        ncol = int(np.searchsorted(want["indptr"], short, side="right")) - 1      # columns that fit whole are the restatement's
        nb = int(want["indptr"][ncol])
        assert torch.equal(lay.indptr[:ncol + 1], t(want["indptr"][:ncol + 1])) and bool((lay.indptr[ncol + 1:65] <= short).all())
        assert torch.equal(lay.pos[:nb], t(want["pos"][:nb])) and torch.equal(bits(lay.p[:nb]), t(want["p_ij"][:nb].astype(np.int32)))
        ix = log_graph()[1]
        assert c.K == len(np.union1d(np.array(sl), ix[lay.pos[:short].cpu().numpy()]))   # no source marked for an unwritten edge
        lay.assert_equals(lay(seeds, 3, mode), want)                              # the following call, with room: the restatement's
        short_k = Layer(cuda, "log", 64, want["K"] - 1, want["B"])
        c = short_k(seeds, 3, mode)
        assert c.err == 4 and c.K == want["K"] - 1 and c.B == want["B"]
        short_k.assert_guards()
        short_k.assert_clean()
        check_index(short_k.src.cpu(), short_k.t_indptr.cpu(), short_k.t_edge.cpu(), c.K, c.B, short_k.cap_k) # clamped, and still walkable
        short_s = Layer(cuda, "log", 63, want["K"], want["B"])
        c = short_s(seeds, 3, mode)
        assert c.err & 64 and c.S == 63
        short_s.assert_guards()
        short_s.assert_clean()
        check_index(short_s.src.cpu(), short_s.t_indptr.cpu(), short_s.t_edge.cpu(), c.K, c.B, short_s.cap_k) # clamped, and still walkable


def test_a_non_finite_exp3_weight_is_flagged_and_the_scratch_left_idle(cuda, log_layer):
    sl = log_graph()[3]
    ip = log_graph()[0]
    row = log_layer.rows[1].clone()
    row[int(ip[sl[5]]) + 1] = float("inf")
    c = log_layer(_dev(sl, cuda), 3, 1, row=row)
    assert c.err & 16 and c.S == 64                                               # BLISS_ERR_NONFINITE, through the pending-error word
    log_layer.assert_guards()
    log_layer.assert_clean()
    log_layer.assert_equals(log_layer(_dev(sl, cuda), 3, 1), ref_layer("log", 1, sl, 3, 0, 0))


@pytest.mark.parametrize("mode", [0, 1])
def test_captured_layer_replays_bit_equal(cuda, mode):
    sl = log_graph()[3]
    seeds = _dev(sl, cuda)
    lay = Layer(cuda, "log", 64, 2000, 4000)
    c = lay(seeds, 3, mode, step=7, layer=1, bump=1)
    lay.assert_equals(c, ref_layer("log", mode, sl, 3, 7, 1))
    direct = lay.snapshot(c, 64)
    lay.fill()
    lay.p.fill_(-7.0)
    lay.step.fill_(7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lay(seeds, 3, mode, layer=1, bump=1, set_step=False, sync=False)
    torch.cuda.synchronize()
    assert int(lay.step.item()) == 7                                              # (the capture executed nothing)
    snaps = []
    for _ in range(2):
        lay.step.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert int(lay.step.item()) == 8
        cr = lay.lib.LayerCounts.from_buffer_copy(lay.counts[:10].cpu().numpy().tobytes())
        snaps.append(lay.snapshot(cr, 64))
        lay.assert_guards()
        lay.assert_clean()
    assert torch.equal(snaps[0], direct) and torch.equal(snaps[1], direct)
    graph.replay()                                                                # the next draw step: another draw
    torch.cuda.synchronize()
    cr = lay.lib.LayerCounts.from_buffer_copy(lay.counts[:10].cpu().numpy().tobytes())
    lay.assert_equals(cr, ref_layer("log", mode, sl, 3, 8, 1))


def test_inclusion_frequencies_on_the_device(cuda):
    """The two columns of the CPU statistics test, 2048 draw steps counted by the device's own step counter: the rule is
    deterministic, so the counts are the restatement's integers."""
    ip, ix, q = cpu.stat_graph()
    E = len(ix)
    want_hits, ps = cpu.inclusion_counts()
    g = (ip, ix.astype(np.int32), np.arange(E, dtype=np.int32), None, q, q)
    for s, f in enumerate(cpu.STAT_F):
        lay = Layer(cuda, g, 1, 1 + E, E)
        seeds = _dev([s], cuda)
        hits = torch.zeros(E, dtype=torch.int64, device=cuda)
        one = torch.ones(E, dtype=torch.int64, device=cuda)
        for t in range(cpu.STAT_STEPS):
            lay(seeds, f, 0, layer=cpu.STAT_LAYER, bump=1, set_step=t == 0, sync=False)
            hits.index_add_(0, lay.pos[:E].long().clamp(0, E - 1), one * (torch.arange(E, device=cuda) < lay.counts[4]))
        torch.cuda.synchronize()
        assert int(lay.step.item()) == cpu.STAT_STEPS and int(lay.counts[5]) == 0
        a, b = int(ip[s]), int(ip[s + 1])
        got = hits.cpu().numpy()
        assert np.array_equal(got[a:b], want_hits[s]) and int(got.sum()) == int(want_hits[s].sum())
        cpu.check_inclusion(got[a:b], ps[s])
        lay.assert_clean()
