"""GPU suite (-m gpu): the weighted device-side neighbor draw (csrc/neighbor_w.hip) against the CPU restatement
of its rule (tests/wneighbor_ref.py).  The race keys hold an fp64 log, so they are compared within one fp32 ulp; everything behind
them is exact: the DEVICE's own keys go into the restatement and every block array, the sources, the by-source index, the counts
and q_ij must be equal, the Hajek weights within one bf16 ulp.

The graph is tests/test_gpu_neighbor.py's (6000 nodes; in-degrees 0, 1, 2, 6, 7, 8, 255, 256, 257, 1023, 1024, 1025, 4998 .. 5001, a
multi-edge, seeds that are sources of other seeds, a self-loop, permuted edge ids)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import wneighbor_ref as ref
from block_invariants import check_index
from oracle import bliss_oracle as bo
from test_gpu_neighbor import GUARD, HUB, SEED, V, Layer, graph_dev, graph_np, seeds67  # noqa: F401  (graph_dev: a fixture)
from test_wneighbor_ref import COLUMNS, check_inclusion

pytestmark = pytest.mark.gpu

FANOUTS = [1, 7, 256, 1024, 5000, -1]
FILL = 0xDEADBEEF                                                               # keys_out before a call
FILL_I32 = int(np.uint32(FILL).view(np.int32))


@functools.lru_cache(maxsize=None)
def prob_np():
    """Raw-mode probabilities by CSC position (fp32 values of bf16): positive over nine octaves, a ninth zeros, a NaN and a
    negative entry inside the hub column."""
    ip, _, _ = graph_np()
    E = int(ip[-1])
    rng = np.random.default_rng(21)
    q = ref.rbf(np.exp2(rng.uniform(-6, 3, E)).astype(np.float32))
    q[rng.permutation(E)[:E // 9]] = 0.0
    a = int(ip[HUB])
    q[a + 17], q[a + 1200] = np.nan, -2.0
    return q


@functools.lru_cache(maxsize=None)
def exp3_row_np():
    """An EXP3 row by CSC position: random positive bf16 weights in [2^-8, 2^4]."""
    ip, _, _ = graph_np()
    return ref.rbf(np.exp2(np.random.default_rng(22).uniform(-8, 4, int(ip[-1]))).astype(np.float32))


def bf16_dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).bfloat16().contiguous()


class WLayer(Layer):
    """Hand-allocated buffers of direct bliss_wneighbor_layer calls; every output array is followed by guard words."""

    def __init__(self, dev, graph_dev, cap_s, cap_k, cap_b, num_nodes=V):
        super().__init__(dev, graph_dev, cap_s, cap_k, cap_b)
        self.E = int(self.ix.numel())
        self.g.num_nodes = num_nodes
        self.kept_map = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(self.lib.lib.bliss_wneighbor_scratch_bytes(num_nodes, cap_s, self.E)) // 4, dtype=torch.int32,
                                   device=dev)
        self.keys_out = torch.zeros(self.E + GUARD, dtype=torch.int32, device=dev)
        self.num_nodes = num_nodes

    def __call__(self, seeds, fanout, prob, mode=0, eta=0.4, step=0, layer=0, bump=0, ov=None, n_seeds_dev=None, record=0,
                 set_step=True, keys_out=True, transpose=True, sync=True):
        _lib = self.lib
        if set_step:
            self.step.fill_(step)
        if keys_out:
            self.keys_out.fill_(FILL_I32)
        n_seeds = -1 if n_seeds_dev is not None else int(seeds.numel())
        cnt_ptr = self.counts.data_ptr() + 40 * record
        ws = _lib.LayerWs(cnt_ptr, self.seg_ptr.data_ptr(), 0, 0, 0, 0, 0, 0, self.kept_nid.data_ptr(), 0, 0, 0, 0, self.cap_k)
        ws.kept_map = self.kept_map.data_ptr()
        out = _lib.BlockOut(self.indptr.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), self.pos.data_ptr(), self.eid.data_ptr(),
                            self.w.data_ptr(), self.q.data_ptr(), 0, 0, 0, self.cap_b)
        st = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib.bliss_wneighbor_layer(C.byref(self.g), seeds.data_ptr(), n_seeds, 0 if n_seeds_dev is None else n_seeds_dev,
                                            self.cap_s, fanout, 0 if ov is None else ov.data_ptr(), SEED, self.step.data_ptr(), layer,
                                            bump, mode, prob.data_ptr(), float(np.float32(eta)), float(np.float32(1.0 - eta)),
                                            self.keys_out.data_ptr() if keys_out else 0, C.byref(ws), C.byref(out),
                                            self.scratch.data_ptr(), st)
        assert rc == 0, rc
        if transpose:
            rc = _lib.lib.bliss_block_transpose(self.src.data_ptr(), cnt_ptr + 16, self.cap_b, self.cap_b, self.cap_k,
                                                self.t_indptr.data_ptr(), self.t_edge.data_ptr(), self.tr_temp.data_ptr(), self.tr_bytes, st)
            assert rc == 0, rc
        if not sync:
            return None
        torch.cuda.synchronize()
        return _lib.LayerCounts.from_buffer_copy(self.counts[10 * record:10 * record + 10].cpu().numpy().tobytes())

    def dev_keys(self):
        assert bool((self.keys_out[self.E:] == FILL_I32).all()), "guard words after keys_out"
        return self.keys_out[:self.E].cpu().numpy().view(np.uint32).copy()

    def assert_clean(self):
        words = -(-(-(-self.num_nodes // 32)) // 1024) * 1024
        assert bool((self.kept_map == -1).all()), "kept_map is not clean"
        assert int(self.scratch[:16 + words].abs().sum()) == 0, "tickets / bitmap are not zero"

    def got(self, c):
        n = lambda t: t.cpu().numpy()
        S, K, B = c.S, c.K, c.B
        return dict(S=S, E=c.E, K=K, B=B, indptr=n(self.indptr[:S + 1]), pos=n(self.pos[:B]), dst=n(self.dst[:B]), eid=n(self.eid[:B]),
                    src=n(self.src[:B]), kept_nid=n(self.kept_nid[:K]), t_indptr=n(self.t_indptr[:K + 1]), t_edge=n(self.t_edge[:B]),
                    q_ij=n(self.q[:B].view(torch.int16)).view(np.uint16), weights=n(self.w[:B].float()))

    def assert_equals(self, c, want):
        assert (c.C, c.err) == (c.K, 0), (c.C, c.K, c.err)
        ref.compare(self.got(c), want)
        self.assert_guards()
        self.assert_clean()


def want_layer(seeds, fanout, q_pos, keys, step=0, layer=0):
    ip, ix, ei = graph_np()
    return ref.sample_layer(ip, ix, ei, np.array(seeds), fanout, SEED, step, layer, q_pos, keys_override=keys)


def assert_keys(dev, seeds, fanout, q_pos, step, layer):
    """Device keys within one fp32 ulp of the restatement's, +inf exactly; nothing stored for whole columns."""
    ip, _, _ = graph_np()
    want, mask = ref.frontier_keys(ip, np.array(seeds), fanout, SEED, step, layer, q_pos)
    assert bool((dev[~mask] == FILL).all()), "a key was stored outside the non-whole seed columns"
    inf = want[mask] == ref.INF_BITS
    assert np.array_equal(dev[mask] == ref.INF_BITS, inf)
    diff = np.abs(dev[mask].astype(np.int64) - want[mask].astype(np.int64))
    print("fanout %d: %d keys, %d +inf, %d one ulp off" % (fanout, int(mask.sum()), int(inf.sum()), int((diff == 1).sum())))
    assert int(diff.max(initial=0)) <= 1


@pytest.fixture(scope="module")
def layer67(cuda, graph_dev):
    return WLayer(cuda, graph_dev, 80, V, int(graph_dev[1].numel()))


@pytest.mark.parametrize("fanout", FANOUTS)
def test_raw_mode_keys_and_the_exact_path(cuda, graph_dev, layer67, fanout):
    """Raw mode with zeros, a NaN and a negative entry in ``prob``."""
    q_pos = prob_np()
    prob = bf16_dev(q_pos, cuda)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    for step, layer in ((0, 0), (5, 2)):
        c = layer67(seeds, fanout, prob, step=step, layer=layer)
        keys = layer67.dev_keys()
        assert_keys(keys, seeds67(), fanout, q_pos, step, layer)
        layer67.assert_equals(c, want_layer(seeds67(), fanout, q_pos, keys, step, layer))
    one = WLayer(cuda, graph_dev, 1, 5001, 5000)                                  # S = 1: the hub alone, exact capacities
    c = one(torch.tensor([HUB], dtype=torch.int32, device=cuda), fanout, prob, step=3, layer=1)
    one.assert_equals(c, want_layer((HUB,), fanout, q_pos, one.dev_keys(), 3, 1))
    assert c.B == (5000 if fanout < 0 else min(fanout, 5000))


@pytest.mark.parametrize("fanout", [7, 256])
def test_planted_keys(cuda, graph_dev, layer67, fanout):
    ip, _, _ = graph_np()
    E = int(ip[-1])
    q_pos = prob_np()
    prob = bf16_dev(q_pos, cuda)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    one = np.float32(1.0).view(np.uint32)
    planted = [np.full(E, one, dtype=np.uint32),                                  # every key equal: the lowest positions
               np.where(np.arange(E) % 2 == 0, one + np.uint32(1), one).astype(np.uint32)]   # two values one ulp apart, alternating
    few = np.full(E, ref.INF_BITS, dtype=np.uint32)                               # +inf everywhere but fanout - 1 positions a column
    rng = np.random.default_rng(23)
    for nid in seeds67():
        a, b = int(ip[nid]), int(ip[nid + 1])
        if b - a > fanout:
            few[a + rng.permutation(b - a)[:fanout - 1]] = rng.integers(1, 2 ** 30, fanout - 1).astype(np.uint32)
    planted.append(few)
    for ov in planted:
        c = layer67(seeds, fanout, prob, ov=torch.from_numpy(ov.view(np.int32)).to(cuda))
        want = want_layer(seeds67(), fanout, q_pos, ov)
        layer67.assert_equals(c, want)
        keys = layer67.dev_keys()                                                 # the planted keys come back through keys_out
        _, mask = ref.frontier_keys(ip, np.array(seeds67()), fanout, SEED, 0, 0, q_pos)
        assert np.array_equal(keys[mask], ov[mask]) and bool((keys[~mask] == FILL).all())
    s = seeds67().index(HUB)                                                      # the last case: fanout - 1 finite keys, one filler
    a = int(ip[HUB])
    kept = want["pos"][want["indptr"][s]:want["indptr"][s + 1]]
    fin = np.nonzero(few[a:a + 5000] != ref.INF_BITS)[0] + a
    assert len(kept) == fanout and set(fin.tolist()) <= set(kept.tolist())
    filler = (set(kept.tolist()) - set(fin.tolist())).pop()
    assert filler == min(p for p in range(a, a + 5000) if few[p] == ref.INF_BITS)


@pytest.mark.parametrize("eta", [0.1, 0.4])
def test_exp3_mode_q_is_the_oracles_on_every_frontier_edge(cuda, graph_dev, layer67, eta):
    ip, ix, ei = graph_np()
    w_pos = exp3_row_np()
    row = bf16_dev(w_pos, cuda)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    c = layer67(seeds, -1, row, mode=1, eta=eta)
    g = bo.CSC(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(ei))
    fr = bo.expand_frontier(g, torch.tensor(seeds67()))
    w_eid = torch.empty(int(ip[-1]), dtype=torch.bfloat16)
    w_eid[torch.from_numpy(ei).long()] = torch.from_numpy(w_pos).bfloat16()
    want_q, _ = bo.exp3_edge_prob(g, fr, w_eid, eta)
    assert c.err == 0 and c.B == c.E == fr.pos.numel()
    assert torch.equal(layer67.pos[:c.B].cpu().long(), fr.pos)                    # fanout -1: the block is the frontier
    assert torch.equal(layer67.q[:c.B].cpu().view(torch.int16), want_q.view(torch.int16))
    assert bool((layer67.w[:c.B] == 1).all())
    # the same probabilities drive the draw: the restatement's EXP3 q (equal to the oracle's, tests/test_wneighbor_ref.py)
    q_pos = ref.exp3_q_pos(ip, np.array(seeds67()), w_pos, eta)
    for fanout in (7, 1024):
        c = layer67(seeds, fanout, row, mode=1, eta=eta, step=2, layer=1)
        keys = layer67.dev_keys()
        assert_keys(keys, seeds67(), fanout, q_pos, 2, 1)
        layer67.assert_equals(c, want_layer(seeds67(), fanout, q_pos, keys, 2, 1))


def test_capacity_overflows_raise_their_bit_and_leave_the_scratch_idle(cuda, graph_dev):
    q_pos = prob_np()
    prob = bf16_dev(q_pos, cuda)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    full = WLayer(cuda, graph_dev, 67, V, 67 * 7)
    c = full(seeds, 7, prob)
    keys = full.dev_keys()
    want = want_layer(seeds67(), 7, q_pos, keys)
    full.assert_equals(c, want)
    ov = torch.from_numpy(keys.view(np.int32)).to(cuda)
    E = int(graph_dev[1].numel())
    shared = torch.zeros(int(full.lib.lib.bliss_wneighbor_scratch_bytes(V, 67, E)) // 4, dtype=torch.int32, device=cuda)
    for cap_s, cap_k, cap_b, bit in ((67, want["K"] - 1, want["B"], 4), (67, want["K"], want["B"] - 1, 8), (66, want["K"], want["B"], 64)):
        short = WLayer(cuda, graph_dev, cap_s, cap_k, cap_b)
        short.scratch = shared
        c = short(seeds, 7, prob, ov=ov)
        assert c.err & bit, (c.err, bit)
        assert c.K <= cap_k and c.B <= cap_b and c.S <= cap_s
        short.assert_guards()
        short.assert_clean()
        check_index(short.src.cpu(), short.t_indptr.cpu(), short.t_edge.cpu(), c.K, c.B, cap_k)       # clamped, and still walkable
        # the same scratch and kept_map serve a call with enough room: bitmap, tickets and kept_map were left idle
        roomy = WLayer(cuda, graph_dev, 67, want["K"], want["B"])                 # (the exact capacities hold everything)
        roomy.scratch, roomy.kept_map = shared, short.kept_map
        roomy.assert_equals(roomy(seeds, 7, prob, ov=ov), want)


def test_a_seed_id_out_of_range_is_an_empty_column(cuda, graph_dev):
    q_pos = prob_np()
    prob = bf16_dev(q_pos, cuda)
    ids = list(seeds67()[:20])
    lay = WLayer(cuda, graph_dev, 32, V, 32 * 7)
    for bad in (V, -1, 2 ** 31 - 1):
        mixed = ids[:9] + [bad] + ids[9:]
        c = lay(torch.tensor(mixed, dtype=torch.int32, device=cuda), 7, prob, step=1)
        assert c.err == 2 and c.S == 21                                           # BLISS_ERR_CAP_CAND, as the uniform draw flags it
        lay.assert_guards()
        lay.assert_clean()
        row = lay.indptr[:22].cpu().numpy()
        assert row[10] == row[9]                                                  # nothing was drawn for it (column 9)
    c = lay(torch.tensor(ids, dtype=torch.int32, device=cuda), 7, prob, step=1)   # and the next call is whole
    lay.assert_equals(c, want_layer(tuple(ids), 7, q_pos, lay.dev_keys(), 1, 0))


def test_replay_and_the_step_bump(cuda, graph_dev, layer67):
    q_pos = prob_np()
    prob = bf16_dev(q_pos, cuda)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    snaps = []
    for _ in range(2):
        c = layer67(seeds, 7, prob, step=9, layer=1, bump=0)
        assert int(layer67.step.item()) == 9                                      # bumped by the last-sampled layer only
        g = layer67.got(c)
        g["keys"] = layer67.dev_keys()
        snaps.append(g)
    for name in snaps[0]:
        assert np.array_equal(np.asarray(snaps[0][name]), np.asarray(snaps[1][name])), name
    c = layer67(seeds, 7, prob, step=9, layer=1, bump=1)
    assert int(layer67.step.item()) == 10                                         # once per call, by one workgroup
    assert np.array_equal(layer67.got(c)["pos"], snaps[0]["pos"])                 # (the call itself drew with step 9)
    c = layer67(seeds, 7, prob, layer=1, bump=1, set_step=False)
    assert int(layer67.step.item()) == 11
    layer67.assert_equals(c, want_layer(seeds67(), 7, q_pos, layer67.dev_keys(), 10, 1))
    assert not np.array_equal(layer67.got(c)["pos"], snaps[0]["pos"])


@pytest.mark.parametrize("which", ["a", "b"])
def test_inclusion_frequencies_on_the_device(cuda, which):
    """The issue's two columns (positions 0..7, q = 1..8, fanout 3; positions 100..107, fanout 2) over draw steps 0..2047 counted by
    the device's own step counter: within 5 sigma of the exact inclusion probabilities of successive sampling."""
    a, q, f = COLUMNS[which]
    ip = torch.tensor([0, 8, 100, 108] + [108] * 6, dtype=torch.int64, device=cuda)          # nodes 0 and 2 hold the two columns
    ix = (torch.arange(108, dtype=torch.int32, device=cuda) % 6) + 3
    lay = WLayer(cuda, (ip, ix, torch.arange(108, dtype=torch.int32, device=cuda)), 1, 4, 3, num_nodes=9)
    q_pos = np.ones(108, dtype=np.float32)
    q_pos[a:a + 8] = q
    prob = bf16_dev(q_pos, cuda)
    seeds = torch.tensor([0 if which == "a" else 2], dtype=torch.int32, device=cuda)
    hits = torch.zeros(108, dtype=torch.int64, device=cuda)
    errs = torch.zeros(1, dtype=torch.int32, device=cuda)
    one = torch.ones(f, dtype=torch.int64, device=cuda)
    for t in range(2048):
        lay(seeds, f, prob, layer=1, bump=1, set_step=t == 0, keys_out=False, transpose=False, sync=False)
        hits.index_add_(0, lay.pos[:f].long(), one)
        errs |= lay.counts[5:6] | (lay.counts[4:5] != f).int()
    torch.cuda.synchronize()
    assert int(lay.step.item()) == 2048 and int(errs.item()) == 0
    hits = hits.cpu().numpy()
    assert int(hits[:a].sum()) == 0 and int(hits[a + 8:].sum()) == 0
    check_inclusion(hits[a:a + 8], which, 2048)
