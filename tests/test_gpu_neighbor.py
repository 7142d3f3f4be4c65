"""GPU suite (-m gpu): the device-side neighbor sampler (csrc/neighbor.hip) against the CPU restatement of its rule
(tests/neighbor_ref.py), array for array with torch.equal -- the rule is integers only, so there is no tolerance anywhere.

The graph is hand-built (6000 nodes): its first nodes have in-degrees 0, 1, 2, 6, 7, 8, 255, 256, 257, 1023, 1024, 1025, 4998, 4999,
5000 and 5001 (every fanout of the cases below has columns of degree fanout - 1, fanout and fanout + 1, and the select kernel's
256-edge chunks are met from both sides), the other nodes 0..12; edge ids are a permutation; one column holds the same source
twice, and seeds are sources of other seeds."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import neighbor_ref as ref
from block_invariants import check_index
from test_neighbor_ref import check_inclusion, inclusion_counts

pytestmark = pytest.mark.gpu

V = 6000
DEG = [0, 1, 2, 6, 7, 8, 255, 256, 257, 1023, 1024, 1025, 4998, 4999, 5000, 5001]
HUB = 14                                                                       # the column of degree 5000
SEED = 1234
GUARD = 8


@functools.lru_cache(maxsize=None)
def graph_np():
    rng = np.random.default_rng(11)
    deg = np.concatenate([np.array(DEG), rng.integers(0, 13, V - len(DEG))])
    indptr = np.zeros(V + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.integers(0, V, int(indptr[-1]))
    indices[indptr[2]:indptr[3]] = 4000                                         # a multi-edge: both in-edges of node 2 from 4000
    indices[indptr[5]] = HUB                                                    # seeds that are sources of other seeds
    indices[indptr[HUB] + 3] = 5
    indices[indptr[HUB] + 4] = HUB                                              # and a self-loop
    eid = rng.permutation(int(indptr[-1]))
    return indptr, indices.astype(np.int32), eid.astype(np.int32)


@functools.lru_cache(maxsize=None)
def seeds67():
    rest = np.random.default_rng(12).permutation(np.arange(len(DEG), V))[:67 - len(DEG)]
    return tuple(np.random.default_rng(13).permutation(np.concatenate([np.arange(len(DEG)), rest])).tolist())


@functools.lru_cache(maxsize=None)
def ref_layer(seeds, fanout, step, layer):
    ip, ix, ei = graph_np()
    return ref.sample_layer(ip, ix, ei, np.array(seeds), fanout, SEED, step, layer)


@pytest.fixture(scope="module")
def graph_dev(cuda):
    ip, ix, ei = graph_np()
    return torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda), torch.from_numpy(ei).to(cuda)


class Layer:
    """Hand-allocated buffers of direct bliss_neighbor_layer calls; every output array is followed by guard words."""

    def __init__(self, dev, graph_dev, cap_s, cap_k, cap_b):
        from bliss_gnn_amd import _lib
        self.lib, self.dev = _lib, dev
        self.ip, self.ix, self.ei = graph_dev
        self.cap_s, self.cap_k, self.cap_b = cap_s, cap_k, cap_b
        self.g = _lib.Graph(self.ip.data_ptr(), self.ix.data_ptr(), self.ei.data_ptr(), V, int(self.ix.numel()))
        i32 = lambda n: torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(20, dtype=torch.int32, device=dev)
        self.seg_ptr, self.indptr = i32(cap_s + 1), i32(cap_s + 1)
        self.src, self.dst, self.pos, self.eid = i32(cap_b), i32(cap_b), i32(cap_b), i32(cap_b)
        self.w = torch.full((cap_b + GUARD,), -7.0, dtype=torch.bfloat16, device=dev)
        self.q = torch.full((cap_b + GUARD,), -7.0, dtype=torch.bfloat16, device=dev)
        self.kept_nid = i32(cap_k)
        self.t_indptr, self.t_edge = i32(cap_k + 1), i32(max(cap_b, 1))
        self.kept_map = torch.full((V,), -1, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(_lib.lib.bliss_neighbor_scratch_bytes(V, cap_s)) // 4, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.tr_bytes = int(_lib.lib.bliss_block_transpose_temp_bytes(cap_b, cap_k))
        self.tr_temp = torch.empty(max(self.tr_bytes, 1), dtype=torch.uint8, device=dev)

    def __call__(self, seeds, fanout, step=0, layer=0, bump=0, ov=None, n_seeds_dev=None, record=0, set_step=True):
        _lib = self.lib
        if set_step:
            self.step.fill_(step)
        n_seeds = -1 if n_seeds_dev is not None else int(seeds.numel())
        cnt_ptr = self.counts.data_ptr() + 40 * record
        ws = _lib.LayerWs(cnt_ptr, self.seg_ptr.data_ptr(), 0, 0, 0, 0, 0, 0, self.kept_nid.data_ptr(), 0, 0, 0, 0, self.cap_k)
        ws.kept_map = self.kept_map.data_ptr()
        out = _lib.BlockOut(self.indptr.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), self.pos.data_ptr(), self.eid.data_ptr(),
                            self.w.data_ptr(), self.q.data_ptr(), 0, 0, 0, self.cap_b)
        st = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib.bliss_neighbor_layer(C.byref(self.g), seeds.data_ptr(), n_seeds, 0 if n_seeds_dev is None else n_seeds_dev,
                                           self.cap_s, fanout, 0 if ov is None else ov.data_ptr(), SEED, self.step.data_ptr(), layer,
                                           bump, C.byref(ws), C.byref(out), self.scratch.data_ptr(), st)
        assert rc == 0, rc
        rc = _lib.lib.bliss_block_transpose(self.src.data_ptr(), cnt_ptr + 16, self.cap_b, self.cap_b, self.cap_k,
                                            self.t_indptr.data_ptr(), self.t_edge.data_ptr(), self.tr_temp.data_ptr(), self.tr_bytes, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return _lib.LayerCounts.from_buffer_copy(self.counts[10 * record:10 * record + 10].cpu().numpy().tobytes())

    def assert_guards(self):
        for name, n in (("seg_ptr", self.cap_s + 1), ("indptr", self.cap_s + 1), ("src", self.cap_b), ("dst", self.cap_b),
                        ("pos", self.cap_b), ("eid", self.cap_b), ("kept_nid", self.cap_k), ("w", self.cap_b), ("q", self.cap_b)):
            assert bool((getattr(self, name)[n:] == -7).all()), "guard words after %s were overwritten" % name

    def assert_clean(self):
        """What a replay relies on: kept_map all -1, tickets and bitmap all zero."""
        words = -(-(-(-V // 32)) // 1024) * 1024
        assert bool((self.kept_map == -1).all()), "kept_map is not clean"
        assert int(self.scratch[:16 + words].abs().sum()) == 0, "tickets / bitmap are not zero"

    def assert_equals(self, c, want):
        dev = self.dev
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
        S, K, B = want["S"], want["K"], want["B"]
        assert (c.S, c.E, c.C, c.K, c.B, c.err) == (S, want["E"], K, K, B, 0), (c.S, c.E, c.C, c.K, c.B, c.err, S, want["E"], K, B)
        assert torch.equal(self.indptr[:S + 1], t(want["indptr"]))
        for name in ("pos", "dst", "eid", "src"):
            assert torch.equal(getattr(self, name)[:B], t(want[name])), name
        assert torch.equal(self.kept_nid[:K], t(want["kept_nid"]))
        assert torch.equal(self.t_indptr[:K + 1], t(want["t_indptr"])) and torch.equal(self.t_edge[:B], t(want["t_edge"]))
        assert bool((self.w[:B] == 1).all()) and bool((self.q[:B] == 1).all())
        self.assert_guards()
        self.assert_clean()


@pytest.fixture(scope="module")
def layer67(cuda, graph_dev):
    return Layer(cuda, graph_dev, 80, V, int(graph_dev[1].numel()))


@pytest.mark.parametrize("fanout", [1, 7, 256, 4999, 5000, -1])
def test_one_layer_of_67_seeds_and_of_one(cuda, graph_dev, layer67, fanout):
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    for step, layer in ((0, 0), (5, 2)):
        c = layer67(seeds, fanout, step=step, layer=layer)
        layer67.assert_equals(c, ref_layer(seeds67(), fanout, step, layer))
    c = layer67(seeds, fanout, step=0, layer=0)                                  # again on the same scratch: nothing was left behind
    layer67.assert_equals(c, ref_layer(seeds67(), fanout, 0, 0))
    one = Layer(cuda, graph_dev, 1, 5001, 5000)                                  # S = 1: the hub alone, exact capacities
    c = one(torch.tensor([HUB], dtype=torch.int32, device=cuda), fanout, step=3, layer=1)
    one.assert_equals(c, ref_layer((HUB,), fanout, 3, 1))
    assert c.B == (5000 if fanout < 0 else min(fanout, 5000))


def test_second_layer_reads_its_seed_count_from_the_device(cuda, graph_dev):
    ip, ix, ei = graph_np()
    lays = ref.sample_blocks(ip, ix, ei, np.array(seeds67()[:9]), [7, 3], SEED, 4)
    first = Layer(cuda, graph_dev, 16, 200, 9 * 7)
    c0 = first(torch.tensor(seeds67()[:9], dtype=torch.int32, device=cuda), 7, step=4, layer=0)
    first.assert_equals(c0, lays[0])
    second = Layer(cuda, graph_dev, 200, 200 * 4, 200 * 3)
    # the seeds are the first layer's kept nodes (capacity-padded), their number is the K of its counts record
    c1 = second(first.kept_nid[:200], 3, step=4, layer=1, bump=1, n_seeds_dev=first.counts.data_ptr() + 12)
    second.assert_equals(c1, lays[1])
    assert int(second.step.item()) == 5                                           # bumped once, by one workgroup


def test_planted_ties(cuda, graph_dev, layer67):
    ip, ix, ei = graph_np()
    E = int(ip[-1])
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    # every key equal: the lowest positions of every column
    ov = np.full(E, 0x80000001, dtype=np.uint32)
    c = layer67(seeds, 256, ov=torch.from_numpy(ov.view(np.int32)).to(cuda))
    want = ref.sample_layer(ip, ix, ei, np.array(seeds67()), 256, SEED, 0, 0, keys_override=ov)
    layer67.assert_equals(c, want)
    s = seeds67().index(11)                                                       # the column of degree 1025
    assert want["pos"][want["indptr"][s]:want["indptr"][s + 1]].tolist() == list(range(int(ip[11]), int(ip[11]) + 256))
    # three equal keys at positions 10, 300 and 1500 of the hub straddle the threshold: 254 keys below, two of the three kept
    a = int(ip[HUB])
    ov = (np.random.default_rng(14).permutation(E).astype(np.uint32) * np.uint32(2) + np.uint32(1))        # odd, distinct
    tie = a + np.array([10, 300, 1500])
    others = np.sort(np.delete(ov[a:a + 5000], tie - a))
    T = others[253] + np.uint32(1)                                                # even: above 254 of the others, below the rest
    assert others[253] < T < others[254]
    ov[tie] = T
    c = layer67(seeds, 256, ov=torch.from_numpy(ov.view(np.int32)).to(cuda))
    want = ref.sample_layer(ip, ix, ei, np.array(seeds67()), 256, SEED, 0, 0, keys_override=ov)
    layer67.assert_equals(c, want)
    s = seeds67().index(HUB)
    kept = set(layer67.pos[want["indptr"][s]:want["indptr"][s + 1]].cpu().tolist())
    assert a + 10 in kept and a + 300 in kept and a + 1500 not in kept


def test_capacity_overflows_raise_their_bit_and_write_nothing_beyond(cuda, graph_dev):
    want = ref_layer(seeds67(), 7, 0, 0)
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    short_k = Layer(cuda, graph_dev, 67, want["K"] - 1, want["B"])
    c = short_k(seeds, 7)
    assert c.err == 4 and c.K == want["K"] - 1 and c.B == want["B"]
    short_k.assert_guards()
    short_k.assert_clean()
    check_index(short_k.src.cpu(), short_k.t_indptr.cpu(), short_k.t_edge.cpu(), c.K, c.B, short_k.cap_k)     # clamped, and still walkable
    short_b = Layer(cuda, graph_dev, 67, want["K"], want["B"] - 1)
    c = short_b(seeds, 7)
    assert c.err == 8 and c.B == want["B"] - 1
    short_b.assert_guards()
    short_b.assert_clean()
    check_index(short_b.src.cpu(), short_b.t_indptr.cpu(), short_b.t_edge.cpu(), c.K, c.B, short_b.cap_k)     # clamped, and still walkable
    exact = Layer(cuda, graph_dev, 67, want["K"], want["B"])                      # the exact capacities hold everything
    exact.assert_equals(exact(seeds, 7), want)
    short_s = Layer(cuda, graph_dev, 66, want["K"], want["B"])
    c = short_s(seeds, 7)
    assert c.err & 64 and c.S == 66
    short_s.assert_guards()
    short_s.assert_clean()
    check_index(short_s.src.cpu(), short_s.t_indptr.cpu(), short_s.t_edge.cpu(), c.K, c.B, short_s.cap_k)     # clamped, and still walkable


def test_inclusion_frequencies_on_the_device(cuda):
    """One column of degree 8 at positions 0..7, fanout 3, 2048 draw steps counted by the device's own step counter: the rule is
    deterministic, so the counts are the restatement's, and those are within 5 sigma of uniform."""
    ip = torch.tensor([0, 8] + [8] * 8, dtype=torch.int64, device=cuda)
    ix = torch.arange(1, 9, dtype=torch.int32, device=cuda)
    lay = Layer(cuda, (ip, ix, torch.arange(8, dtype=torch.int32, device=cuda)), 1, 4, 3)
    lay.g.num_nodes = 9
    lay.kept_map = torch.full((9,), -1, dtype=torch.int32, device=cuda)
    lay.scratch = torch.zeros(int(lay.lib.lib.bliss_neighbor_scratch_bytes(9, 1)) // 4, dtype=torch.int32, device=cuda)
    seeds = torch.zeros(1, dtype=torch.int32, device=cuda)
    hits = torch.zeros(8, dtype=torch.int64, device=cuda)
    one = torch.ones(3, dtype=torch.int64, device=cuda)
    for t in range(2048):
        c = lay(seeds, 3, layer=1, bump=1, set_step=t == 0)
        assert c.err == 0 and c.B == 3
        hits.index_add_(0, lay.pos[:3].long(), one)
    assert int(lay.step.item()) == 2048
    hits = hits.cpu().numpy()
    assert np.array_equal(hits, inclusion_counts())
    check_inclusion(hits)


# ------------------------------------------------------------------------------------------------- through the sampler
def _graph(graph_dev):
    import bliss_gnn_amd as bg
    ip, ix, ei = graph_dev
    return bg.Graph(ip, ix, ei)


def _assert_blocks(blocks, lays, cuda):
    import bliss_gnn_amd as bg
    t = lambda a: torch.from_numpy(np.asarray(a)).to(cuda)
    for blk, want in zip(reversed(blocks), lays):                                 # sampling order
        c = blk._counts
        assert (c.S, c.E, c.K, c.B, c.err) == (want["S"], want["E"], want["K"], want["B"], 0)
        assert (blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()) == (want["S"], want["K"], want["B"])
        assert torch.equal(blk.indptr, t(want["indptr"])) and torch.equal(blk.src, t(want["src"])) and torch.equal(blk.dst, t(want["dst"]))
        assert torch.equal(blk.pos, t(want["pos"])) and torch.equal(blk.edata[bg.EID], t(want["eid"]))
        assert torch.equal(blk.srcdata[bg.NID], t(want["kept_nid"]))
        ti, te = blk.transposed()
        assert torch.equal(ti, t(want["t_indptr"])) and torch.equal(te[:want["B"]], t(want["t_edge"]))
        assert bool((blk.edata["edge_weights"] == 1).all()) and blk.edata["edge_weights"].dtype == torch.bfloat16


def test_sampler_draws_the_restatements_blocks_and_keeps_its_state_on_the_device(cuda, graph_dev):
    from bliss_gnn_amd import fit
    g = _graph(graph_dev)
    ip, ix, ei = graph_np()
    s = fit.NeighborSampler([3, 7], seed=SEED, draw="device")                     # input-most first: sampled 7, then 3
    seeds = torch.tensor(seeds67(), dtype=torch.int32, device=cuda)
    torch.manual_seed(77)
    rng_cpu, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    for step in range(3):
        assert s.draw_step() == step                                              # one per call
        _, _, blocks = s.sample_blocks(g, seeds)
        _assert_blocks(blocks, ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [7, 3], SEED, step), cuda)
    assert torch.equal(torch.get_rng_state(), rng_cpu) and torch.equal(torch.cuda.get_rng_state(), rng_gpu)
    # the same state draws the same blocks
    again = []
    for _ in range(2):
        s.reset_draw(SEED, step=41)
        again.append(s.sample_blocks(g, seeds)[2])
        assert s.draw_step() == 42
    for b1, b2 in zip(*again):
        assert torch.equal(b1.pos, b2.pos) and torch.equal(b1.src, b2.src) and torch.equal(b1.srcdata["_ID"], b2.srcdata["_ID"])
    _assert_blocks(again[0], ref.sample_blocks(ip, ix, ei, np.array(seeds67()), [7, 3], SEED, 41), cuda)
    # replay hygiene of the engine's own scratch
    eng = s._engine
    words = -(-(-(-V // 32)) // 1024) * 1024
    assert int(eng._nb_scr[:16 + words].abs().sum()) == 0
    for st in eng._sets.values():
        assert bool((st["kept_map"] == -1).all())


@pytest.mark.parametrize("fanout", [5001, -1])
def test_fanout_at_least_the_largest_degree_is_the_full_neighbourhood(cuda, graph_dev, fanout):
    """The blocks of MultiLayerFullNeighborSampler up to the order of the sources: per destination, the same (source, edge id) set."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    g = _graph(graph_dev)
    seeds = torch.tensor(seeds67()[:20], dtype=torch.int32, device=cuda)
    _, _, mine = fit.NeighborSampler([fanout, fanout], draw="device").sample_blocks(g, seeds)
    _, _, full = fit.MultiLayerFullNeighborSampler(2).sample_blocks(g, seeds)

    def columns(b):
        nid = b.srcdata[bg.NID].cpu().numpy()
        rows = np.stack([nid[b.dst.cpu().numpy()], nid[b.src.cpu().numpy()], b.edata[bg.EID].cpu().numpy()], 1)
        return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]

    for a, b in zip(mine, full):
        assert a.num_edges() == b.num_edges() and a.num_src_nodes() == b.num_src_nodes()
        assert np.array_equal(np.sort(a.srcdata[bg.NID].cpu().numpy()), np.sort(b.srcdata[bg.NID].cpu().numpy()))
        assert np.array_equal(columns(a), columns(b))
