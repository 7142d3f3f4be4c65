"""GPU suite (-m gpu): bliss_sage_infer_spmm alone (csrc/sage_infer.hip).

Both reductions must equal, bit for bit, what the block kernels give on graph.full_neighbor_block of every batch with h gathered
through srcdata["_ID"]: 'mean' against bliss_spmm_fwd (weighted_aggregate(blk, x, None, mean=True)), 'max' against
bliss_spmm_max_fwd (max_aggregate(blk, x, None)).  'mean' also lies within bounds.SPMM_K["bf16"] = (1, 0.25) of the float64 value
(one rounding at the store; an fp32 sum of at most SPMM_MAX_ROW terms -- the longest row has 1569); 'max' equals the float64
segment maximum exactly.

Graphs: chung_lu_csc(2500, 600000, seed=9) at batch sizes 128 / 37 (every batch at 16-edge chunks), 300 (chunks of 32 and 16 in
one run) and 1250 (64) -- asserted from indptr -- and the 60-node multigraph of gcn_infer_ref.small_multigraph at 1 / 7 / 60 / 100.
dim 1, 3, 41 (one feature per lane), 4, 64, 260 (8-byte accesses; 260 is a second trip of the column loop).  Ranges: everything,
a middle range of whole batches, the short last batch alone, an empty range; a feature row stride above dim; a slice of h that
breaks the 8-byte alignment; NaN-filled outputs with guard rows and columns; two launches."""
import numpy as np
import pytest
import torch

import gcn_infer_ref as gref
import sage_infer_ref as ref
from bounds import SPMM_K, SPMM_MAX_ROW, assert_within, spmm_terms

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CASES = [("synthetic", 128), ("synthetic", 300), ("synthetic", 1250), ("synthetic", 37), ("small", 1), ("small", 7), ("small", 60), ("small", 100)]
CHUNKS = {128: {16}, 300: {16, 32}, 1250: {64}, 37: {16}}
_cache = {}


def _graph(name, cuda):
    if name not in _cache:
        import bliss_gnn_amd as bg
        if name == "synthetic":
            from bliss_gnn_amd.synth import chung_lu_csc
            ip, ix, _ = chung_lu_csc(2500, 600000, seed=9)
            ip, ix = ip.numpy().astype(np.int64), ix.numpy().astype(np.int32)
        elif name == "designed":
            ip, ix, _ = ref.designed_graph()
        else:
            ip, ix = gref.small_multigraph()
        _cache[name] = (bg.Graph(torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda)), ip, ix)
    return _cache[name]


def _blocks(name, g, bs):
    """The full-neighbour block of every batch, built once per (graph, batch size) and left unchanged."""
    from bliss_gnn_amd.graph import full_neighbor_block
    key = ("blocks", name, bs)
    if key not in _cache:
        V = g.num_nodes()
        _cache[key] = [(b0, min(V, b0 + bs), full_neighbor_block(g, b0, min(V, b0 + bs))) for b0 in range(0, V, bs)]
    return _cache[key]


def _feats(V, dim):
    return torch.randn(V, dim, generator=torch.Generator().manual_seed(100 + dim)).bfloat16()


def _block_rows(name, g, bs, h, reduce):
    """The block path's message passing, batch by batch."""
    from bliss_gnn_amd.nn import max_aggregate, weighted_aggregate
    out = torch.empty(g.num_nodes(), h.shape[1], dtype=BF, device=h.device)
    for b0, b1, blk in _blocks(name, g, bs):
        x = h[blk.srcdata["_ID"].long()]
        out[b0:b1] = max_aggregate(blk, x, None) if reduce == "max" else weighted_aggregate(blk, x, None, mean=True)
    return out


def _ranges(ip, bs):
    """(everything, a middle range of whole batches or None, the last batch alone)."""
    bounds, _ = gref.batch_table(ip, bs)
    nb, V = bounds.size - 1, ip.size - 1
    mid = (int(bounds[nb // 3]), int(bounds[(2 * nb) // 3])) if nb >= 3 else None
    return (0, V), mid, (int(bounds[-2]), V)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run(g, ip, bs, h, reduce, r0, r1, h_stride, out_stride, h_col0=0, guard=1):
    """rows r0 .. r1 - 1 into a NaN-filled [guard + rows + guard, out_stride] buffer, from features held at columns h_col0 .. of a
    NaN-filled [V, h_stride] buffer"""
    from bliss_gnn_amd.nn import sage_infer_spmm
    V, dim = h.shape
    hh = torch.full((V, h_stride), float("nan"), dtype=BF, device=h.device)
    hh[:, h_col0:h_col0 + dim] = h
    big = torch.full((r1 - r0 + 2 * guard, out_stride), float("nan"), dtype=BF, device=h.device)
    e0, e1 = int(ip[r0]), int(ip[r1])
    sage_infer_spmm(g.indptr, g.indices, bs, r0, r1, e0, e1 - e0, hh[:, h_col0:h_col0 + dim], big[guard:guard + r1 - r0, :dim], reduce)
    rows = big[guard:guard + r1 - r0]
    assert bool(big[:guard].isnan().all()) and bool(big[guard + r1 - r0:].isnan().all()), "guard rows"
    assert bool(rows[:, dim:].isnan().all()), "guard columns"
    return rows[:, :dim]


@pytest.mark.parametrize("dim", [1, 3, 4, 41, 64, 260])
@pytest.mark.parametrize("name,bs", CASES)
def test_range_spmm_has_the_bits_of_the_blocks(cuda, name, bs, dim):
    g, ip, ix = _graph(name, cuda)
    if name == "synthetic":                                               # the chunk lengths this case is here for
        assert set(gref.batch_chunks(ip, bs)) == CHUNKS[bs], (bs, gref.batch_chunks(ip, bs))
    V = ip.size - 1
    assert int(np.diff(ip).max()) < SPMM_MAX_ROW
    h_cpu = _feats(V, dim)
    h = h_cpu.to(cuda)
    whole, mid, last = _ranges(ip, bs)
    dst = torch.from_numpy(gref.edge_dst(ip))
    for reduce in ("mean", "max"):
        want = _block_rows(name, g, bs, h, reduce)
        run = lambda r0, r1, hs, os_, c0=0: _run(g, ip, bs, h, reduce, r0, r1, hs, os_, c0)
        got = run(0, V, dim, dim)
        assert torch.equal(_bits(got), _bits(want)), reduce
        assert torch.equal(_bits(run(0, V, dim, dim)), _bits(got)), reduce                       # a second launch
        assert torch.equal(_bits(run(0, V, dim + 4, dim + 4)), _bits(got)), reduce               # strides above dim (8-byte path kept)
        assert torch.equal(_bits(run(0, V, dim + 1, dim + 3)), _bits(got)), reduce               # strides that force one feature per lane
        assert torch.equal(_bits(run(0, V, dim + 4, dim, 1)), _bits(got)), reduce                # a slice of h off the 8-byte alignment
        if mid is not None:
            assert torch.equal(_bits(run(mid[0], mid[1], dim, dim + 4)), _bits(want[mid[0]:mid[1]])), reduce
        assert torch.equal(_bits(run(last[0], last[1], dim + 4, dim)), _bits(want[last[0]:last[1]])), reduce
        assert run(last[0], last[0], dim, dim + 4).shape == (0, dim)                             # an empty range writes nothing
        if reduce == "mean":
            r64, mag = spmm_terms(torch.from_numpy(ix), dst, V, h_cpu.float(), mean=True)
            r = assert_within(got.cpu(), r64, mag, *SPMM_K["bf16"], "sage infer mean %s bs %d dim %d" % (name, bs, dim))
            print("SAGE-INFER-MEAN %s bs %d dim %d: worst ratio %.3f" % (name, bs, dim, r))
        else:
            seg = torch.full((V, dim), -float("inf"), dtype=torch.float64).scatter_reduce(
                0, dst[:, None].expand(-1, dim), h_cpu.double()[torch.from_numpy(ix).long()], "amax", include_self=True)
            seg = torch.where(torch.isinf(seg), torch.zeros_like(seg), seg)                      # a row without edges: 0
            assert torch.equal(got.cpu().double(), seg)


def test_small_graph_against_the_restatement(cuda):
    """The exact order, restated: the kernel's rows equal tests/sage_infer_ref bit for bit on the small graph."""
    from bliss_gnn_amd.nn import sage_infer_spmm
    g, ip, ix = _graph("small", cuda)
    h_cpu = _feats(60, 7)
    h_cpu[3, 0], h_cpu[5, 0] = -0.0, 0.0
    hn = h_cpu.float().numpy()
    for bs in (1, 7, 60):
        for reduce, want in (("mean", ref.mean_f32(ip, ix, bs, hn)), ("max", ref.max_f32(ip, ix, hn))):
            out = torch.empty(60, 7, dtype=BF, device=cuda)
            sage_infer_spmm(g.indptr, g.indices, bs, 0, 60, 0, ix.size, h_cpu.to(cuda), out, reduce)
            assert np.array_equal(out.float().cpu().numpy().view(np.uint32), want.view(np.uint32)), (bs, reduce)


def test_the_designed_row_follows_the_chunk_order(cuda):
    """A row of 40 edges that starts mid-chunk, whose plain edge-order sum rounds to other bits than its chunk-order sum: the kernel
    gives the chunk order's, as the block kernel does."""
    g, ip, ix = _graph("designed", cuda)
    _, _, hn = ref.designed_graph()
    h = torch.from_numpy(hn).to(BF).to(cuda)
    r = ref.DESIGNED_ROW
    for bs in (4, 2):
        want = ref.mean_f32(ip, ix, bs, hn)
        assert want[r, 0] != ref.mean_f32(ip, ix, bs, hn, chunks=False)[r, 0]
        got = _run(g, ip, bs, h, "mean", 0, 4, 2, 2)
        assert np.array_equal(got.float().cpu().numpy().view(np.uint32), want.view(np.uint32)), bs
        assert torch.equal(_bits(got), _bits(_block_rows("designed", g, bs, h, "mean"))), bs
        mx = _run(g, ip, bs, h, "max", 0, 4, 2, 2)
        assert np.array_equal(mx.float().cpu().numpy().view(np.uint32), ref.max_f32(ip, ix, hn).view(np.uint32)), bs


@pytest.mark.parametrize("dim", [1, 4])
def test_signed_zeros_and_negative_rows(cuda, dim):
    """-0.0 and +0.0 in one row: the first edge wins the max, the mean is +0.  A row of negative values only keeps its (negative)
    maximum.  A row without edges is +0."""
    import bliss_gnn_amd as bg
    rows = [[0, 1], [1, 0], [2, 3, 2], [], [3]]                           # sources: 0 = -0.0, 1 = +0.0, 2 = -1.5, 3 = -0.25
    ip = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    ix = np.array([j for r in rows for j in r], dtype=np.int32)
    g = bg.Graph(torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda))
    col = torch.tensor([-0.0, 0.0, -1.5, -0.25, 7.0])
    h = col[:, None].expand(5, dim).contiguous().to(BF).to(cuda)
    neg0, pos0 = -32768, 0                                                # the bf16 bits of -0.0 and +0.0 as int16
    b = lambda v: int(torch.tensor([v]).to(BF).view(torch.int16))
    for bs in (5, 2):
        mx = _bits(_run(g, ip, bs, h, "max", 0, 5, dim, dim)).cpu()
        assert mx[:, 0].tolist() == [neg0, pos0, b(-0.25), pos0, b(-0.25)], (bs, mx[:, 0].tolist())
        mean = _bits(_run(g, ip, bs, h, "mean", 0, 5, dim, dim)).cpu()
        third = float(np.float32(-3.25) * (np.float32(1.0) / np.float32(3.0)))                   # the fp32 sum is exact; one fp32 product
        assert mean[:, 0].tolist() == [pos0, pos0, b(third), pos0, b(-0.25)], (bs, mean[:, 0].tolist())
        assert bool((mx == mx[:, :1]).all()) and bool((mean == mean[:, :1]).all())               # every column alike
        from bliss_gnn_amd.graph import full_neighbor_block
        for reduce, got in (("max", mx), ("mean", mean)):                 # and the block kernels agree
            from bliss_gnn_amd.nn import max_aggregate, weighted_aggregate
            for b0 in range(0, 5, bs):
                b1 = min(5, b0 + bs)
                blk = full_neighbor_block(g, b0, b1)
                x = h[blk.srcdata["_ID"].long()]
                w = max_aggregate(blk, x, None) if reduce == "max" else weighted_aggregate(blk, x, None, mean=True)
                assert torch.equal(_bits(w).cpu(), got[b0:b1]), (bs, reduce, b0)
