"""GPU suite (-m gpu): the entry points of csrc/gcn_infer.hip alone.

bliss_gcn_infer_src_norms must equal the NumPy float32 restatement (tests/gcn_infer_ref.py) bit for bit; bliss_gcn_infer_spmm must
equal, bit for bit, what nn._gcn_spmm + bliss_gcn_norms give on graph.full_neighbor_block of every batch, and lie within
gcn_ref.GCN_SPMM_K = (1, 0.25) of the float64 restatement (one rounding at the store; an fp32 sum of at most 16 384 terms -- the
longest row has 1569).

Graphs: chung_lu_csc(2500, 600000, seed=9) at batch sizes 128 / 37 (every batch at 16-edge chunks), 300 (chunks of 32 and 16 in
one run) and 1250 (64) -- asserted from indptr -- and the 60-node multigraph of gcn_infer_ref.small_multigraph at 1 / 7 / 60 / 100.
dim 1, 7 (one feature per lane), 16, 256 (8-byte accesses).  Ranges: everything, a middle range of whole batches, the short last
batch alone, an empty range; a feature row stride above dim; NaN-filled outputs with guard rows and columns; two launches."""
import numpy as np
import pytest
import torch

import gcn_infer_ref as ref
import gcn_ref
from bounds import assert_within

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
        else:
            ip, ix = ref.small_multigraph()
        _cache[name] = (bg.Graph(torch.from_numpy(ip).to(cuda), torch.from_numpy(ix).to(cuda)), ip, ix)
    return _cache[name]


def _feats(V, dim):
    return torch.randn(V, dim, generator=torch.Generator().manual_seed(100 + dim)).bfloat16()


def _ns(g, bs, ranges, cuda):
    """ns of the given ranges (rows), each by its own call, in a NaN-filled buffer with one guard entry at either end."""
    from bliss_gnn_amd.nn import gcn_infer_src_norms, gcn_infer_state
    E = g.num_edges()
    buf = torch.full((E + 2,), float("nan"), dtype=torch.float32, device=cuda)
    state = gcn_infer_state()
    off = g.indptr.cpu()
    for r0, r1 in ranges:
        e0, e1 = int(off[r0]), int(off[r1])
        gcn_infer_src_norms(g.indptr, g.indices, bs, r0, r1, e0, e1 - e0, buf[1 + e0:1 + e1], state)
    return buf


def _block_rows(g, bs, h):
    """The block path's message passing: bliss_gcn_norms + nn._gcn_spmm on the full-neighbour block of every batch."""
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd.graph import full_neighbor_block
    from bliss_gnn_amd.nn import _gcn_spmm
    V, st = g.num_nodes(), torch.cuda.current_stream().cuda_stream
    out = torch.empty(V, h.shape[1], dtype=BF, device=h.device)
    ns_e = []
    for b0 in range(0, V, bs):
        b1 = min(V, b0 + bs)
        blk = full_neighbor_block(g, b0, b1)
        t_indptr, t_edge = blk.transposed()
        K, S = blk.num_src_nodes(), blk.num_dst_nodes()
        ns = torch.empty(K, dtype=torch.float32, device=h.device)
        nd = torch.empty(S, dtype=torch.float32, device=h.device)
        _lib.check(_lib.lib.bliss_gcn_norms(blk.indptr.data_ptr(), S, t_indptr.data_ptr(), K, nd.data_ptr(), ns.data_ptr(), st), "norms")
        x = h[blk.srcdata["_ID"].long()]
        out[b0:b1] = _gcn_spmm(False, (blk.indptr, blk.src, blk.dst, t_indptr, t_edge), None, ns, nd, x, S, 0)
        ns_e.append(ns[blk.src.long()])
    return out, torch.cat(ns_e)


def _check_classes(name, ip, bs):
    if name == "synthetic":                                               # the chunk lengths this case is here for
        assert set(ref.batch_chunks(ip, bs)) == CHUNKS[bs], (bs, ref.batch_chunks(ip, bs))


def _ranges(ip, bs):
    """(everything, a middle range of whole batches or None, the last batch alone)."""
    bounds, _ = ref.batch_table(ip, bs)
    nb, V = bounds.size - 1, ip.size - 1
    mid = (int(bounds[nb // 3]), int(bounds[(2 * nb) // 3])) if nb >= 3 else None
    return (0, V), mid, (int(bounds[-2]), V)


@pytest.mark.parametrize("name,bs", CASES)
def test_source_norms_are_the_numpy_values(cuda, name, bs):
    g, ip, ix = _graph(name, cuda)
    _check_classes(name, ip, bs)
    want = torch.from_numpy(ref.norms(ip, ix, bs)[0])
    E = ix.size
    whole, mid, last = _ranges(ip, bs)
    buf = _ns(g, bs, [whole], cuda)
    assert torch.equal(buf[1:1 + E].cpu(), want) and bool(buf[0].isnan()) and bool(buf[E + 1].isnan())
    assert torch.equal(_ns(g, bs, [whole], cuda)[1:1 + E], buf[1:1 + E])
    assert torch.equal(_block_rows(g, bs, _feats(ip.size - 1, 1).to(cuda))[1].cpu(), want)         # = the blocks' ns[src]
    if mid is not None:                                                   # the graph in three calls: the same values
        parts = _ns(g, bs, [(0, mid[0]), mid, (mid[1], ip.size - 1)], cuda)
        assert torch.equal(parts[1:1 + E].cpu(), want)
    only = _ns(g, bs, [last, (last[0], last[0])], cuda).cpu()             # the last batch alone (and an empty range): nothing else written
    e0 = int(ip[last[0]])
    assert torch.equal(only[1 + e0:1 + E], want[e0:]) and bool(only[:1 + e0].isnan().all()) and bool(only[E + 1].isnan())


@pytest.mark.parametrize("dim", [1, 7, 16, 256])
@pytest.mark.parametrize("name,bs", CASES)
def test_range_spmm_has_the_bits_of_the_blocks(cuda, name, bs, dim):
    from bliss_gnn_amd.nn import gcn_infer_spmm
    g, ip, ix = _graph(name, cuda)
    _check_classes(name, ip, bs)
    V, E = ip.size - 1, ix.size
    h_cpu = _feats(V, dim)
    h = h_cpu.to(cuda)
    ns = _ns(g, bs, [(0, V)], cuda)[1:1 + E]
    want = _block_rows(g, bs, h)[0]
    bits = lambda t: t.contiguous().view(torch.int16)
    off = lambda r: int(ip[r])

    def run(r0, r1, h_stride, out_stride, guard=1):
        """rows r0 .. r1 - 1 into a NaN-filled [guard + rows + guard, out_stride] buffer from features of row stride h_stride"""
        hh = torch.full((V, h_stride), float("nan"), dtype=BF, device=cuda)
        hh[:, :dim] = h
        big = torch.full((r1 - r0 + 2 * guard, out_stride), float("nan"), dtype=BF, device=cuda)
        gcn_infer_spmm(g.indptr, g.indices, bs, r0, r1, off(r0), off(r1) - off(r0), ns[off(r0):off(r1)] if r1 > r0 else ns[:0],
                       hh[:, :dim], big[guard:guard + r1 - r0, :dim])
        rows = big[guard:guard + r1 - r0]
        assert bool(big[:guard].isnan().all()) and bool(big[guard + r1 - r0:].isnan().all()), "guard rows"
        assert bool(rows[:, dim:].isnan().all()), "guard columns"
        return rows[:, :dim]

    whole, mid, last = _ranges(ip, bs)
    got = run(0, V, dim, dim)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(run(0, V, dim, dim)), bits(got))                                     # a second launch
    assert torch.equal(bits(run(0, V, dim + 4, dim + 4)), bits(got))                             # strides above dim (8-byte path kept)
    assert torch.equal(bits(run(0, V, dim + 1, dim + 3)), bits(got))                             # strides that force one feature per lane
    if mid is not None:
        assert torch.equal(bits(run(mid[0], mid[1], dim, dim + 4)), bits(want[mid[0]:mid[1]]))
    assert torch.equal(bits(run(last[0], last[1], dim + 4, dim)), bits(want[last[0]:last[1]]))
    assert run(last[0], last[0], dim, dim + 4).shape == (0, dim)                                 # an empty range writes nothing
    ref64, mag = ref.spmm_f64(ip, ix, bs, h_cpu.float().numpy())
    r = assert_within(got.cpu(), torch.from_numpy(ref64), torch.from_numpy(mag), *gcn_ref.GCN_SPMM_K, "gcn infer spmm %s bs %d dim %d" % (name, bs, dim))
    print("GCN-INFER-SPMM %s bs %d dim %d: worst ratio %.3f" % (name, bs, dim, r))


def test_small_graph_against_the_float32_emulation(cuda):
    """The exact order, restated: the kernel's rows equal tests/gcn_infer_ref.spmm_f32 bit for bit on the small graph."""
    from bliss_gnn_amd.nn import gcn_infer_spmm
    g, ip, ix = _graph("small", cuda)
    h_cpu = _feats(60, 7)
    for bs in (1, 7, 60):
        ns = _ns(g, bs, [(0, 60)], cuda)[1:1 + ix.size]
        out = torch.empty(60, 7, dtype=BF, device=cuda)
        gcn_infer_spmm(g.indptr, g.indices, bs, 0, 60, 0, ix.size, ns, h_cpu.to(cuda), out)
        assert np.array_equal(out.float().cpu().numpy(), ref.spmm_f32(ip, ix, bs, h_cpu.float().numpy())), bs
