"""GPU suite: bliss_gat_infer_fwd (GATv2 full-neighbour inference off the graph's CSC) against the fused
training kernel on the full-neighbour block of the same destination range: the same bits, with and without the epilogue."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 7), (2, 8), (4, 64), (4, 256), (8, 32)]
SLOPE = 0.2
# graph (b): in-degrees at the chunk (64) and segment (256) boundaries; rows 0 and 39 have no in-edges
DEGREES_B = [0, 1, 63, 64, 65, 255, 256, 257, 512, 513] + [2, 3, 5, 0, 7, 130, 1, 1, 64, 9] + [4] * 9 + [300, 6, 6, 2, 128, 31, 33, 1, 192, 12, 0]
_graphs = {}


def _graph_a(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(4000, 200000, seed=9)
    return bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda))


def _graph_b(cuda):
    """40 nodes, a multigraph (more in-edges than nodes): row 1's one edge is a self loop, all 64 in-edges of row 3 come from node 5
    (a column of parallel edges), the others from seeded random sources."""
    import bliss_gnn_amd as bg
    V = len(DEGREES_B)
    assert V == 40 and DEGREES_B[0] == 0 and DEGREES_B[-1] == 0
    gen = torch.Generator().manual_seed(17)
    cols = []
    for r, d in enumerate(DEGREES_B):
        c = torch.randint(0, V, (d,), generator=gen, dtype=torch.int32)
        if r == 1:
            c[:] = 1
        if r == 3:
            c[:] = 5
        cols.append(c)
    ip = torch.zeros(V + 1, dtype=torch.int64)
    ip[1:] = torch.tensor(DEGREES_B).cumsum(0)
    return bg.Graph(ip.to(cuda), torch.cat(cols).to(cuda))


def _graph(name, cuda):
    if name not in _graphs:
        _graphs[name] = (_graph_a if name == "a" else _graph_b)(cuda)
    return _graphs[name]


def _ranges(name, g):
    V = g.num_nodes()
    deg = (g.indptr[1:] - g.indptr[:-1]).cpu()
    hub = int(deg.argmax())
    step = 300 if name == "a" else 7
    if name == "a":
        assert int(deg[hub]) > 600                                    # at least three segments
    out = [(0, V)] + [(b, min(V, b + step)) for b in range(0, V, step)] + [(hub, hub + 1), (hub, min(V, hub + step)), (hub, hub)]
    if name == "b":
        out += [(8, 9), (9, 10), (0, 1), (V - 1, V), (5, 9)]         # the 512- and 513-edge rows alone, the empty rows alone
    return out


def _fused_state(cuda):
    return dict(ctr=torch.zeros(2, dtype=torch.int64, device=cuda), ticket=torch.zeros(1, dtype=torch.int32, device=cuda), seed=0,
                err=torch.zeros(1, dtype=torch.int32, device=cuda), row_ws=None)


def _nan_buffer(n, HD, cuda):
    """[n + 2, HD + 8] of NaN: a guard row on each side of the n output rows and eight guard columns behind each of them."""
    return torch.full((n + 2, HD + 8), float("nan"), dtype=torch.bfloat16, device=cuda)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_infer_rows_have_the_bits_of_the_fused_kernel(cuda, name, H, D):
    from bliss_gnn_amd.graph import full_neighbor_block
    from bliss_gnn_amd.nn import GLUE_ACT_ELU, _GatFusedMP, gat_glue, gat_infer_layer, gat_infer_state
    g = _graph(name, cuda)
    V, HD = g.num_nodes(), H * D
    gen = torch.Generator().manual_seed(100 * H + D)
    # all nodes' fc_src rows with a row stride above H*D (a multiple of 4 where the 8-byte loads need it)
    wide = torch.zeros(V, HD + (4 if D % 4 == 0 else 3), dtype=torch.bfloat16, device=cuda)
    wide[:, :HD] = (torch.randn(V, HD, generator=gen) * 0.5).bfloat16().to(cuda)
    feat = wide[:, :HD]
    attn = (torch.randn(1, H, D, generator=gen) * 0.7).bfloat16().to(cuda)
    res_all = torch.randn(V, HD, generator=gen).bfloat16().to(cuda)
    st, fst = gat_infer_state(cuda), _fused_state(cuda)
    for b0, b1 in _ranges(name, g):
        n = b1 - b0
        edges = int(g.indptr[b1]) - int(g.indptr[b0])
        buf = _nan_buffer(n, HD, cuda)
        before = _bits(buf).clone()
        out = buf[1:n + 1, :HD]
        gat_infer_layer(g.indptr, g.indices, b0, b1, edges, feat, attn, H, D, SLOPE, out, state=st)
        first = out.clone()
        after = _bits(buf).clone()
        assert torch.equal(after[0], before[0]) and torch.equal(after[n + 1], before[n + 1]), ("guard rows", b0, b1)
        assert torch.equal(after[:, HD:], before[:, HD:]), ("guard columns", b0, b1)
        if n == 0:
            # the entry point itself with n_rows = 0 (the wrapper returns before it): 0, nothing launched, nothing written
            from bliss_gnn_amd import _lib
            t = _lib.GatInfer()
            t.indptr, t.indices, t.row0, t.n_rows, t.n_edges = g.indptr.data_ptr(), g.indices.data_ptr(), b0, 0, 0
            t.feat, t.feat_stride, t.attn, t.heads, t.head_dim, t.negative_slope = feat.data_ptr(), feat.stride(0), attn.data_ptr(), H, D, SLOPE
            t.out, t.out_stride = buf.data_ptr(), buf.stride(0)
            assert _lib.lib.bliss_gat_infer_fwd(C.byref(t), torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(_bits(buf), before)
            continue
        # the reference: the fused training forward (p = 0) on the full-neighbour block of the range
        if edges:
            blk = full_neighbor_block(g, b0, b1)
            with torch.no_grad():
                rst, _ = _GatFusedMP.apply(feat[blk.srcdata["_ID"].long()], attn, blk, H, D, SLOPE, 0.0, fst)
        else:                                                         # (the fused entry point takes no block without edges: zero rows)
            rst = torch.zeros(n, HD, dtype=torch.bfloat16, device=cuda)
        assert torch.equal(_bits(first), _bits(rst)), ("rst", b0, b1, H, D)
        # a second launch on the same scratch: the row state cleaned itself
        out.fill_(float("nan"))
        gat_infer_layer(g.indptr, g.indices, b0, b1, edges, feat, attn, H, D, SLOPE, out, state=st)
        assert torch.equal(_bits(out), _bits(first)), ("second launch", b0, b1)
        # residual + ELU in the same launch == gat_glue on the fused kernel's rst
        want = gat_glue(rst, res_all[b0:b1], H, D, act=GLUE_ACT_ELU)[0]
        out.fill_(float("nan"))
        gat_infer_layer(g.indptr, g.indices, b0, b1, edges, feat, attn, H, D, SLOPE, out, res=res_all[b0:b1], act=GLUE_ACT_ELU, state=st)
        assert torch.equal(_bits(out), _bits(want)), ("epilogue", b0, b1, H, D)
        assert torch.equal(_bits(buf)[0], before[0]) and torch.equal(_bits(buf)[n + 1], before[n + 1]) and torch.equal(_bits(buf)[:, HD:], before[:, HD:])
        # residual alone (the last layer of a residual model has no activation)
        want = gat_glue(rst, res_all[b0:b1], H, D)[0]
        gat_infer_layer(g.indptr, g.indices, b0, b1, edges, feat, attn, H, D, SLOPE, out, res=res_all[b0:b1], state=st)
        assert torch.equal(_bits(out), _bits(want)), ("residual", b0, b1, H, D)
    assert int(st["err"].item()) == 0 and int(fst["err"].item()) == 0
    assert int(st["row_ws"].abs().max().item()) == 0                  # every shared row's words are back at zero


def test_rows_without_in_edges_are_zero(cuda):
    from bliss_gnn_amd.nn import gat_infer_layer
    g = _graph("b", cuda)
    V, H, D = g.num_nodes(), 2, 8
    feat = torch.randn(V, H * D, generator=torch.Generator().manual_seed(1)).bfloat16().to(cuda)
    attn = torch.randn(1, H, D, generator=torch.Generator().manual_seed(2)).bfloat16().to(cuda)
    out = torch.full((V, H * D), float("nan"), dtype=torch.bfloat16, device=cuda)
    gat_infer_layer(g.indptr, g.indices, 0, V, g.num_edges(), feat, attn, H, D, SLOPE, out)
    zero = [r for r, d in enumerate(DEGREES_B) if d == 0]
    assert len(zero) == 3 and bool((out[zero] == 0).all()) and bool(torch.isfinite(out.float()).all())
    # a single in-edge: the softmax coefficient is 1, the row is its source's (row 1: the self loop)
    assert torch.equal(out[1], feat[1]) and torch.equal(out[16], feat[int(g.indices[int(g.indptr[16])])])


def test_wrapper_refuses_what_the_kernel_does_not_take(cuda):
    from bliss_gnn_amd.nn import gat_infer_layer
    g = _graph("b", cuda)
    V = g.num_nodes()
    attn = torch.zeros(1, 2, 8, dtype=torch.bfloat16, device=cuda)
    out = torch.zeros(V, 16, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(NotImplementedError, match="bf16"):
        gat_infer_layer(g.indptr, g.indices, 0, V, g.num_edges(), torch.zeros(V, 16, device=cuda), attn, 2, 8, SLOPE, out)
    with pytest.raises(NotImplementedError, match="bliss_gat_fused_supported"):
        gat_infer_layer(g.indptr, g.indices, 0, V, g.num_edges(), torch.zeros(V, 2 * 258, dtype=torch.bfloat16, device=cuda),
                        torch.zeros(1, 2, 258, dtype=torch.bfloat16, device=cuda), 2, 258, SLOPE, torch.zeros(V, 516, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(ValueError):
        gat_infer_layer(g.indptr, g.indices, 0, V + 1, g.num_edges(), torch.zeros(V, 16, dtype=torch.bfloat16, device=cuda), attn, 2, 8, SLOPE, out)


def test_more_rows_than_the_one_sweep_descriptor_path(cuda):
    """A range of more than 16384 rows takes the descriptor builder's scanning path: same bits as the fused kernel on the block,
    and as two ranges that each take the one-sweep path."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.graph import full_neighbor_block
    from bliss_gnn_amd.nn import _GatFusedMP, gat_infer_layer, gat_infer_state
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(20000, 600000, seed=4)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda))
    V, H, D = g.num_nodes(), 2, 8
    assert int((ip[1:] - ip[:-1]).max()) > 256                         # shared rows among them
    feat = (torch.randn(V, H * D, generator=torch.Generator().manual_seed(1)) * 0.5).bfloat16().to(cuda)
    attn = torch.randn(1, H, D, generator=torch.Generator().manual_seed(2)).bfloat16().to(cuda)
    st = gat_infer_state(cuda)
    whole = torch.empty(V, H * D, dtype=torch.bfloat16, device=cuda)
    gat_infer_layer(g.indptr, g.indices, 0, V, g.num_edges(), feat, attn, H, D, SLOPE, whole, state=st)
    halves = torch.empty_like(whole)
    cut = 16384
    e_cut = int(g.indptr[cut])
    gat_infer_layer(g.indptr, g.indices, 0, cut, e_cut, feat, attn, H, D, SLOPE, halves[:cut], state=st)
    gat_infer_layer(g.indptr, g.indices, cut, V, g.num_edges() - e_cut, feat, attn, H, D, SLOPE, halves[cut:], state=st)
    blk = full_neighbor_block(g, 0, V)
    with torch.no_grad():
        rst, _ = _GatFusedMP.apply(feat[blk.srcdata["_ID"].long()], attn, blk, H, D, SLOPE, 0.0, _fused_state(cuda))
    assert torch.equal(_bits(whole), _bits(rst)) and torch.equal(_bits(halves), _bits(rst))
    assert int(st["err"].item()) == 0
