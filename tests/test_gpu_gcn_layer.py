"""GPU suite (-m gpu): a ``GraphConv(transforms="tile")`` layer -- forward, d feat, dW and db per element
against fp64 autograd of the formula on the same bf16 operands (gcn_ref.layer_terms), on the edge-shape block exact-size and
capacity-padded (NaN feature rows, edge weights and gradient rows past the live counts; every buffer the layer allocates
pre-filled with NaN) -- and the epilogue kernels on their own against the NumPy restatement, bit for bit.

Constants (gcn_ref.layer_k, composed from bounds.dense_k and the SpMM's (1, 0.25)): a bf16 tensor stored between two launches
costs 1, a stored SpMM result 1.25, an fp32-accumulated product n_terms * 2^-16, the last rounding is k_ulp = 1:
    out  (1, 2.25 + (fin + 1) 2^-16)      the product and the SpMM result stored in front of the epilogue's add
    d x  (1, 1.25 + fout 2^-16)           dZ (SpMM) in front of the product, or the stored product in front of the SpMM's sum
    d W  (1, 1.25 + (rows + 80) 2^-16)    dZ or the stored aggregate in front of the chunked row sum of bliss_sage_wgrad
    d b  (1, (rows + rows / 32 + 1) 2^-16)  fp32 chunk sums, nothing stored in front
all tighter than the library path's GCN_K = (1, 4): the tile path rounds at fewer points.  With the ReLU the backward's mask is
taken from the kernel's stored output (out > 0), after the forward check has held every element to its bound: where the
reference is positive the output is compared as it is; where it is <= 0 the output itself (>= 0) must lie within the bound of
the pre-activation value, which is what ``ref + out`` against ``ref`` states.
db must be bit-equal between the padded and the exact block and across two runs; out and d x likewise on the live rows."""
import numpy as np
import pytest
import torch

import gcn_ref as ref
from bounds import GCN_K, assert_within, dense_k, edge_shape_spec, padded_block, to_block
from gat_glue_ref import rbf as rbf_np

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture
def nan_empty(monkeypatch):
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)


@pytest.fixture(scope="module")
def blocks(cuda):
    spec = edge_shape_spec()
    pad = padded_block(spec, cuda)
    pad._counts_dev[3] = spec.K                         # bliss_layer_counts_t::K: the dense products are bound by the live source count
    return spec, to_block(spec, cuda), pad


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


@pytest.mark.parametrize("fin,fout,relu", [(48, 16, True), (16, 48, False), (602, 256, True), (1024, 7, False), (100, 256, True)])
def test_layer_forward_and_gradients_per_element(cuda, blocks, nan_empty, fin, fout, relu):
    from bliss_gnn_amd.nn import GraphConv
    spec, blk, pad = blocks
    S, K, B = spec.S, spec.K, spec.B
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    torch.manual_seed(2)
    layer = GraphConv(fin, fout, activation=torch.relu if relu else None, allow_zero_in_degree=True, transforms="tile").to(cuda).bfloat16()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(fout, generator=torch.Generator().manual_seed(9)).bfloat16() * 0.1)
    assert layer.tile_refusal() is None
    gen = torch.Generator().manual_seed(3 + fin)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=BF)
    x = torch.cat([torch.randn(K, fin, generator=gen).bfloat16(), nan(Kc - K, fin)]).to(cuda)
    w = torch.cat([(torch.rand(B, generator=gen) + 0.05).bfloat16(), nan(Bc - B)]).to(cuda)
    g = torch.cat([torch.randn(S, fout, generator=gen).bfloat16(), nan(Sc - S, fout)]).to(cuda)
    runs = {}
    for name, b, k_rows, s_rows, n_e in (("exact", blk, K, S, B), ("padded", pad, Kc, Sc, Bc), ("again", pad, Kc, Sc, Bc)):
        layer.zero_grad(set_to_none=True)
        xi = x[:k_rows].clone().requires_grad_(True)
        out = layer(b, xi, edge_weight=w[:n_e].contiguous())
        out.backward(g[:s_rows].contiguous())
        runs[name] = (out.detach(), xi.grad, layer.weight.grad.clone(), layer.bias.grad.clone())
    torch.cuda.synchronize()
    out, dx, dW, db = runs["exact"]
    src, dst = spec.src.to(cuda), spec.dst.to(cuda)
    T = ref.layer_terms(src, dst, S, K, x[:K], layer.weight, layer.bias, w[:B], g[:S], mask=(out > 0) if relu else None)
    k = ref.layer_k(fin, fout, Kc)
    assert all(kk[0] <= GCN_K[0] and kk[1] <= GCN_K[1] for kk in k.values())
    rst = T["rst"]
    got_out = torch.where(rst > 0, out.double(), rst + out.double()) if relu else out
    r = {"out": assert_within(got_out, rst, T["mag_rst"], *k["out"], "tile graphconv out")}
    for name, (o, d_x, d_W, d_b) in runs.items():
        r[name + " d_x"] = assert_within(d_x[:K], T["d_x"], T["mag_d_x"], *k["d_x"], name + " d feat")
        r[name + " d_W"] = assert_within(d_W, T["d_W"], T["mag_d_W"], *k["d_W"], name + " d W")
        r[name + " d_b"] = assert_within(d_b, T["d_b"], T["mag_d_b"], *k["d_b"], name + " d b")
        assert torch.equal(_bits(o[:S]), _bits(out)) and torch.equal(_bits(d_x[:K]), _bits(dx)), name + ": live rows bit-equal to the exact block"
        assert torch.equal(_bits(d_b), _bits(db)), name + ": db bit-equal"
        assert not bool(o[S:].any()) and not bool(d_x[K:].any()), name + ": rows past the counts must be zero"
    assert torch.equal(_bits(runs["padded"][2]), _bits(runs["again"][2])), "dW repeats"
    print("GCN-LAYER %dx%d relu %d:" % (fin, fout, relu), " ".join("%s %.3f" % kv for kv in sorted(r.items())))


def test_layer_refusals(cuda, blocks):
    from bliss_gnn_amd.nn import GraphConv
    spec, blk, _ = blocks
    with pytest.raises(ValueError, match="transforms"):
        GraphConv(8, 8, transforms="fast")
    x = torch.zeros(spec.K, 8, dtype=BF, device=cuda)
    wide = GraphConv(8, 1025, transforms="tile").to(cuda).bfloat16()
    assert "out_feats <= 1024" in wide.tile_refusal("layer 3") and "layer 3" in wide.tile_refusal("layer 3")
    with pytest.raises(NotImplementedError, match="1024"):
        wide(blk, x)
    with pytest.raises(NotImplementedError, match="ReLU"):
        GraphConv(8, 8, activation=torch.tanh, transforms="tile").to(cuda).bfloat16()(blk, x)
    with pytest.raises(NotImplementedError, match="bf16 parameters"):
        GraphConv(8, 8, transforms="tile").to(cuda)(blk, x)
    with pytest.raises(NotImplementedError, match="bf16 features"):
        GraphConv(8, 8, transforms="tile").to(cuda).bfloat16()(blk, x.float())


# ------------------------------------------------------------------------------------------------ the epilogue on its own
ROWS = [(rows, live) for rows in (1, 33, 65) for live in sorted({0, 1, rows - 1, rows})]


def _db_restated(din, live, chunk):
    """db as the kernels sum it: fp32 in row order inside chunks of ``chunk`` rows, the chunk sums added in chunk order."""
    total = np.zeros(din.shape[1], np.float32)
    for r0 in range(0, live, chunk):
        part = np.zeros(din.shape[1], np.float32)
        for r in range(r0, min(live, r0 + chunk)):
            part = part + din[r]
        total = total + part
    return rbf_np(total)


@pytest.mark.parametrize("rows,live", ROWS)
@pytest.mark.parametrize("width", [7, 16, 256])
def test_epilogue_forward_and_backward_bit_for_bit(cuda, width, rows, live):
    import ctypes as C
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd import nn as bnn
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1000 * width + 10 * rows + live)
    a = rbf_np(rng.standard_normal((rows, width)).astype(np.float32) * 2)
    bias = rbf_np(rng.standard_normal(width).astype(np.float32))
    dout = rbf_np(rng.standard_normal((rows, width)).astype(np.float32))
    relu = width != 16
    chunk = int(_lib.lib.bliss_gcn_db_chunk_rows())
    assert chunk == 32
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(BF)

    def padded(arr):
        t = dev(arr)
        t[live:] = float("nan")
        return t.to(cuda)

    n_dev = torch.tensor([live], dtype=torch.int32, device=cuda)
    for p in (0.0, 0.5):
        state = bnn.gat_drop_state(3, cuda)
        for launch in range(2 if p > 0 else 1):                                 # the second launch draws with counter 1
            ad, dd, bd = padded(a), padded(dout), dev(bias).to(cuda)
            nanbuf = lambda *shape: torch.full(shape, float("nan"), dtype=BF, device=cuda)
            out, norm, din, db = nanbuf(rows, width), nanbuf(rows), nanbuf(rows, width), nanbuf(width)
            part = torch.full((max(((rows + chunk - 1) // chunk) * width, 4),), float("nan"), dtype=torch.float32, device=cuda)
            used = torch.full((1,), -1, dtype=torch.int32, device=cuda)
            t = bnn._gcn_epilogue_args(rows, n_dev.data_ptr(), width, relu, p, state, used)
            t.a, t.a_stride, t.bias = ad.data_ptr(), ad.stride(0), bd.data_ptr()
            t.out, t.out_stride, t.norm_out = out.data_ptr(), out.stride(0), norm.data_ptr()
            _lib.check(_lib.lib.bliss_gcn_epilogue_fwd(C.byref(t), st), "fwd")
            t.dout, t.dout_stride, t.din, t.din_stride = dd.data_ptr(), dd.stride(0), din.data_ptr(), din.stride(0)
            t.db, t.db_partials = db.data_ptr(), part.data_ptr()
            _lib.check(_lib.lib.bliss_gcn_epilogue_bwd(C.byref(t), st), "bwd")
            torch.cuda.synchronize()
            if p > 0:
                assert int(used[0]) == launch and int(state["ctr"][0]) == launch + 1
            w_out = ref.epilogue_fwd(a, bias, relu, p, state["seed"], launch, live)
            w_din, db64, mag_db = ref.epilogue_bwd(dout, w_out, relu, p, state["seed"], launch, live)
            g_out, g_din = out.float().cpu().numpy(), din.float().cpu().numpy()
            assert np.array_equal(g_out, w_out), ("out", p, launch)
            assert np.array_equal(g_din, w_din), ("din", p, launch)
            assert np.array_equal(db.float().cpu().numpy(), _db_restated(w_din, live, chunk)), ("db bits", p, launch)
            assert_within(db, torch.from_numpy(db64), torch.from_numpy(mag_db), *dense_k(live + live // chunk + 1), "db")
            assert torch.equal(_bits(norm[:live]), _bits(bnn.embed_norm(out[:live]))) if live else True
            assert not bool(norm[live:].any())
            want_norm = torch.from_numpy(ref.row_norm(w_out))
            assert_within(norm, want_norm, want_norm, *dense_k(width), "norm")


def test_epilogue_without_bias_and_norm(cuda):
    """bias NULL, norm_out NULL, no ReLU, p = 0: the live rows are copied, the rest zeroed; the backward passes the live rows on."""
    import ctypes as C
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd import nn as bnn
    st = torch.cuda.current_stream().cuda_stream
    rows, live, width = 40, 17, 12
    a = torch.randn(rows, width, generator=torch.Generator().manual_seed(1)).bfloat16().to(cuda)
    out, din = torch.full_like(a, float("nan")), torch.full_like(a, float("nan"))
    n_dev = torch.tensor([live], dtype=torch.int32, device=cuda)
    t = bnn._gcn_epilogue_args(rows, n_dev.data_ptr(), width, False, 0.0, None, None)
    t.a, t.a_stride, t.out, t.out_stride = a.data_ptr(), a.stride(0), out.data_ptr(), out.stride(0)
    _lib.check(_lib.lib.bliss_gcn_epilogue_fwd(C.byref(t), st), "fwd")
    t.dout, t.dout_stride, t.din, t.din_stride = a.data_ptr(), a.stride(0), din.data_ptr(), din.stride(0)
    _lib.check(_lib.lib.bliss_gcn_epilogue_bwd(C.byref(t), st), "bwd")
    torch.cuda.synchronize()
    for got in (out, din):
        assert torch.equal(_bits(got[:live]), _bits(a[:live])) and not bool(got[live:].any())
