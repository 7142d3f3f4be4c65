"""GPU suite: bliss_tile_gemm_wide (csrc/sage.hip) -- k_tile_gemm with K walked in panels of 1024 columns --
element by element against float64 on the same bf16 operands with the bound of tests/bounds.py,

    |got - ref| <= k_ulp * ulp_bf16(ref) + k_mag * 2^-8 * mag,     (k_ulp, k_mag) = bounds.dense_k(K1 + K2 (+ 1 with a bias)),

at the K where a panel walk goes wrong: one column, one MFMA step and one W slab past a seam (1025, 1039 .. 1041, 1087 .. 1089),
the Cora width 1433 (odd: element-wise staging), two and three seams (2047 .. 2049, 3073) and the limit 16384.  The conventions
are those of tests/test_gpu_sage_dense_edges.py: operand rows beyond the device-side count are NaN (Inf when gathered), outputs
are pre-filled with NaN, a misaligned operand is an odd-stride window of a NaN buffer, every test prints ``RATIO`` lines.
Beside the bound: an exact one-hot probe of the seam columns, bit equality with bliss_tile_gemm wherever one panel covers K,
and bit equality of in_norm / out_norm with embed_norm and of a_copy with the gathered rows at every K."""
import ctypes as C

import pytest
import torch

from bounds import assert_within, dense_k, gemm_terms, ulp_bf16
from wide_cases import BF, INF, NAN, fwd_inputs, one_hot_rows, rand

pytestmark = pytest.mark.gpu


def _report(case, ratios):
    for k, v in ratios.items():
        print("RATIO %s %s %.3f" % (case, k, v))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _place(t, dev, view, fill=NAN):
    """``t`` on the device: contiguous, or (view) as the window base[:, 1:1 + cols] of a ``fill``-ed buffer with an odd row
    stride: the data pointer is 2 bytes off 4-byte alignment and every second row starts on an odd element."""
    if not view:
        return t.to(dev).contiguous(), None
    rows, cols = t.shape
    width = cols + 3 + (cols % 2)                            # odd, >= cols + 3
    base = torch.full((rows, width), fill, dtype=t.dtype, device=dev)
    v = base[:, 1:1 + cols]
    v.copy_(t.to(dev))
    assert v.data_ptr() % 4 == 2 and v.stride(0) % 2 == 1
    return v, base


def _frame_untouched(base, cols):
    return bool(torch.isnan(base[:, 0]).all()) and bool(torch.isnan(base[:, 1 + cols:]).all())


def _launch(entry, first, second=None):
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd._engine import _stream
    fn = {"wide": _lib.lib.bliss_tile_gemm_wide, "tile": _lib.lib.bliss_tile_gemm}[entry]
    _lib.check(fn(C.byref(first), None if second is None else C.byref(second), _stream()), "bliss_tile_gemm(%s)" % entry)


def _fwd(dev, K1, N, M, K2=0, gather=False, bias=True, relu=False, views=(), pad=NAN, p=0.0, seed=0, entry="wide", inputs=None):
    """One launch of ``entry`` on the operands of wide_cases.fwd_inputs.  Returns the outputs, the fp64 reference and magnitude."""
    from bliss_gnn_amd import nn as bnn
    c = inputs or fwd_inputs(K1, N, M, K2=K2, gather=gather, bias=bias, pad=pad, seed=seed)
    mb = c["mb"]
    src1, _ = _place(c["table"] if gather else c["a1"], dev, "a1" in views)
    w1d, _ = _place(c["w1"], dev, "w1" in views)
    a2d = w2d = None
    if K2:
        a2d, _ = _place(c["a2"], dev, "a2" in views)
        w2d, _ = _place(c["w2"], dev, "w2" in views)
    out, out_base = _place(torch.full((mb, N), NAN, dtype=BF), dev, "out" in views)
    copy, copy_base = _place(torch.full((mb, K1), NAN, dtype=BF), dev, "copy" in views) if gather else (None, None)
    in_norm = torch.full((mb,), NAN, dtype=BF, device=dev)
    out_norm = torch.full((mb,), NAN, dtype=BF, device=dev)
    m_dev = torch.tensor([M], dtype=torch.int32, device=dev)
    ctr = torch.zeros(66, dtype=torch.int64, device=dev) if p > 0 else None
    bd = None if c["b"] is None else c["b"].to(dev)
    _launch(entry, bnn._tg_args(src1, w1d, out, mb, ids=c["ids"].to(torch.int32).to(dev) if gather else None, a2=a2d, w2=w2d, bias=bd,
                                m_dev=m_dev.data_ptr(), a_copy=copy, in_norm=in_norm, out_norm=out_norm, relu=relu, p=p, seed=77, ctr=ctr))
    torch.cuda.synchronize()
    if out_base is not None:
        assert _frame_untouched(out_base, N), "written beside the output rows"
    if copy_base is not None:
        assert _frame_untouched(copy_base, K1), "written beside the copied rows"
    if p > 0:
        assert int(ctr[0]) == 1 and int(ctr[1]) == 0
    a1 = c["a1"].to(dev)
    ref, mag = gemm_terms(a1[:M], c["w1"].to(dev), None if not K2 else c["a2"][:M].to(dev), None if not K2 else c["w2"].to(dev), bd)
    if relu:
        ref = torch.relu(ref)
    return dict(out=out.clone(), copy=None if copy is None else copy.clone(), in_norm=in_norm, out_norm=out_norm, ref=ref, mag=mag,
                a1=a1, M=M, n_terms=c["n_terms"])


def _fwd_check(r, what, gather=False):
    from bliss_gnn_amd import nn as bnn
    M, out = r["M"], r["out"]
    ratio = assert_within(out[:M], r["ref"], r["mag"], *dense_k(r["n_terms"]), what + " out")
    assert not bool(out[M:].view(torch.int16).any()), what + ": padding rows of out must be exact zeros"
    assert torch.equal(_bits(r["in_norm"][:M]), _bits(bnn.embed_norm(r["a1"][:M].contiguous()))), what + " in_norm"
    assert torch.equal(_bits(r["out_norm"][:M]), _bits(bnn.embed_norm(out[:M].contiguous()))), what + " out_norm"
    assert not bool(_bits(r["in_norm"][M:]).any()) and not bool(_bits(r["out_norm"][M:]).any()), what + " norms of padding rows"
    if gather:
        assert torch.equal(_bits(r["copy"][:M]), _bits(r["a1"][:M])) and not bool(_bits(r["copy"][M:]).any()), what + " row copy"
    return ratio


# (K, N, M): every K of {1025, 1039, 1040, 1041, 1087, 1088, 1089, 1433, 2047, 2048, 2049, 3073, 16384}, every N of {1, 41, 255, 256}
# and every M of {1, 31, 33, 70} at least once; the Cora input layer's (1433, 256) and (1433, 41)
WIDE_SHAPES = [(1025, 1, 1), (1039, 41, 31), (1040, 255, 33), (1041, 256, 70), (1087, 1, 31), (1088, 41, 33), (1089, 255, 70),
               (1433, 256, 33), (1433, 41, 70), (2047, 255, 1), (2048, 256, 31), (2049, 41, 33), (3073, 256, 70), (16384, 41, 33),
               (16384, 256, 70)]


@pytest.mark.parametrize("K,N,M", WIDE_SHAPES, ids=lambda v: str(v))
def test_wide_single_product_against_fp64(cuda, K, N, M):
    """One product, plain and gathered (repeated and out-of-order ids), with and without bias, with and without ReLU:
    dense_k(K (+ 1)); padding rows exact zeros; in_norm / out_norm bit-equal to embed_norm; a_copy bit-equal to the gathered rows.
    Rows beyond the device-side count are NaN (Inf when gathered), as is the table row the ids beyond the count name."""
    r = {}
    for gather, bias, relu in ((False, True, False), (True, False, True), (True, True, True), (False, False, False)):
        res = _fwd(cuda, K, N, M, gather=gather, bias=bias, relu=relu, pad=INF if gather else NAN)
        r["g%d-b%d-r%d" % (gather, bias, relu)] = _fwd_check(res, "wide fwd %dx%dx%d" % (M, K, N), gather)
    _report("wide-fwd-%d-%d-%d" % (K, N, M), r)


@pytest.mark.parametrize("K1,K2,N,M", [(1433, 1433, 41, 33), (2048, 602, 256, 70)], ids=lambda v: str(v))
def test_wide_dual_product_against_fp64(cuda, K1, K2, N, M):
    """Both products in one accumulator, each walked in its own panels through the one LDS tile: dense_k(K1 + K2 + 1)."""
    r = {}
    for relu in (False, True):
        r["relu%d" % relu] = _fwd_check(_fwd(cuda, K1, N, M, K2=K2, relu=relu), "wide dual %dx(%d+%d)x%d" % (M, K1, K2, N))
    _report("wide-dual-%d-%d-%d-%d" % (K1, K2, N, M), r)


@pytest.mark.parametrize("K", [1025, 1433, 2049, 16384])
def test_wide_seam_probe_is_exact(cuda, K):
    """Row r of A is one-hot at one of the columns 0, 1023, 1024, 1025, K - 1 (and 2047, 2048 for K > 2048): out[r, n] must have
    the BITS of W[n, c] -- a seam column that is dropped gives 0, one staged twice 2 W, one read from panel 0 again another
    column of W -- and with a bias the bits of bf16(float(W[n, c]) + float(b[n]))."""
    from bliss_gnn_amd import nn as bnn
    N, M = 41, 70
    gen = torch.Generator().manual_seed(K)
    a, col = one_hot_rows(K, M)
    w, b = rand(gen, N, K).to(cuda), rand(gen, N).to(cuda)
    ad = a.to(cuda)
    for bias in (None, b):
        out = torch.full((M, N), NAN, dtype=BF, device=cuda)
        _launch("wide", bnn._tg_args(ad, w, out, M, bias=bias))
        torch.cuda.synchronize()
        want = w[:, col.to(cuda)].t()
        if bias is not None:
            want = (want.float() + bias.float()[None, :]).to(BF)
        bad = (_bits(out) != _bits(want)).any(1).nonzero().reshape(-1).tolist()
        assert not bad, "K %d bias %s: rows %s (columns %s) differ" % (K, bias is not None, bad[:8], [int(col[r]) for r in bad[:8]])


@pytest.mark.parametrize("K1,K2,N,M", [(602, 0, 256, 70), (1024, 0, 41, 33), (256, 256, 256, 70)], ids=lambda v: str(v))
def test_one_panel_is_the_narrow_kernel(cuda, K1, K2, N, M):
    """At K <= 1024 the wide entry point runs one panel per operand: every output has the bits of bliss_tile_gemm on the same
    arguments -- out, in_norm, out_norm, a_copy, the zero rows; the dual product with ReLU and dropout p = 0.25 from equal fresh
    counters."""
    kw = dict(K2=K2, gather=not K2, relu=bool(K2), p=0.25 if K2 else 0.0)
    narrow, wide = _fwd(cuda, K1, N, M, entry="tile", **kw), _fwd(cuda, K1, N, M, entry="wide", **kw)
    for name in ("out", "in_norm", "out_norm") + (("copy",) if not K2 else ()):
        assert torch.equal(_bits(wide[name]), _bits(narrow[name])), "%s of the wide entry point differs from bliss_tile_gemm's" % name
    if not K2:
        _report("wide-one-panel-%d-%d-%d" % (K1, N, M), {"out": _fwd_check(wide, "one panel", True)})


@pytest.mark.parametrize("K1,K2,N,M,gather", [(1434, 0, 64, 45, True), (2048, 1100, 32, 33, False)])
def test_wide_alignment_does_not_change_a_bit(cuda, K1, K2, N, M, gather):
    """Each operand in turn, then all together, as a misaligned window against the aligned run of the same numbers (in which
    every panel takes its fast paths: K, N even, aligned pointers): every output bit equal, the aligned run inside the bound."""
    base = _fwd(cuda, K1, N, M, K2=K2, gather=gather)
    ratio = _fwd_check(base, "wide aligned", gather)
    which = ["a1", "w1", "out"] + (["a2", "w2"] if K2 else []) + (["copy"] if gather else [])
    for v in which + [tuple(which)]:
        got = _fwd(cuda, K1, N, M, K2=K2, gather=gather, views=v if isinstance(v, tuple) else (v,))
        for name in ("out", "in_norm", "out_norm") + (("copy",) if gather else ()):
            assert torch.equal(_bits(got[name]), _bits(base[name])), "%s differs with %s misaligned" % (name, v)
    _report("wide-align-%d-%d-%d-%d-g%d" % (K1, K2, N, M, gather), {"out": ratio})


def test_wide_pair_launch(cuda):
    """Two argument sets in one launch (blockIdx.y) at the Cora width: fc_neigh over 70 source rows (67 live), fc_self (+ bias)
    over the first 33 of them (1 live); the second set has fewer tiles than the grid."""
    from bliss_gnn_amd import nn as bnn
    F, N, n_src, n_dst, src_cnt, dst_cnt = 1433, 41, 70, 33, 67, 1
    gen = torch.Generator().manual_seed(F + n_src)
    x = rand(gen, n_src, F)
    x[src_cnt:] = NAN
    wn, ws, b = rand(gen, N, F, scale=F ** -0.5).to(cuda), rand(gen, N, F, scale=F ** -0.5).to(cuda), rand(gen, N).to(cuda)
    xd = x.to(cuda)
    z = torch.full((n_src, N), NAN, dtype=BF, device=cuda)
    y = torch.full((n_dst, N), NAN, dtype=BF, device=cuda)
    norm = torch.full((n_src,), NAN, dtype=BF, device=cuda)
    cnt = torch.tensor([src_cnt, dst_cnt], dtype=torch.int32, device=cuda)
    _launch("wide", bnn._tg_args(xd, wn, z, n_src, m_dev=cnt.data_ptr(), in_norm=norm),
            bnn._tg_args(xd, ws, y, n_dst, bias=b, m_dev=cnt.data_ptr() + 4))
    torch.cuda.synchronize()
    rz, mz = gemm_terms(xd[:src_cnt], wn)
    ry, my = gemm_terms(xd[:dst_cnt], ws, bias=b)
    r = {"z": assert_within(z[:src_cnt], rz, mz, *dense_k(F), "pair z"), "y": assert_within(y[:dst_cnt], ry, my, *dense_k(F + 1), "pair y")}
    assert not bool(_bits(z[src_cnt:]).any()) and not bool(_bits(y[dst_cnt:]).any()) and not bool(_bits(norm[src_cnt:]).any())
    assert torch.equal(_bits(norm[:src_cnt]), _bits(bnn.embed_norm(xd[:src_cnt].contiguous())))
    _report("wide-pair-%d-%d-%d-%d" % (F, N, n_src, n_dst), r)


def test_wide_dropout(cuda):
    """p = 0.25 at (1433, 41, 70): the keep mask is recovered from the output; kept elements are held to ref / (1 - p) with one
    more stored rounding (k_mag + 1), dropped ones are exact zeros, and of the elements that are further than their bound above
    zero a share p +- 0.02 is dropped."""
    K1, N, M, p = 1433, 41, 70, 0.25
    res = _fwd(cuda, K1, N, M, relu=True, p=p)
    out, ref, mag = res["out"][:M], res["ref"], res["mag"]
    kept = out > 0
    k = dense_k(res["n_terms"], stored=1.0)
    ratio = assert_within(out, ref * kept / (1 - p), mag * kept / (1 - p), *k, "wide dropout out")
    assert not bool(_bits(res["out"][M:]).any())
    clear = ref > 2 * (ulp_bf16(ref) + k[1] * 2.0 ** -8 * mag)
    share = 1.0 - float((kept & clear).sum()) / float(clear.sum())
    print("SHARE wide-dropout %.4f" % share)
    assert abs(share - p) < 0.02, share
    _report("wide-dropout-%d-%d-%d" % (K1, N, M), {"out": ratio})
