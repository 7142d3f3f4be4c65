"""GPU suite: the three hand-written MFMA kernels of the SAGE layers -- k_tile_gemm (csrc/sage.hip), k_dgrad and k_wgrad +
k_wgrad_reduce (csrc/sage_bwd.hip) -- and the four autograd nodes of nn.py that drive them, element by element against
float64 on the same bf16 operands, at the shapes where such kernels go wrong, with the bound of tests/bounds.py:

    |got - ref| <= k_ulp * ulp_bf16(ref) + k_mag * 2^-8 * mag,     mag = the reference on absolute values, per element.

Constants (derived from where the kernels round; tests/test_bounds.py shows on the CPU what they catch):
  forward, dgrad   bounds.dense_k(K1 + K2 (+ 1 with a bias)) = (1, n * 2^-16): fp32 accumulation of n terms (n roundings of
                   relative size 2^-24 = n * 2^-16 in units of 2^-8 of the magnitude), ONE rounding to bf16 (half a spacing
                   of the fp32 sum, which may lie one binade above ref: k_ulp 1).
  forward dropout  one more stored rounding, t = rbf(acc + b) before rbf(t / (1 - p)): k_mag + 1, on ref / (1 - p).
  wgrad            bounds.dense_k(rows + chunks): per chunk an fp32 sum over its rows, the chunks summed in fp32 in order.
  layers           bounds.sage_layer_k: + 1 per bf16 value stored between launches on the path (Z, agg, dZ / T; an SpMM result
                   1.25 with its own fp32 sum), + 1 per dropout multiply, magnitudes through the GEMMs and the SpMM.
Every operand row beyond the device-side count is NaN (one case each: +Inf), every output that the caller allocates is
pre-filled with NaN: the valid results must not see them and the padding rows must come out as exact zeros.  A misaligned
operand is a column window base[:, 1:1 + cols] of a wider NaN buffer with an odd row stride (2-byte aligned, odd stride): it
must give the bits of the aligned run.  Every test prints ``RATIO <case> <tensor> <largest |got - ref| / bound>`` (pytest -s)
for the margin table of DESIGN.md 3."""
import json
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":                                   # the BLISS_WGRAD_WGS child (see the end of the file)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bounds import (WGRAD_LOUD_CASES, assert_within, dense_k, dgrad_terms, edge_shape_spec, gemm_terms, many_hubs_spec, padded_block,
                    row_count_spec, sage_layer_k, sage_layer_terms, to_block, ulp_bf16, wgrad_inputs, wgrad_loud_rows, wgrad_plan, wgrad_terms)

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
BF = torch.bfloat16


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
    """The buffer around a window still holds its NaN fill: nothing was written beside the rows."""
    return bool(torch.isnan(base[:, 0]).all()) and bool(torch.isnan(base[:, 1 + cols:]).all())


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


# ------------------------------------------------------------------------------------------------ forward: k_tile_gemm
def _fwd(dev, K1, N, M, K2=0, gather=False, bias=True, relu=False, views=(), pad=NAN, p=0.0, extra=40, seed=0):
    """One launch: out = epilogue(A1 W1^T (+ A2 W2^T) + bias) on m_bound = M + extra rows of which M exist (device-side count).
    Returns the outputs, the fp64 reference and its magnitude."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(1000 * K1 + 10 * N + M + seed)
    mb = M + extra
    T = 300
    if gather:
        table = _rand(gen, T, K1)
        table[T - 1] = pad                                   # the row the ids beyond the count point at: never loaded
        ids = torch.randint(0, T - 1, (mb,), generator=gen)
        ids[: min(M, 8)] = ids[0]                            # repeated ids; random ids are out of order anyway
        ids[M:] = T - 1
        a1 = table[ids]
    else:
        a1 = _rand(gen, mb, K1)
    a1[M:] = pad
    w1 = _rand(gen, N, K1, scale=K1 ** -0.5)
    a2 = w2 = None
    if K2:
        a2, w2 = _rand(gen, mb, K2), _rand(gen, N, K2, scale=K2 ** -0.5)
        a2[M:] = pad
    b = _rand(gen, N) if bias else None
    src1, _ = _place(table if gather else a1, dev, "a1" in views)
    w1d, _ = _place(w1, dev, "w1" in views)
    a2d = w2d = None
    if K2:
        a2d, _ = _place(a2, dev, "a2" in views)
        w2d, _ = _place(w2, dev, "w2" in views)
    out, out_base = _place(torch.full((mb, N), NAN, dtype=BF), dev, "out" in views)
    copy, copy_base = _place(torch.full((mb, K1), NAN, dtype=BF), dev, "copy" in views) if gather else (None, None)
    in_norm = torch.full((mb,), NAN, dtype=BF, device=dev)
    out_norm = torch.full((mb,), NAN, dtype=BF, device=dev)
    m_dev = torch.tensor([M], dtype=torch.int32, device=dev)
    ctr = torch.zeros(66, dtype=torch.int64, device=dev) if p > 0 else None
    bd = None if b is None else b.to(dev)
    bnn._tile_gemm(bnn._tg_args(src1, w1d, out, mb, ids=ids.to(torch.int32).to(dev) if gather else None, a2=a2d, w2=w2d, bias=bd,
                                m_dev=m_dev.data_ptr(), a_copy=copy, in_norm=in_norm, out_norm=out_norm, relu=relu, p=p, seed=77, ctr=ctr))
    torch.cuda.synchronize()
    if out_base is not None:
        assert _frame_untouched(out_base, N), "written beside the output rows"
    if copy_base is not None:
        assert _frame_untouched(copy_base, K1), "written beside the copied rows"
    if p > 0:
        assert int(ctr[0]) == 1 and int(ctr[1]) == 0
    ref, mag = gemm_terms(a1[:M].to(dev), w1.to(dev), None if a2 is None else a2[:M].to(dev), None if w2 is None else w2.to(dev), bd)
    if relu:
        ref = torch.relu(ref)
    return dict(out=out.clone(), copy=None if copy is None else copy.clone(), in_norm=in_norm, out_norm=out_norm, ref=ref, mag=mag,
                a1=a1.to(dev), M=M, n_terms=K1 + K2 + (1 if bias else 0))


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


# (K, N, M): every K of {1, 7, 16, 63, 64, 65, 602, 1024}, every N of {1, 3, 31, 32, 33, 41, 255, 256}, every M of {1, 31, 32, 33,
# 777} at least once, and the models' (602, 256), (602, 41), (256, 256), (1024, 256)
FWD_SHAPES = [(1, 1, 1), (7, 3, 31), (16, 31, 32), (63, 32, 33), (64, 33, 777), (65, 41, 31), (602, 255, 33), (1024, 256, 32),
              (602, 256, 777), (602, 41, 777), (256, 256, 777), (1024, 256, 33), (1, 256, 33), (1024, 1, 31), (16, 256, 1)]


@pytest.mark.parametrize("K,N,M", FWD_SHAPES, ids=lambda v: str(v))
def test_tile_gemm_single_product_edges(cuda, K, N, M):
    """One product at every edge of K (the k tail of the MFMA step, of the 64-slab, K < 16), N (column tail inside and at the
    edge of a wave's 32 columns) and M (row tail, one row), plain and gathered (repeated and out-of-order ids), with and
    without bias, with and without ReLU: dense_k(K (+ 1)).  Rows beyond the device-side count are NaN (Inf when gathered),
    as is the table row the ids beyond the count name."""
    r = {}
    for gather, bias, relu in ((False, True, False), (True, False, True), (True, True, True)):
        res = _fwd(cuda, K, N, M, gather=gather, bias=bias, relu=relu, pad=INF if gather else NAN)
        r["g%d-b%d-r%d" % (gather, bias, relu)] = _fwd_check(res, "fwd %dx%dx%d" % (M, K, N), gather)
    _report("fwd-%d-%d-%d" % (K, N, M), r)


@pytest.mark.parametrize("K1,K2,N,M", [(256, 256, 256, 777), (602, 256, 256, 33), (16, 48, 48, 31), (1024, 63, 41, 32), (7, 65, 255, 1),
                                       (200, 72, 64, 70)], ids=lambda v: str(v))
def test_tile_gemm_dual_product_edges(cuda, K1, K2, N, M):
    """Both products in one accumulator with K1 != K2 (and the layers' 256 + 256): dense_k(K1 + K2 + 1)."""
    r = {}
    for relu in (False, True):
        r["relu%d" % relu] = _fwd_check(_fwd(cuda, K1, N, M, K2=K2, relu=relu), "dual %dx(%d+%d)x%d" % (M, K1, K2, N))
    _report("dual-%d-%d-%d-%d" % (K1, K2, N, M), r)


@pytest.mark.parametrize("K1,K2,N,M,gather", [(200, 72, 64, 70, False), (200, 72, 64, 70, True), (602, 0, 256, 45, True), (64, 128, 32, 33, False)])
def test_tile_gemm_alignment_does_not_change_a_bit(cuda, K1, K2, N, M, gather):
    """Each operand in turn as a misaligned window (A1 or the gathered table: `even` false; the row copy: `copy32` false; W1,
    W2: the element-wise slab path for every slab instead of K / 64 full ones; the output: `pair_ok` false; A2: `even` false
    for the second product) against the aligned run of the same numbers, in which all of them are true (K, N even, K >= 64):
    every output bit equal, and the aligned run inside the bound."""
    base = _fwd(cuda, K1, N, M, K2=K2, gather=gather)
    ratio = _fwd_check(base, "aligned", gather)
    which = ["a1", "w1", "out"] + (["a2", "w2"] if K2 else []) + (["copy"] if gather else [])
    for v in which + [tuple(which)]:
        got = _fwd(cuda, K1, N, M, K2=K2, gather=gather, views=v if isinstance(v, tuple) else (v,))
        for name in ("out", "in_norm", "out_norm") + (("copy",) if gather else ()):
            assert torch.equal(_bits(got[name]), _bits(base[name])), "%s differs with %s misaligned" % (name, v)
    _report("align-%d-%d-%d-%d-g%d" % (K1, K2, N, M, gather), {"out": ratio})


@pytest.mark.parametrize("K1,K2,N,M", [(256, 256, 256, 777), (602, 0, 41, 333)])
def test_tile_gemm_dropout(cuda, K1, K2, N, M):
    """p = 0.25: the keep mask is recovered from the output (as test_sage_epilogue_kernel does); kept elements are held to
    ref / (1 - p) with one more stored rounding (k_mag + 1), dropped ones are exact zeros, and of the elements that are
    further than their bound above zero a share p +- 0.02 is dropped."""
    p = 0.25
    res = _fwd(cuda, K1, N, M, K2=K2, relu=True, p=p)
    out, ref, mag = res["out"][:M], res["ref"], res["mag"]
    kept = out > 0
    k = dense_k(res["n_terms"], stored=1.0)
    ratio = assert_within(out, ref * kept / (1 - p), mag * kept / (1 - p), *k, "dropout out")
    assert not bool(_bits(res["out"][M:]).any())
    clear = ref > 2 * (ulp_bf16(ref) + k[1] * 2.0 ** -8 * mag)
    share = 1.0 - float((kept & clear).sum()) / float(clear.sum())
    assert abs(share - p) < 0.02, share
    _report("dropout-%d-%d-%d-%d" % (K1, K2, N, M), {"out": ratio})


@pytest.mark.parametrize("F,N,n_src,n_dst,src_cnt,dst_cnt", [(602, 256, 500, 120, 500, 120), (602, 256, 500, 150, 470, 101),
                                                              (256, 41, 333, 33, 300, 32), (48, 16, 70, 65, 67, 1)])
def test_tile_gemm_pair_launch(cuda, F, N, n_src, n_dst, src_cnt, dst_cnt):
    """Two argument sets in one launch (blockIdx.y): fc_neigh over the source rows, fc_self (+ bias) over the first n_dst of
    them, n_dst < n_src ending inside a tile, each with its own device-side count; the second set has fewer tiles than the
    grid."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(F + n_src)
    x = _rand(gen, n_src, F)
    x[src_cnt:] = NAN
    wn, ws, b = _rand(gen, N, F, scale=F ** -0.5).to(cuda), _rand(gen, N, F, scale=F ** -0.5).to(cuda), _rand(gen, N).to(cuda)
    xd = x.to(cuda)
    z = torch.full((n_src, N), NAN, dtype=BF, device=cuda)
    y = torch.full((n_dst, N), NAN, dtype=BF, device=cuda)
    norm = torch.full((n_src,), NAN, dtype=BF, device=cuda)
    cnt = torch.tensor([src_cnt, dst_cnt], dtype=torch.int32, device=cuda)
    bnn._tile_gemm(bnn._tg_args(xd, wn, z, n_src, m_dev=cnt.data_ptr(), in_norm=norm),
                   bnn._tg_args(xd, ws, y, n_dst, bias=b, m_dev=cnt.data_ptr() + 4))
    torch.cuda.synchronize()
    rz, mz = gemm_terms(xd[:src_cnt], wn)
    ry, my = gemm_terms(xd[:dst_cnt], ws, bias=b)
    r = {"z": assert_within(z[:src_cnt], rz, mz, *dense_k(F), "pair z"), "y": assert_within(y[:dst_cnt], ry, my, *dense_k(F + 1), "pair y")}
    assert not bool(_bits(z[src_cnt:]).any()) and not bool(_bits(y[dst_cnt:]).any()) and not bool(_bits(norm[src_cnt:]).any())
    assert torch.equal(_bits(norm[:src_cnt]), _bits(bnn.embed_norm(xd[:src_cnt].contiguous())))
    _report("pair-%d-%d-%d-%d" % (F, N, n_src, n_dst), r)


# ------------------------------------------------------------------------------------------------ dgrad: k_dgrad
def _dgrad(dev, M, mb, K1, N, K2=0, M2=0, m2b=0, views=(), pad=NAN, seed=0):
    """out = A1 W1 (+ A2 W2 on rows < min(M2, M)); M, M2 are the device-side counts, mb, m2b the bounds."""
    from bliss_gnn_amd.nn import sage_dgrad
    gen = torch.Generator().manual_seed(1000 * K1 + 10 * N + M + seed)
    a1, w1 = _rand(gen, mb, K1, scale=0.1), _rand(gen, K1, N, scale=0.2)
    a1[M:] = pad
    a1d, _ = _place(a1, dev, "a1" in views)
    w1d, _ = _place(w1, dev, "w1" in views)
    a2 = w2 = a2d = w2d = None
    if K2:
        a2, w2 = _rand(gen, m2b, K2, scale=0.1), _rand(gen, K2, N, scale=0.2)
        a2[M2:] = pad
        a2d, _ = _place(a2, dev, "a2" in views)
        w2d, _ = _place(w2, dev, "w2" in views)
    cnt = torch.tensor([M, M2], dtype=torch.int32, device=dev)
    out = sage_dgrad(a1d, w1d, mb, cnt.data_ptr(), a2=a2d, w2=w2d, m2_bound=m2b, m2_dev=cnt.data_ptr() + 4 if K2 else 0)
    torch.cuda.synchronize()
    m2 = min(M2, M)
    ref, mag = dgrad_terms(a1[:M].to(dev), w1.to(dev), None if not K2 else torch.nan_to_num(a2).to(dev), None if not K2 else w2.to(dev),
                           m2=m2 if K2 else None)
    return out, ref, mag


# (M, m_bound, K1, K2, N, M2 on the device, m2_bound): K1, K2 over {1, 7, 15, 16, 17, 63, 64, 65, 200, 256}, N over {1, 3, 255, 256,
# 257, 601, 602}, M2 over {0, 1, 31, 32, 33, M}; the cut of m_dev inside a tile and on a tile edge; m2_dev > m_dev
DGRAD_CASES = [(33, 70, 1, 0, 1, 0, 0), (70, 100, 7, 15, 3, 1, 40), (64, 96, 16, 17, 255, 31, 64), (77, 130, 63, 64, 256, 32, 40),
               (100, 140, 65, 200, 257, 33, 50), (130, 160, 256, 256, 601, 130, 160), (45, 64, 200, 1, 602, 45, 64),
               (50, 90, 17, 63, 601, 60, 64), (32, 33, 15, 7, 257, 40, 48), (3300, 3333, 256, 256, 257, 1300, 1400), (1, 1, 256, 0, 601, 0, 0)]


@pytest.mark.parametrize("M,mb,K1,K2,N,M2,m2b", DGRAD_CASES, ids=lambda v: str(v))
def test_dgrad_edges(cuda, M, mb, K1, K2, N, M2, m2b):
    """dense_k(K1 + K2).  Odd N above 256 (the element-wise store in a second blockIdx.y tile), the second product ending
    inside a tile, on a tile edge and beyond the first product's rows (the M2 > M clamp), K1 / K2 off the MFMA step and
    the 64-row W slab together with a ragged N; rows in [m_dev, m_bound) are exact zeros; rows of A1 / A2 beyond the
    device-side counts are NaN."""
    out, ref, mag = _dgrad(cuda, M, mb, K1, N, K2, M2, m2b)
    ratio = assert_within(out[:M], ref, mag, *dense_k(K1 + K2), "dgrad")
    assert out.shape == (mb, N) and not bool(_bits(out[M:]).any()), "rows beyond the count must be exact zeros"
    _report("dgrad-%d-%d-%d-%d-%d" % (M, K1, K2, N, M2), {"out": ratio})


@pytest.mark.parametrize("M,mb,K1,K2,N,M2,m2b", [(77, 130, 200, 64, 256, 33, 40), (77, 130, 65, 17, 601, 33, 40), (45, 64, 256, 256, 602, 45, 64)])
def test_dgrad_alignment_does_not_change_a_bit(cuda, M, mb, K1, K2, N, M2, m2b):
    """a1, a2, w1, w2 as misaligned windows (ld8_masked(..., aligned=false) for the rows and for the W slabs) against the
    aligned run; +Inf instead of NaN beyond the counts."""
    base, ref, mag = _dgrad(cuda, M, mb, K1, N, K2, M2, m2b, pad=INF)
    ratio = assert_within(base[:M], ref, mag, *dense_k(K1 + K2), "dgrad aligned")
    for v in ("a1", "a2", "w1", "w2", ("a1", "a2", "w1", "w2")):
        got, _, _ = _dgrad(cuda, M, mb, K1, N, K2, M2, m2b, views=v if isinstance(v, tuple) else (v,), pad=INF)
        assert torch.equal(_bits(got), _bits(base)), "dgrad differs with %s misaligned" % (v,)
    _report("dgrad-align-%d-%d-%d" % (K1, K2, N), {"out": ratio})


# ------------------------------------------------------------------------------------------------ wgrad: k_wgrad + k_wgrad_reduce
def _workspace(problems):
    """bliss_sage_wgrad_workspace for [(rows_bound, n_out, k_in)]: the chunk plan as the library made it (floats)."""
    from bliss_gnn_amd import _lib
    arr = (_lib.WGrad * len(problems))()
    for a, (rb, n_out, k_in) in zip(arr, problems):
        a.d, a.x, a.dw = 256, 256, 256                       # (only checked for null)
        a.d_stride, a.n_out, a.x_stride, a.k_in, a.rows_bound, a.dw_stride = n_out, n_out, k_in, k_in, rb, k_in
    return int(_lib.lib.bliss_sage_wgrad_workspace(arr, len(problems)))


def _wgrad(dev, probs, target=80, views=(), pad=NAN, seed=0, loud=False):
    """probs: [(rows_bound, rows on the device, n_out, k_in, want_bias)].  Runs the launch pair twice (bit-equal), checks every
    dW / db against fp64 with dense_k(rows + chunks) of the plan computed here from the documented rule, and the library's
    workspace against that plan.  Returns the ratios."""
    from bliss_gnn_amd.nn import sage_wgrad
    plan, floats = wgrad_plan([(rb, k) for rb, _, _, k, _ in probs], target)
    assert _workspace([(rb, n, k) for rb, _, n, k, _ in probs]) == floats, "the library planned other chunks than %s" % (plan,)
    cnt = torch.tensor([r for _, r, _, _, _ in probs], dtype=torch.int32, device=dev)
    args, keep = [], []
    for i, ((rb, rows, n_out, k_in, wb), (chunks, rpc)) in enumerate(zip(probs, plan)):
        ids = wgrad_loud_rows(rows, chunks, rpc) if loud else None
        d, x = wgrad_inputs(rb, n_out, k_in, 91 + seed + 7 * i, rows=rows, loud=ids, pad=pad)
        dd, _ = _place(d, dev, "d" in views)
        xd, _ = _place(x, dev, "x" in views)
        keep.append((d, x))
        args.append((dd, xd, rb, cnt.data_ptr() + 4 * i, wb))
    o1 = sage_wgrad(args)
    o2 = sage_wgrad(args)
    torch.cuda.synchronize()
    r, outs = {}, []
    for i, ((rb, rows, n_out, k_in, wb), (chunks, rpc), (d, x)) in enumerate(zip(probs, plan, keep)):
        (dw, db), (dw2, db2) = o1[i], o2[i]
        assert torch.equal(_bits(dw), _bits(dw2)) and (db is None or torch.equal(_bits(db), _bits(db2))), "not reproducible"
        rw, mw, rbias, mb_ = wgrad_terms(d.to(dev), x.to(dev), rows)
        k = dense_k(rows + chunks)
        r["dW%d" % i] = assert_within(dw, rw, mw, *k, "wgrad dW%d %s plan %s" % (i, probs[i], plan[i]))
        assert (db is not None) == bool(wb)
        if wb:
            r["db%d" % i] = assert_within(db, rbias, mb_, *k, "wgrad db%d %s plan %s" % (i, probs[i], plan[i]))
        outs.append((dw, db))
    return r, plan, outs


def _wid(case):
    probs = case[0]
    plan, _ = wgrad_plan([(rb, k) for rb, _, _, k, _ in probs])
    return "+".join("%dof%dx%dx%d%s-plan%dx%d" % (r, rb, n, k, "b" if wb else "", c, rpc) for (rb, r, n, k, wb), (c, rpc) in zip(probs, plan))


# one problem: (rows_bound, rows, n_out, k_in, want_bias); the plan (chunks x rows_per_chunk) is in the id
WGRAD_SINGLE = [
    ([(1, 1, 1, 1, True)],), ([(33, 33, 7, 5, True)],), ([(64, 64, 41, 127, False)],), ([(64, 1, 256, 128, True)],),      # one chunk
    ([(65, 65, 255, 128, True)],), ([(130, 130, 256, 128, True)],), ([(640, 640, 41, 128, True)],),                       # the ceil(rows / 64) cap
    ([(640, 65, 41, 128, True)],), ([(640, 64, 7, 128, True)],),                                                           # one row into chunk 2; chunk 1 only
    ([(5120, 5120, 256, 128, True)],), ([(5200, 5200, 255, 127, True)],), ([(5200, 520, 41, 5, True)],),                   # the full 80 chunks
    ([(5200, 5190, 256, 129, True)],),                                                                                     # two column tiles: 40 chunks
    ([(3000, 3000, 256, 602, True)],), ([(3000, 2881, 41, 602, True)],), ([(3000, 300, 256, 602, False)],),                # 16 chunks, ragged last
    ([(3000, 1, 256, 602, True)],), ([(3000, 193, 1, 602, True)],),                                                        # count 1; one row into chunk 2
]
WGRAD_PAIRS = [
    ([(3000, 3000, 256, 602, False), (1200, 1200, 256, 602, True)],), ([(3000, 300, 256, 602, True), (1200, 1177, 256, 602, False)],),
    ([(3000, 2999, 256, 602, False), (1200, 120, 256, 602, True)],), ([(3000, 3000, 256, 602, False), (3000, 2000, 256, 256, True)],),
    ([(3000, 300, 256, 602, True), (3000, 300, 256, 256, True)],), ([(2000, 1999, 41, 256, False), (500, 1, 41, 256, True)],),
    ([(2100, 2100, 256, 256, False), (2100, 210, 256, 256, True)],), ([(70, 70, 7, 129, True), (33, 3, 7, 1, True)],),
]


@pytest.mark.parametrize("case", WGRAD_SINGLE + WGRAD_PAIRS, ids=_wid)
def test_wgrad_plans_and_counts(cuda, case):
    """Every branch of wgrad_plan -- one chunk, the ceil(rows_bound / 64) cap, the full 80 chunks, 16 chunks of a 602-wide
    input alone, two problems sharing the 80 (different k_in: 80 / tiles_all), a ragged last chunk after rows_per_chunk is
    rounded up to 32 -- with the device-side count at the bound, at 1, one row into the second chunk and at a tenth of the
    bound (most chunks hold no row: k_wgrad returns, k_wgrad_reduce sums only the chunks that hold rows), independently
    on both problems of a pair; n_out over {1, 7, 41, 255, 256}, k_in over {1, 5, 127, 128, 129, 602}; bias on either problem.
    Rows beyond the count are NaN.  dense_k(rows + chunks)."""
    r, plan, _ = _wgrad(cuda, case[0])
    _report("wgrad-" + _wid(case), r)


@pytest.mark.parametrize("probs", [[(640, 601, 41, 128, True)], [(3000, 2881, 256, 602, True), (1200, 1177, 255, 129, True)]],
                         ids=lambda p: "+".join("%dx%dx%d" % (r, n, k) for _, r, n, k, _ in p))
def test_wgrad_alignment_does_not_change_a_bit(cuda, probs):
    """d and x as misaligned windows (ld8_masked(..., aligned=false) in wg_load) against the aligned run; +Inf beyond the counts."""
    r, _, base = _wgrad(cuda, probs, pad=INF)
    for v in (("d",), ("x",), ("d", "x")):
        _, _, got = _wgrad(cuda, probs, views=v, pad=INF)
        for (dw, db), (gw, gb) in zip(base, got):
            assert torch.equal(_bits(dw), _bits(gw)) and torch.equal(_bits(db), _bits(gb)), "wgrad differs with %s misaligned" % (v,)
    _report("wgrad-align", r)


@pytest.mark.parametrize("rows_bound,rows,n_out,k_in", WGRAD_LOUD_CASES)
def test_wgrad_loud_rows(cuda, rows_bound, rows, n_out, k_in):
    """The input layer's weight gradient at full size with loud rows (bounds.wgrad_loud_rows: the last row of every chunk,
    the first of the next, the last valid row carry 64x the gradient): tests/test_bounds.py shows on these inputs that losing
    any one of them fails the bound, which one ordinary row out of 11 000 would not."""
    r, plan, _ = _wgrad(cuda, [(rows_bound, rows, n_out, k_in, True)], loud=True)
    _report("wgrad-loud-%d-plan%dx%d" % (rows_bound, *plan[0]), r)


# ---- BLISS_WGRAD_WGS: read once per process (a function-local static), so every target runs in a child process of its own
WGS_CASE = (5000, 4877, 256, 602)
WGS_TARGETS = (1, 37, 448)


def _wgs_loud():
    rb, rows, _, k_in = WGS_CASE
    ids = set()
    for t in WGS_TARGETS + (80,):
        (chunks, rpc), = wgrad_plan([(rb, k_in)], t)[0]
        ids.update(wgrad_loud_rows(rows, chunks, rpc))
    return sorted(ids)


def _wgs_child(target):
    """In the child: the weight gradient of WGS_CASE (the same inputs for every target: loud rows at every target's chunk
    boundaries) under the BLISS_WGRAD_WGS of the environment; prints one JSON line."""
    from bliss_gnn_amd.nn import sage_wgrad
    dev = torch.device("cuda:0")
    rb, rows, n_out, k_in = WGS_CASE
    d, x = wgrad_inputs(rb, n_out, k_in, 17, rows=rows, loud=_wgs_loud())
    (chunks, rpc), = wgrad_plan([(rb, k_in)], target)[0]
    floats = _workspace([(rb, n_out, k_in)])
    cnt = torch.tensor([rows], dtype=torch.int32, device=dev)
    (dw, db), = sage_wgrad([(d.to(dev), x.to(dev), rb, cnt.data_ptr(), True)])
    (dw2, db2), = sage_wgrad([(d.to(dev), x.to(dev), rb, cnt.data_ptr(), True)])
    torch.cuda.synchronize()
    rw, mw, rbias, mb_ = wgrad_terms(d.to(dev), x.to(dev), rows)
    k = dense_k(rows + chunks)
    out = dict(target=target, floats=floats, chunks=floats // (256 * (-(-k_in // 128) * 128 + 4)), rows_per_chunk=rpc,
               same=bool(torch.equal(_bits(dw), _bits(dw2)) and torch.equal(_bits(db), _bits(db2))),
               dW=assert_within(dw, rw, mw, *k, "dW"), db=assert_within(db, rbias, mb_, *k, "db"),
               sum_bits=int(_bits(dw).long().sum()))
    print("WGS " + json.dumps(out))


def test_wgrad_target_from_the_environment_in_child_processes(cuda):
    """BLISS_WGRAD_WGS = 1, 37, 448, each in a fresh child process started with the variable in its environment (one at a time,
    a timeout each, no further child after one that failed): the library plans the chunks the documented rule gives for that
    target (1 x 5024, 7 x 736, 79 x 64 for 5000 x 602), and every target's dW and db are within dense_k(rows + chunks) of the
    same fp64 reference on the same loud-row inputs."""
    r, plans = {}, set()
    for t in WGS_TARGETS:
        env = dict(os.environ, BLISS_WGRAD_WGS=str(t))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--wgs-child", str(t)], env=env, capture_output=True, text=True,
                             timeout=300)
        assert res.returncode == 0, "child for target %d: exit %d\n%s\n%s" % (t, res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        line = [l for l in res.stdout.splitlines() if l.startswith("WGS ")]
        assert len(line) == 1, res.stdout[-2000:]
        o = json.loads(line[0][4:])
        (chunks, rpc), = wgrad_plan([(WGS_CASE[0], WGS_CASE[3])], t)[0]
        assert (o["chunks"], o["rows_per_chunk"]) == (chunks, rpc) and o["same"], o
        assert o["dW"] <= 1 and o["db"] <= 1
        plans.add((chunks, rpc))
        r["dW-wgs%d-plan%dx%d" % (t, chunks, rpc)], r["db-wgs%d" % t] = o["dW"], o["db"]
    assert plans == {(1, 5024), (7, 736), (79, 64)}
    _report("wgrad-env", r)


# ------------------------------------------------------------------------------------------------ the four autograd nodes
_SPECS = {}


def _spec(name):
    if name not in _SPECS:
        _SPECS[name] = {"edge": edge_shape_spec, "hubs": many_hubs_spec, "r16384": lambda: row_count_spec(16384),
                        "r16385": lambda: row_count_spec(16385)}[name]()
    return _SPECS[name]


def _run_layer(dev, spec, blk, padded, node, fin, fout, relu, p, bias, gather, seed, mfma_bwd=True):
    """One SAGE layer through ``node`` the way model.py / shard_static.py chain it; returns the kernel's tensors and the
    operands for the reference."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(seed)
    S, K = spec.S, spec.K
    Sb, Kb, Bb = blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()
    cd = blk._counts_dev.data_ptr() if padded else 0
    src_dev, dst_dev = (cd + 12, cd) if padded else (0, 0)
    leaf = lambda t: t.to(dev).requires_grad_(True)
    h = _rand(gen, Kb, fin)
    h[K:] = NAN
    wn, ws = leaf(_rand(gen, fout, fin, scale=fin ** -0.5)), leaf(_rand(gen, fout, fin, scale=fin ** -0.5))
    b = leaf(_rand(gen, fout)) if bias else None
    ew = (torch.rand(Bb, generator=gen) + 0.05).to(BF).to(dev)
    g = _rand(gen, Sb, fout)
    g[S:] = NAN
    g = g.to(dev)
    ctr = torch.zeros(66, dtype=torch.int64, device=dev) if p > 0 else None
    two = node in ("split", "dual")
    h_dst = ids = hd_ref = None
    if two and not gather:
        h_dst = _rand(gen, Sb, fin)
        h_dst[S:] = NAN
        h_dst = leaf(h_dst)
        hd_ref = h_dst.detach()[:S]
    if gather:
        ids = torch.zeros(Sb if node == "split" else Kb, dtype=torch.int64)
        if node == "split":                                  # destinations anywhere among the source rows
            ids[:S] = torch.randperm(K, generator=gen)[:S]
        else:                                                # pair: the block's source rows out of a table, repeated ids
            T = K + 50
            ids[:K] = torch.randint(0, T, (K,), generator=gen)
        ids = ids.to(torch.int32).to(dev)
    if node == "pair" and gather:
        table = leaf(_rand(gen, T, fin))
        h_ref = table.detach()[ids.long()][:K]
        z, y, rows, _ = bnn._SageLinearPair.apply(table, ids, wn, ws, b, Kb, Sb, src_dev, dst_dev)
        assert torch.equal(_bits(rows[:K]), _bits(h_ref)) and not bool(_bits(rows[K:]).any())
        h = table
    else:
        h = leaf(h)
        h_ref = h.detach()[:K]
    if node == "pair" and not gather:
        z, y, _, _ = bnn._SageLinearPair.apply(h, None, wn, ws, b, Kb, Sb, src_dev, dst_dev)
    elif node == "split":
        z, y, _ = bnn._SageLinearSplit.apply(h, h_dst, wn, ws, b, src_dev, dst_dev, ids)
        if gather:
            hd_ref = h_ref[ids.long()[:S]]
    if node in ("pair", "split"):
        agg = bnn.weighted_aggregate(blk, z, ew, mean=True)
        out = bnn.sage_epilogue(y, agg, p, ctr, 5)[0] if relu else y + agg
    elif node == "dual":
        agg = bnn.weighted_aggregate(blk, h, ew, mean=True)
        out, _ = bnn._SageDualLinear.apply(agg, h_dst, wn, ws, b, relu, p, ctr, 5, Sb, dst_dev)
    else:
        out, _ = bnn.sage_agg_dual(blk, h, ew, wn, ws, b, relu, p, ctr, 5, dst_dev)
    out.backward(g)
    torch.cuda.synchronize()
    return dict(out=out.detach(), h=h, h_dst=h_dst, wn=wn, ws=ws, b=b, g=g, ew=ew, h_ref=h_ref, hd_ref=hd_ref, ids=ids)


# node, in, out, ReLU, dropout, bias, gathered rows
LAYER_CONFIGS = [("pair", 602, 256, True, 0.25, True, False), ("pair", 602, 256, True, 0.0, True, True), ("pair", 256, 41, False, 0.0, True, False),
                 ("pair", 48, 16, True, 0.0, False, False), ("split", 602, 256, True, 0.25, True, False), ("split", 48, 16, True, 0.0, True, True),
                 ("split", 256, 41, False, 0.0, False, False), ("dual", 256, 256, True, 0.25, True, False), ("dual", 16, 48, True, 0.0, False, False),
                 ("aggdual", 256, 256, True, 0.25, True, False), ("aggdual", 16, 48, False, 0.0, True, False), ("aggdual", 256, 256, True, 0.0, False, False)]
LAYER_BLOCKS = [("edge", False), ("edge", True), ("r16384", False), ("r16385", True), ("hubs", False)]


def _check_layer(dev, spec, padded, node, fin, fout, relu, p, bias, gather, t, what, library=False):
    S, K = spec.S, spec.K
    src, dst = spec.src.to(dev), spec.dst.to(dev)
    B = spec.B
    o = dict(src=src, dst=dst, S=S, h=t["h_ref"], w_neigh=t["wn"].detach(), w_self=t["ws"].detach(), bias=None if t["b"] is None else t["b"].detach(),
             ew=t["ew"][:B], h_dst=t["hd_ref"])
    out = t["out"]
    lin_first = fin > fout
    two_nodes = library or (node == "split" and gather)
    k = sage_layer_k(fin, fout, max(K, S), p > 0, lin_first, two_nodes=two_nodes)
    r = {}
    assert not bool(_bits(out[S:]).any()), what + ": padding rows of out must be exact zeros"
    mask = None
    if relu:
        mask = out[:S] > 0
    if relu and p == 0:
        # the reference's own ReLU holds the kernel's mask wherever it is decided: |relu(a) - relu(b)| <= |a - b|, so the bound
        # of the pre-activation (its unmasked magnitude) holds for relu(rst) too
        f = sage_layer_terms(**o, relu=True)
        r["out"] = assert_within(out[:S], torch.relu(f["rst"]), f["mag_rst"], *k["out"], what + " out (reference mask)")
    ref = sage_layer_terms(**o, g=t["g"][:S], mask=mask, p=p, relu=relu)
    r["out_m"] = assert_within(out[:S], ref["out"], ref["mag_out"], *k["out"], what + " out")
    if p > 0:
        pre = sage_layer_terms(**o, relu=True)
        clear = pre["rst"] > 2 * (ulp_bf16(pre["rst"]) + k["out"][1] * 2.0 ** -8 * pre["mag_rst"])
        share = 1.0 - float((mask & clear).sum()) / float(clear.sum())
        assert abs(share - p) < 0.02, share
    r["d_wn"] = assert_within(t["wn"].grad, ref["d_wn"], ref["mag_d_wn"], *k["d_wn"], what + " d W_neigh")
    r["d_ws"] = assert_within(t["ws"].grad, ref["d_ws"], ref["mag_d_ws"], *k["d_ws"], what + " d W_self")
    if bias:
        r["d_b"] = assert_within(t["b"].grad, ref["d_b"], ref["mag_d_b"], *k["d_b"], what + " d b")
    if node == "pair" and gather:
        assert t["h"].grad is None
        return r
    d_h, mag_h = ref["d_h"], ref["mag_d_h"]
    if node == "split" and gather:                           # fc_self's input gradient goes back into the source rows it was gathered from
        ids = t["ids"].long()[:S]
        d_h, mag_h = d_h.index_add(0, ids, ref["d_hdst"]), mag_h.index_add(0, ids, ref["mag_d_hdst"])
    r["d_h"] = assert_within(t["h"].grad[:K], d_h, mag_h, *k["d_h"], what + " d h")
    assert not bool(_bits(t["h"].grad[K:]).any()), what + ": padding rows of d h must be exact zeros"
    if t["h_dst"] is not None:
        r["d_hdst"] = assert_within(t["h_dst"].grad[:S], ref["d_hdst"], ref["mag_d_hdst"], *k["d_hdst"], what + " d h_dst")
        assert not bool(_bits(t["h_dst"].grad[S:]).any()), what + ": padding rows of d h_dst must be exact zeros"
    return r


@pytest.mark.parametrize("block,padded", LAYER_BLOCKS, ids=lambda v: str(v))
@pytest.mark.parametrize("cfg", LAYER_CONFIGS, ids=lambda c: "-".join(str(v) for v in c))
def test_sage_layer_nodes_per_element(cuda, block, padded, cfg):
    """_SageLinearPair (with and without gathered ids), _SageLinearSplit (destination rows handed in or gathered),
    _SageDualLinear and sage_agg_dual on the designed blocks of the message-passing suite (edge shapes, 16 384 / 16 385 rows,
    many hubs; capacity-padded copies with the device-side counts below the bounds and NaN rows beyond them) at the models'
    widths: output, d h (and d h_dst), both d W and d b against fp64 (bounds.sage_layer_terms, whose backward
    tests/test_bounds.py checks against autograd) with bounds.sage_layer_k.  The ReLU / dropout mask of the reference's
    backward is the kernel's (out > 0), after the forward check against the reference's own ReLU (p = 0) or the dropped share
    of the clearly positive elements (p > 0) has held it."""
    node, fin, fout, relu, p, bias, gather = cfg
    spec = _spec(block)
    blk = padded_block(spec, cuda) if padded else to_block(spec, cuda)
    if padded:
        blk._counts_dev[3] = spec.K                          # bliss_layer_counts_t: the true source count (word 3)
    t = _run_layer(cuda, spec, blk, padded, node, fin, fout, relu, p, bias, gather, seed=fin + fout)
    what = "%s %s%s %d->%d" % (node, block, "-padded" if padded else "", fin, fout)
    _report(what.replace(" ", "-") + "-p%g-g%d" % (p, gather), _check_layer(cuda, spec, padded, node, fin, fout, relu, p, bias, gather, t, what))


@pytest.mark.parametrize("cfg", [("pair", 602, 256, True, 0.0, True, False), ("dual", 256, 256, True, 0.25, True, False),
                                 ("aggdual", 256, 256, True, 0.25, True, False), ("aggdual", 16, 48, False, 0.0, True, False)],
                         ids=lambda c: "-".join(str(v) for v in c))
def test_sage_layer_nodes_library_backward_per_element(cuda, cfg, monkeypatch):
    """BLISS_SAGE_MFMA_BWD=0 (read on every call): the library GEMMs of the fallback are held to the same fp64 reference as
    the MFMA kernels; the routes that store one more value on the way to d h (d W_neigh in front of the transposed SpMM, dZ W_neigh
    in front of addmm_) take sage_layer_k's two_nodes constant."""
    monkeypatch.setenv("BLISS_SAGE_MFMA_BWD", "0")
    node, fin, fout, relu, p, bias, gather = cfg
    spec = _spec("edge")
    t = _run_layer(cuda, spec, to_block(spec, cuda), False, node, fin, fout, relu, p, bias, gather, seed=fin + fout)
    what = "%s-library edge %d->%d" % (node, fin, fout)
    _report(what.replace(" ", "-"), _check_layer(cuda, spec, False, node, fin, fout, relu, p, bias, gather, t, what, library=node != "dual"))


if __name__ == "__main__":
    assert sys.argv[1] == "--wgs-child"
    _wgs_child(int(sys.argv[2]))
