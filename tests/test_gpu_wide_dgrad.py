"""GPU suite: bliss_dgrad_wide (csrc/sage_bwd.hip) -- out = A[m, k] . W[k, n] with k walked in panels of 1024
rows of W -- element by element against float64 with bounds.dense_k(K1 + K2), an exact one-hot probe of the panel seams, bit
equality with bliss_gat_dgrad where one panel covers k, and a misaligned run.  Conventions of tests/test_gpu_sage_dense_edges.py:
rows beyond the device-side counts are NaN / Inf, m_bound = M + 40, rows in [M, m_bound) come out as exact zeros."""
import ctypes as C

import pytest
import torch

from bounds import assert_within, dense_k, dgrad_terms
from test_gpu_wide_gemm import _bits, _place, _report
from wide_cases import BF, INF, NAN, one_hot_rows, rand

pytestmark = pytest.mark.gpu


def _call(entry, a1, w1, m_bound, m_dev=0, a2=None, w2=None, m2_bound=0, m2_dev=0):
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd._engine import _stream
    out = torch.full((m_bound, w1.shape[1]), NAN, dtype=BF, device=a1.device)
    t = _lib.DGrad()
    t.a1, t.a1_stride, t.w1, t.w1_stride, t.k1 = a1.data_ptr(), a1.stride(0), w1.data_ptr(), w1.stride(0), w1.shape[0]
    if a2 is not None:
        t.a2, t.a2_stride, t.w2, t.w2_stride, t.k2 = a2.data_ptr(), a2.stride(0), w2.data_ptr(), w2.stride(0), w2.shape[0]
        t.m2_bound, t.m2_dev = int(m2_bound), int(m2_dev)
    t.m_bound, t.m_dev, t.n = int(m_bound), int(m_dev), w1.shape[1]
    t.out, t.out_stride = out.data_ptr(), out.stride(0)
    fn = {"wide": _lib.lib.bliss_dgrad_wide, "gat": _lib.lib.bliss_gat_dgrad}[entry]
    _lib.check(fn(C.byref(t), _stream()), "dgrad(%s)" % entry)
    return out


def _dgrad(dev, M, K1, N, K2=0, M2=0, views=(), pad=NAN, entry="wide", extra=40):
    """out = A1 W1 (+ A2 W2 on rows < min(M2, M)); M, M2 are the device-side counts, M + extra and M2 + extra the bounds."""
    gen = torch.Generator().manual_seed(1000 * K1 + 10 * N + M)
    mb, m2b = M + extra, M2 + extra
    a1, w1 = rand(gen, mb, K1, scale=0.1), rand(gen, K1, N, scale=0.2)
    a1[M:] = pad
    a1d, _ = _place(a1, dev, "a1" in views)
    w1d, _ = _place(w1, dev, "w1" in views)
    a2 = w2 = a2d = w2d = None
    if K2:
        a2, w2 = rand(gen, m2b, K2, scale=0.1), rand(gen, K2, N, scale=0.2)
        a2[M2:] = pad
        a2d, _ = _place(a2, dev, "a2" in views)
        w2d, _ = _place(w2, dev, "w2" in views)
    cnt = torch.tensor([M, M2], dtype=torch.int32, device=dev)
    out = _call(entry, a1d, w1d, mb, cnt.data_ptr(), a2=a2d, w2=w2d, m2_bound=m2b, m2_dev=cnt.data_ptr() + 4 if K2 else 0)
    torch.cuda.synchronize()
    ref, mag = dgrad_terms(a1[:M].to(dev), w1.to(dev), None if not K2 else torch.nan_to_num(a2, posinf=0.0).to(dev),
                           None if not K2 else w2.to(dev), m2=min(M2, M) if K2 else None)
    return out, ref, mag


# (K, N, M): every K of {1025, 1040, 1089, 1433, 2048, 2049, 16384}, every N of {1, 16, 255, 256, 257, 602}, every M of {1, 33, 70}
WIDE_DGRAD = [(1025, 1, 1), (1040, 16, 33), (1089, 255, 70), (1433, 256, 33), (1433, 602, 70), (2048, 257, 1), (2049, 602, 33),
              (16384, 16, 70), (16384, 257, 33)]


@pytest.mark.parametrize("K,N,M", WIDE_DGRAD, ids=lambda v: str(v))
def test_wide_dgrad_against_fp64(cuda, K, N, M):
    """dense_k(K); rows in [M, M + 40) exact zeros; rows of A beyond the device-side count are NaN; N past 256 runs a second
    column block (blockIdx.y) through the same panels."""
    out, ref, mag = _dgrad(cuda, M, K, N)
    ratio = assert_within(out[:M], ref, mag, *dense_k(K), "wide dgrad")
    assert out.shape == (M + 40, N) and not bool(_bits(out[M:]).any()), "rows beyond the count must be exact zeros"
    _report("wide-dgrad-%d-%d-%d" % (K, N, M), {"out": ratio})


def test_wide_dgrad_dual_product(cuda):
    """(K1, K2) = (1433, 1100) into one accumulator, the second product on M2 = 33 < M = 70 rows (it ends inside the second row
    tile; the third tile never stages it): dense_k(K1 + K2) -- a pair bliss_gat_dgrad refuses for its LDS."""
    M, M2, K1, K2, N = 70, 33, 1433, 1100, 257
    out, ref, mag = _dgrad(cuda, M, K1, N, K2=K2, M2=M2)
    ratio = assert_within(out[:M], ref, mag, *dense_k(K1 + K2), "wide dgrad dual")
    assert not bool(_bits(out[M:]).any())
    _report("wide-dgrad-dual-%d-%d-%d" % (K1, K2, N), {"out": ratio})


@pytest.mark.parametrize("K", [1025, 1433, 2049, 16384])
def test_wide_dgrad_seam_probe_is_exact(cuda, K):
    """One-hot rows of A at the columns 0, 1023, 1024, 1025, K - 1 (2047, 2048): out[r, :] must have the BITS of W[c, :]."""
    N, M = 257, 70
    a, col = one_hot_rows(K, M)
    w = rand(torch.Generator().manual_seed(K), K, N).to(cuda)
    out = _call("wide", a.to(cuda), w, M)
    torch.cuda.synchronize()
    bad = (_bits(out) != _bits(w[col.to(cuda)])).any(1).nonzero().reshape(-1).tolist()
    assert not bad, "K %d: rows %s (columns %s) differ" % (K, bad[:8], [int(col[r]) for r in bad[:8]])


@pytest.mark.parametrize("K1,K2", [(256, 0), (1024, 0), (256, 256)])
def test_one_panel_dgrad_is_the_narrow_kernel(cuda, K1, K2):
    """At k <= 1024 one panel per operand: the bits of bliss_gat_dgrad on the same arguments, zero rows included."""
    narrow, ref, mag = _dgrad(cuda, 70, K1, 257, K2=K2, M2=33 if K2 else 0, entry="gat")
    wide, _, _ = _dgrad(cuda, 70, K1, 257, K2=K2, M2=33 if K2 else 0, entry="wide")
    assert torch.equal(_bits(wide), _bits(narrow))
    _report("wide-dgrad-one-panel-%d-%d" % (K1, K2), {"out": assert_within(wide[:70], ref, mag, *dense_k(K1 + K2), "one panel")})


def test_wide_dgrad_alignment_does_not_change_a_bit(cuda):
    """a1, a2, w1, w2 as misaligned windows (ld8_masked(..., aligned=false) for the rows and for the W slabs of every panel)
    against the aligned run; +Inf instead of NaN beyond the counts."""
    M, M2, K1, K2, N = 45, 33, 1440, 1100, 258
    base, ref, mag = _dgrad(cuda, M, K1, N, K2=K2, M2=M2, pad=INF)
    ratio = assert_within(base[:M], ref, mag, *dense_k(K1 + K2), "wide dgrad aligned")
    for v in ("a1", "a2", "w1", "w2", ("a1", "a2", "w1", "w2")):
        got, _, _ = _dgrad(cuda, M, K1, N, K2=K2, M2=M2, views=v if isinstance(v, tuple) else (v,), pad=INF)
        assert torch.equal(_bits(got), _bits(base)), "wide dgrad differs with %s misaligned" % (v,)
    _report("wide-dgrad-align-%d-%d-%d" % (K1, K2, N), {"out": ratio})
