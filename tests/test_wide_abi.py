"""CPU suite: bliss_tile_gemm_wide and bliss_dgrad_wide validate their arguments on the host -- BLISS_EINVAL
before any launch, so this runs without a GPU -- and the header's BLISS_WIDE_MAX_K is the constant Python binds."""
import ctypes as C
import os
import re

from conftest import ROOT


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    return _lib


def _buf():
    buf = (C.c_int64 * 64)()
    return buf, C.addressof(buf)


def _gemm(_lib, p, **kw):
    t = _lib.TileGemm()
    t.a1, t.a1_stride, t.w1, t.w1_stride, t.k1 = p, 2048, p, 2048, 2048
    t.m_bound, t.n, t.out, t.out_stride = 4, 8, p, 8
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _dgrad(_lib, p, **kw):
    t = _lib.DGrad()
    t.a1, t.a1_stride, t.w1, t.w1_stride, t.k1 = p, 2048, p, 8, 2048
    t.m_bound, t.n, t.out, t.out_stride = 4, 8, p, 8
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_the_header_constant_is_the_bound_constant():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "bliss_gnn.h")).read()
    m = re.search(r"#define\s+BLISS_WIDE_MAX_K\s+(\d+)", text)
    assert m and int(m.group(1)) == L.WIDE_MAX_K == 16384
    from bliss_gnn_amd import nn
    assert nn.TILE_WIDE_MAX_K == L.WIDE_MAX_K and nn.TILE_GEMM_MAX_K == 1024


def test_tile_gemm_wide_refuses_bad_arguments_before_any_launch():
    L = _lib()
    lib, E = L.lib, L.EINVAL
    keep, p = _buf()
    call = lambda first, second=None: lib.bliss_tile_gemm_wide(C.byref(first), None if second is None else C.byref(second), 0)
    two = dict(a2=p, a2_stride=2048, w2=p, w2_stride=2048)
    assert lib.bliss_tile_gemm_wide(None, None, 0) == E                                   # no argument set
    assert call(_gemm(L, p, k1=0)) == E
    assert call(_gemm(L, p, k1=L.WIDE_MAX_K + 1)) == E
    assert call(_gemm(L, p, k2=L.WIDE_MAX_K + 1, **two)) == E
    assert call(_gemm(L, p, k2=-1, **two)) == E
    assert call(_gemm(L, p, n=257)) == E
    assert call(_gemm(L, p, n=0)) == E
    assert call(_gemm(L, p, m_bound=0)) == E
    for field in ("a1", "w1", "out"):
        assert call(_gemm(L, p, **{field: None})) == E, field                             # a null operand
    for field in ("a2", "w2"):
        assert call(_gemm(L, p, k2=2048, **dict(two, **{field: None}))) == E, field       # a second product without an operand
    assert call(_gemm(L, p, drop_p=0.25)) == E                                            # a dropout probability without a counter
    assert call(_gemm(L, p, drop_p=1.0, drop_ctr=p)) == E
    assert call(_gemm(L, p), _gemm(L, p, k1=L.WIDE_MAX_K + 1)) == E                       # the second set is checked as well
    assert call(_gemm(L, p), _gemm(L, p, n=257)) == E
    del keep


def test_dgrad_wide_refuses_bad_arguments_before_any_launch():
    L = _lib()
    lib, E = L.lib, L.EINVAL
    keep, p = _buf()
    call = lambda t: lib.bliss_dgrad_wide(C.byref(t), 0)
    two = dict(a2=p, a2_stride=2048, w2=p, w2_stride=8, m2_bound=4)
    assert lib.bliss_dgrad_wide(None, 0) == E
    assert call(_dgrad(L, p, k1=0)) == E
    assert call(_dgrad(L, p, k1=L.WIDE_MAX_K + 1)) == E
    assert call(_dgrad(L, p, k2=L.WIDE_MAX_K + 1, **two)) == E
    assert call(_dgrad(L, p, k2=-1, **two)) == E
    assert call(_dgrad(L, p, n=0)) == E
    assert call(_dgrad(L, p, m_bound=0)) == E
    for field in ("a1", "w1", "out"):
        assert call(_dgrad(L, p, **{field: None})) == E, field
    for field in ("a2", "w2"):
        assert call(_dgrad(L, p, k2=2048, **dict(two, **{field: None}))) == E, field
    assert call(_dgrad(L, p, k2=2048, **dict(two, m2_bound=0))) == E                      # a second product over no rows
    del keep


def test_the_narrow_entry_points_keep_their_limit():
    """bliss_tile_gemm, bliss_sage_dgrad and bliss_gat_dgrad still refuse what they refused: 1025 columns (and 257 for the SAGE
    dgrad), before any launch."""
    L = _lib()
    lib, E = L.lib, L.EINVAL
    keep, p = _buf()
    assert lib.bliss_tile_gemm(C.byref(_gemm(L, p, k1=1025)), None, 0) == E
    assert lib.bliss_gat_dgrad(C.byref(_dgrad(L, p, k1=1025)), 0) == E
    assert lib.bliss_sage_dgrad(C.byref(_dgrad(L, p, k1=257)), 0) == E
    del keep
