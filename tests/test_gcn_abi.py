"""CPU suite: the entry points of csrc/gcn.hip are exported and bound, and refuse bad arguments on the host
before any launch (so this runs without a GPU): null pointers, negative counts, row strides below the row length, a dropout
probability outside [0, 1), a dropout without its counter words, a bias gradient without its scratch."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def env():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    buf = (C.c_int64 * 64)()
    return _lib, C.addressof(buf), buf


NAMES = ("bliss_gcn_norms", "bliss_gcn_spmm_fwd", "bliss_gcn_spmm_bwd", "bliss_gcn_db_chunk_rows", "bliss_gcn_epilogue_fwd",
         "bliss_gcn_epilogue_bwd")


def test_symbols_are_exported_and_bound(env):
    _lib = env[0]
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
    assert _lib.lib.bliss_gcn_db_chunk_rows() == 32
    assert C.sizeof(_lib.GcnEpilogue) == 144


def test_norms_and_spmm_refuse_bad_arguments(env):
    _lib, p, _ = env
    lib, E = _lib.lib, _lib.EINVAL
    assert lib.bliss_gcn_norms(0, 4, p, 4, p, p, 0) == E                                   # no indptr
    assert lib.bliss_gcn_norms(p, 4, p, 4, 0, p, 0) == E                                   # no nd
    assert lib.bliss_gcn_norms(p, 4, 0, 4, p, p, 0) == E                                   # no t_indptr
    assert lib.bliss_gcn_norms(p, -1, p, 4, p, p, 0) == E and lib.bliss_gcn_norms(p, 4, p, -1, p, p, 0) == E
    assert lib.bliss_gcn_norms(p, 0, p, 0, p, p, 0) == 0                                   # nothing to do: no launch
    fwd = lambda indptr=p, src=p, dst=p, ns=p, nd=p, h=p, hs=8, nnz=16, dim=8, out=p, os_=8, part=p: lib.bliss_gcn_spmm_fwd(
        indptr, src, dst, 0, ns, nd, h, hs, 4, 0, nnz, dim, out, os_, part, 0)
    for kw in (dict(indptr=0), dict(src=0), dict(dst=0), dict(ns=0), dict(nd=0), dict(h=0), dict(out=0), dict(part=0), dict(nnz=-1),
               dict(dim=0), dict(hs=7), dict(os_=7)):
        assert fwd(**kw) == E, kw
    bwd = lambda t_indptr=p, t_edge=p, src=p, dst=p, ns=p, nd=p, g=p, gs=8, nnz=16, dim=8, gh=p, hs=8, part=p: lib.bliss_gcn_spmm_bwd(
        t_indptr, t_edge, src, dst, 0, ns, nd, g, gs, 4, 0, nnz, dim, gh, hs, part, 0)
    for kw in (dict(t_indptr=0), dict(t_edge=0), dict(src=0), dict(dst=0), dict(ns=0), dict(nd=0), dict(g=0), dict(gh=0), dict(part=0),
               dict(nnz=-1), dict(dim=0), dict(gs=7), dict(hs=7)):
        assert bwd(**kw) == E, kw


def _epi(_lib, p, **kw):
    t = _lib.GcnEpilogue()
    t.a, t.a_stride, t.n_rows, t.width = p, 8, 4, 8
    t.out, t.out_stride = p, 8
    t.dout, t.dout_stride, t.din, t.din_stride = p, 8, p, 8
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_epilogue_refuses_bad_arguments(env):
    _lib, p, _ = env
    lib, E = _lib.lib, _lib.EINVAL
    assert lib.bliss_gcn_epilogue_fwd(None, 0) == E and lib.bliss_gcn_epilogue_bwd(None, 0) == E
    for kw in (dict(a=None), dict(out=None), dict(n_rows=0), dict(width=0), dict(a_stride=7), dict(out_stride=7), dict(drop_p=1.0),
               dict(drop_p=-0.5), dict(drop_p=0.5), dict(drop_p=0.5, drop_ctr=p), dict(n_rows=1 << 30, width=8)):
        assert lib.bliss_gcn_epilogue_fwd(C.byref(_epi(_lib, p, **kw)), 0) == E, kw
    for kw in (dict(dout=None), dict(din=None), dict(n_rows=0), dict(width=0), dict(dout_stride=7), dict(din_stride=7), dict(drop_p=1.0),
               dict(drop_p=0.5), dict(relu=1, out=None), dict(db=p), dict(db=p, db_partials=p + 2)):
        assert lib.bliss_gcn_epilogue_bwd(C.byref(_epi(_lib, p, **kw)), 0) == E, kw
