"""CPU suite: the row entry points of csrc/spmm.hip (bliss_gather_rows, bliss_sage_epilogue_fwd / _bwd, bliss_embed_norm; DESIGN.md
section 31) validate their arguments on the host -- BLISS_EINVAL before any launch, or 0 for nothing to do, so this runs without a
GPU.  The pointers handed over are host memory no call may get as far as touching."""
import ctypes as C


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    return _lib


def _buf():
    buf = (C.c_int64 * 64)()
    return buf, C.addressof(buf)


def test_gather_rows_refuses_bad_arguments_before_any_launch():
    L = _lib()
    E, keep = L.EINVAL, _buf()
    p = keep[1]
    ok = dict(feat=p, feat_stride=64, ids=p, n_rows=4, dim=64, out=p, out_stride=64, norm_out=p)
    call = lambda **kw: (lambda a: L.lib.bliss_gather_rows(a["feat"], a["feat_stride"], a["ids"], a["n_rows"], a["dim"], a["out"], a["out_stride"],
                                                           a["norm_out"], 0))(dict(ok, **kw))
    for field in ("feat", "ids", "out"):
        assert call(**{field: None}) == E, field
    assert call(dim=0) == E and call(dim=-4) == E
    assert call(feat_stride=63) == E and call(out_stride=63) == E
    assert call(dim=6145, feat_stride=6145, out_stride=6145) == E               # 6144 is the last size one wave stages in LDS
    assert call(dim=6152, feat_stride=6152, out_stride=6152) == E               # (6145 .. 6151 round up to the same 8-element pad)
    assert call(n_rows=0) == 0 and call(n_rows=-1) == 0
    assert call(n_rows=0, norm_out=None) == 0
    assert call(n_rows=0, dim=6152, feat_stride=6152, out_stride=6152) == 0     # nothing to do comes first: no LDS is asked for
    del keep


def test_sage_epilogue_refuses_bad_arguments_before_any_launch():
    L = _lib()
    E, keep = L.EINVAL, _buf()
    p = keep[1]
    ok = dict(a=p, a_stride=8, b=p, b_stride=8, n_rows=4, dim=8, p=0.25, seed=1, ctr=p, out=p, out_stride=8, norm=p)
    fwd = lambda **kw: (lambda a: L.lib.bliss_sage_epilogue_fwd(a["a"], a["a_stride"], a["b"], a["b_stride"], a["n_rows"], a["dim"], a["p"], a["seed"],
                                                                a["ctr"], a["out"], a["out_stride"], a["norm"], 0))(dict(ok, **kw))
    for field in ("a", "b", "out"):
        assert fwd(**{field: None}) == E, field
    assert fwd(dim=0) == E and fwd(dim=-1) == E
    assert fwd(n_rows=-1) == E
    assert fwd(p=-0.01) == E and fwd(p=1.0) == E and fwd(p=1.5) == E and fwd(p=float("nan")) == E
    assert fwd(ctr=None) == E                                                   # p > 0 needs the counter
    assert fwd(n_rows=0) == 0 and fwd(n_rows=0, p=0.0, ctr=None, norm=None) == 0

    okb = dict(dout=p, dout_stride=8, out=p, out_stride=8, n_rows=4, dim=8, p=0.25, din=p, din_stride=8)
    bwd = lambda **kw: (lambda a: L.lib.bliss_sage_epilogue_bwd(a["dout"], a["dout_stride"], a["out"], a["out_stride"], a["n_rows"], a["dim"], a["p"],
                                                                a["din"], a["din_stride"], 0))(dict(okb, **kw))
    for field in ("dout", "out", "din"):
        assert bwd(**{field: None}) == E, field
    assert bwd(dim=0) == E and bwd(dim=-1) == E
    assert bwd(n_rows=-1) == E
    assert bwd(p=-0.01) == E and bwd(p=1.0) == E and bwd(p=float("nan")) == E
    assert bwd(n_rows=0) == 0
    del keep


def test_embed_norm_refuses_bad_arguments_before_any_launch():
    L = _lib()
    E, keep = L.EINVAL, _buf()
    p = keep[1]
    f = L.lib.bliss_embed_norm
    assert f(None, 4, 8, 8, p, 0) == E and f(p, 4, 8, 8, None, 0) == E
    assert f(p, 0, 8, 8, p, 0) == 0 and f(p, -3, 8, 8, p, 0) == 0
    del keep
