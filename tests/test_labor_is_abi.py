"""CPU suite: the device-side LABOR-i sampler's entry points are exported and bound, refuse bad arguments before any launch
(no GPU is touched), and ``fit.ImportanceLaborSampler`` / ``make_sampler("labor-<i>", ...)`` check their keywords."""
import ctypes as C

import pytest


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    return _lib


def test_symbols_are_exported_and_bound():
    _l = _lib()
    raw = C.CDLL(_l.LIB_PATH)
    for n in ("bliss_labor_is_layer", "bliss_labor_is_scratch_bytes"):
        assert hasattr(raw, n), n
    assert len(_l.SIGNATURES["bliss_labor_is_layer"]) == len(_l.SIGNATURES["bliss_labor_layer"]) + 1 == 17        # + iterations
    assert _l.lib.bliss_labor_is_layer.restype is C.c_int
    assert "bliss_labor_is_scratch_bytes" in _l.SPECIAL_SIGNATURES
    assert len(_l.lib.bliss_labor_is_scratch_bytes.argtypes) == 3 and _l.lib.bliss_labor_is_scratch_bytes.restype is C.c_int64


def test_scratch_bytes():
    lib, E = _lib().lib, _lib().EINVAL
    f = lib.bliss_labor_is_scratch_bytes
    assert f(0, 4, 4) == E and f(10, 0, 4) == E and f(-1, 4, 4) == E and f(10, -2, 4) == E and f(10, 4, -1) == E
    for v in (1, 32 * 1024, 32 * 1024 + 1, 32 * 1024 + 37, 6000):
        words = -(-(-(-v // 32)) // 1024) * 1024                     # the bitmap, whole tiles of 1024 words
        prev_s = 0
        for cap_s in (1, 7, 1025):
            prev_b = 0
            for cap_b in (0, 1, 9, 4096):
                n = f(v, cap_s, cap_b)
                # tickets, bitmap, tile counts, two importance buffers, kept counts and scales, p_e
                assert n % 16 == 0 and n >= 4 * (16 + words + words // 1024 + 2 * v + 2 * cap_s + cap_b)
                assert n >= lib.bliss_labor_scratch_bytes(v, cap_s) + 4 * (2 * v + cap_s + cap_b) - 15
                assert n >= prev_b                                   # monotone in every argument
                prev_b = n
            assert prev_b >= prev_s
            prev_s = prev_b
        assert f(v + 1, 7, 9) >= f(v, 7, 9)


def test_layer_refuses_bad_arguments_before_any_launch():
    _l = _lib()
    lib, E = _l.lib, _l.EINVAL
    buf = (C.c_int64 * 64)()                                         # 16-byte aligned stand-in for every device pointer
    p = C.addressof(buf)
    assert p % 16 == 0

    def call(g=None, seeds=p, n_seeds=1, n_dev=0, cap_s=4, fanout=2, ov=0, step=p, bump=1, dep=0, iters=1, ws=None, out=None,
             scratch=p, **kw):
        gg = _l.Graph(p, p, 0, 10, 100) if g is None else g
        w = _l.LayerWs() if ws is None else ws
        if ws is None:
            w.counts, w.seg_ptr, w.kept_nid, w.kept_map, w.cap_k = p, p, p, p, 8
        o = _l.BlockOut(p, p, p, p, p, p, p, 0, 0, 0, 16) if out is None else out
        for k, v in kw.items():
            setattr(w if hasattr(w, k) else o, k, v)
        return lib.bliss_labor_is_layer(C.byref(gg) if g != 0 else None, seeds, n_seeds, n_dev, cap_s, fanout, ov, 5, step, 0, bump,
                                        dep, iters, C.byref(w) if ws != 0 else None, C.byref(o) if out != 0 else None, scratch, 0)

    for iters in (0, 1, 8):
        for dep in (0, 1):
            kw = dict(dep=dep, iters=iters)
            assert call(g=0, **kw) == E and call(ws=0, **kw) == E and call(out=0, **kw) == E
            assert call(seeds=0, **kw) == E and call(scratch=0, **kw) == E
            assert call(cap_s=0, **kw) == E and call(cap_s=-3, **kw) == E
            assert call(fanout=0, **kw) == E
    for iters in (-1, 9, 2 ** 31 - 1, -2 ** 31):                      # the iteration count is a launch-time constant in 0 .. 8
        assert call(iters=iters) == E
    assert call(g=_l.Graph(p, p, 0, 10, 2 ** 31)) == E               # int32 edge positions
    assert call(g=_l.Graph(p, p, 0, 10, -1)) == E and call(g=_l.Graph(p, p, 0, 0, 100)) == E
    assert call(g=_l.Graph(0, p, 0, 10, 100)) == E and call(g=_l.Graph(p, 0, 0, 10, 100)) == E
    assert call(scratch=p + 8) == E                                  # misaligned scratch
    assert call(n_seeds=-1, n_dev=0) == E                            # a device-side count needs its pointer
    assert call(step=0) == E and call(step=0, bump=0) == E           # the hash needs the step counter ...
    assert call(step=0, ov=p, bump=1) == E                           # ... and so does the bump
    for field in ("counts", "seg_ptr", "kept_nid", "kept_map", "indptr", "src", "dst", "pos", "eid", "edge_weights", "q_ij"):
        assert call(**{field: 0}) == E, field
    assert call(cap_k=0) == E and call(cap_b=-1) == E


def test_keywords_of_the_importance_labor_sampler():
    _lib()
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.fit import ImportanceLaborSampler, LaborSampler
    assert bg.ImportanceLaborSampler is ImportanceLaborSampler and issubclass(ImportanceLaborSampler, LaborSampler)
    s = ImportanceLaborSampler([4, 4], seed=9)
    assert s.iterations == 1 and s.draw == "device" and s.draw_step() == 0 and s._engine is None and s.nodes_per_layer == [4, 4]
    assert s.layer_dependency is False and ImportanceLaborSampler([4], 2, True).layer_dependency is True
    assert ImportanceLaborSampler([4], 3).iterations == 3 and ImportanceLaborSampler([4], iterations=0).iterations == 0
    assert ImportanceLaborSampler([4], iterations=8).iterations == 8
    s.reset_draw(seed=3, step=17)
    assert s.draw_step() == 17
    for name in ("sample_blocks", "sample_blocks_static", "finish_static", "check_errors"):
        assert callable(getattr(s, name))
    ImportanceLaborSampler([4], prefetch_node_feats=None)            # (unknown DGL keywords are ignored)
    for it in (-1, 9, 1.5, True):                                    # -1 = DGL's "until convergence": cannot be captured
        with pytest.raises(ValueError):
            ImportanceLaborSampler([4, 4], iterations=it)
    assert LaborSampler([4]).__dict__.get("iterations") is None      # (LABOR-0 is unchanged)
    with pytest.raises(NotImplementedError):
        LaborSampler([4], importance_sampling=1)


def test_make_sampler_returns_it():
    _lib()
    from bliss_gnn_amd.fit import ImportanceLaborSampler, LaborSampler, make_sampler
    for i in (1, 2, 8):
        s = make_sampler("labor-%d" % i, [4, 3])
        assert type(s) is ImportanceLaborSampler and s.iterations == i and s.draw == "device" and s.fanouts == [4, 3]
    assert type(make_sampler("labor-1", [4], draw="host")) is ImportanceLaborSampler
    assert type(make_sampler("labor", [4])) is LaborSampler
    for name in ("labor-0", "labor-9", "labor-", "labor--1", "labor-x", "labor-01"):
        with pytest.raises(ValueError):
            make_sampler(name, [4])
