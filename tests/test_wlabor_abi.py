"""CPU suite: the weighted device-side LABOR sampler's entry points are exported and bound, refuse bad arguments before any launch
(no GPU is touched), and ``fit.WeightedLaborSampler`` / ``fit.BanditLaborSampler`` / ``make_sampler("labor-exp3", ...)`` check
their keywords."""
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
    for n in ("bliss_wlabor_layer", "bliss_wlabor_scratch_bytes"):
        assert hasattr(raw, n), n
    # bliss_labor_layer's arguments + mode, prob_pos, eta, one_minus_eta (bliss_wneighbor_layer's) + p_ij
    assert len(_l.SIGNATURES["bliss_wlabor_layer"]) == len(_l.SIGNATURES["bliss_labor_layer"]) + 5 == 21
    assert _l.lib.bliss_wlabor_layer.restype is C.c_int
    assert "bliss_wlabor_scratch_bytes" in _l.SPECIAL_SIGNATURES
    assert len(_l.lib.bliss_wlabor_scratch_bytes.argtypes) == 3 and _l.lib.bliss_wlabor_scratch_bytes.restype is C.c_int64
    assert (_l.WN_RAW, _l.WN_EXP3) == (0, 1)


def test_scratch_bytes():
    lib, E = _lib().lib, _lib().EINVAL
    f = lib.bliss_wlabor_scratch_bytes
    assert f(0, 4, 4) == E and f(10, 0, 4) == E and f(-1, 4, 4) == E and f(10, -2, 4) == E and f(10, 4, -1) == E
    for v in (1, 32 * 1024, 32 * 1024 + 1, 32 * 1024 + 37, 6000):
        words = -(-(-(-v // 32)) // 1024) * 1024                     # the bitmap, whole tiles of 1024 words
        prev_s = 0
        for cap_s in (1, 7, 1025):
            prev_b = 0
            for cap_b in (0, 1, 9, 4096):
                n = f(v, cap_s, cap_b)
                # tickets, bitmap, tile counts, per seed two 8-byte records and a kept count, p_e
                assert n % 16 == 0 and n >= 4 * (16 + words + words // 1024 + 5 * cap_s + cap_b)
                assert n >= lib.bliss_labor_scratch_bytes(v, cap_s) + 4 * (4 * cap_s + cap_b) - 15
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

    def call(g=None, seeds=p, n_seeds=1, n_dev=0, cap_s=4, fanout=2, ov=0, step=p, bump=1, dep=0, mode=0, prob=p, eta=0.4, ome=0.6,
             ws=None, out=None, p_ij=p, scratch=p, **kw):
        gg = _l.Graph(p, p, 0, 10, 100) if g is None else g
        w = _l.LayerWs() if ws is None else ws
        if ws is None:
            w.counts, w.seg_ptr, w.kept_nid, w.kept_map, w.cap_k = p, p, p, p, 8
        o = _l.BlockOut(p, p, p, p, p, p, p, 0, 0, 0, 16) if out is None else out
        for k, v in kw.items():
            setattr(w if hasattr(w, k) else o, k, v)
        return lib.bliss_wlabor_layer(C.byref(gg) if g != 0 else None, seeds, n_seeds, n_dev, cap_s, fanout, ov, 5, step, 0, bump, dep,
                                      mode, prob, eta, ome, C.byref(w) if ws != 0 else None, C.byref(o) if out != 0 else None, p_ij,
                                      scratch, 0)

    for mode in (_l.WN_RAW, _l.WN_EXP3):
        for dep in (0, 1):
            kw = dict(dep=dep, mode=mode)
            # what bliss_labor_layer refuses
            assert call(g=0, **kw) == E and call(ws=0, **kw) == E and call(out=0, **kw) == E
            assert call(seeds=0, **kw) == E and call(scratch=0, **kw) == E
            assert call(cap_s=0, **kw) == E and call(cap_s=-3, **kw) == E
            assert call(fanout=0, **kw) == E
            assert call(g=_l.Graph(p, p, 0, 10, 2 ** 31), **kw) == E  # int32 edge positions
            assert call(g=_l.Graph(p, p, 0, 10, -1), **kw) == E and call(g=_l.Graph(p, p, 0, 0, 100), **kw) == E
            assert call(g=_l.Graph(0, p, 0, 10, 100), **kw) == E and call(g=_l.Graph(p, 0, 0, 10, 100), **kw) == E
            assert call(scratch=p + 8, **kw) == E                     # misaligned scratch
            assert call(n_seeds=-1, n_dev=0, **kw) == E               # a device-side count needs its pointer
            assert call(step=0, **kw) == E and call(step=0, bump=0, **kw) == E       # the hash needs the step counter ...
            assert call(step=0, ov=p, bump=1, **kw) == E              # ... and so does the bump
            for field in ("counts", "seg_ptr", "kept_nid", "kept_map", "indptr", "src", "dst", "pos", "eid", "edge_weights", "q_ij"):
                assert call(**{field: 0}, **kw) == E, field
            assert call(cap_k=0, **kw) == E and call(cap_b=-1, **kw) == E
            # what bliss_wneighbor_layer refuses
            assert call(prob=0, **kw) == E and call(prob=p + 1, **kw) == E
            assert call(ov=p + 2, bump=0, **kw) == E                  # planted keys are 32-bit words
            # the new output
            assert call(p_ij=0, **kw) == E and call(p_ij=p + 1, **kw) == E
    for mode in (-1, 2, 7):
        assert call(mode=mode) == E
    for eta, ome in ((-0.1, 0.6), (0.4, -0.6), (float("nan"), 0.6), (0.4, float("nan"))):
        assert call(mode=_l.WN_EXP3, eta=eta, ome=ome) == E


def test_keywords_of_the_two_samplers():
    _lib()
    import torch
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.fit import (BanditLaborSampler, BanditNeighborSampler, ImportanceLaborSampler, LaborSampler,
                                   WeightedLaborSampler)
    assert bg.WeightedLaborSampler is WeightedLaborSampler and bg.BanditLaborSampler is BanditLaborSampler
    assert issubclass(WeightedLaborSampler, LaborSampler) and not issubclass(WeightedLaborSampler, ImportanceLaborSampler)
    assert issubclass(BanditLaborSampler, bg.BanditLadiesSampler) and not issubclass(BanditLaborSampler, BanditNeighborSampler)
    s = WeightedLaborSampler([4, 4], "w", seed=9)
    assert s.prob == "w" and s.draw == "device" and s.draw_step() == 0 and s._engine is None and s.nodes_per_layer == [4, 4]
    assert s.layer_dependency is False and WeightedLaborSampler([4], "w", True).layer_dependency is True
    assert WeightedLaborSampler([4], prob=torch.ones(3)).prob.numel() == 3
    with pytest.raises(ValueError):
        WeightedLaborSampler([4], None)
    with pytest.raises(TypeError):
        WeightedLaborSampler([4])
    b = BanditLaborSampler([4, 3], seed=9)
    assert (b.eta, b.T, b.model, b.draw, b.layer_dependency) == (0.4, 5000, "sage", "device", False)
    assert b.fanouts == b.nodes_per_layer == [4, 3] and b._engine is None and b.exp3_weights is None
    assert BanditLaborSampler([4], eta=0.1, num_steps=7, model="gat", layer_dependency=True).layer_dependency is True
    for x in (s, b):
        x.reset_draw(seed=3, step=17)
        assert x.draw_step() == 17
        for name in ("sample_blocks", "sample_blocks_static", "finish_static", "check_errors", "reset_draw"):
            assert callable(getattr(x, name))
    assert callable(b.exp3)
    WeightedLaborSampler([4], "w", prefetch_node_feats=None)         # (unknown DGL keywords are ignored)
    with pytest.raises(NotImplementedError):                         # the pinned refusal stays: LABOR-0 itself takes no prob
        LaborSampler([4], prob="w")


def test_make_sampler_names():
    _lib()
    from bliss_gnn_amd.fit import BanditLaborSampler, ImportanceLaborSampler, LaborSampler, make_sampler
    s = make_sampler("labor-exp3", [4, 3], eta=0.2, num_steps=11, model="gat")
    assert type(s) is BanditLaborSampler and (s.eta, s.T, s.model, s.draw) == (0.2, 11, "gat", "device") and s.fanouts == [4, 3]
    assert type(make_sampler("labor-exp3", [4], draw="host")) is BanditLaborSampler
    assert type(make_sampler("labor", [4])) is LaborSampler                  # unchanged
    s = make_sampler("labor-2", [4])
    assert type(s) is ImportanceLaborSampler and s.iterations == 2
    for name in ("labor-exp", "labor-exp33", "labor-0"):
        with pytest.raises(ValueError):
            make_sampler(name, [4])
