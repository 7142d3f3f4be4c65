"""CPU suite: the weighted neighbor draw's entry points are exported and bound, refuse bad arguments before any launch (no GPU
is touched), and ``fit.NeighborSampler(prob=...)`` / ``fit.BanditNeighborSampler`` / ``make_sampler("neighbor-exp3", ...)`` check
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
    for n in ("bliss_wneighbor_layer", "bliss_wneighbor_scratch_bytes"):
        assert hasattr(raw, n), n
    # bliss_neighbor_layer's arguments + mode, prob, eta, 1 - eta, keys_out
    assert len(_l.SIGNATURES["bliss_wneighbor_layer"]) == len(_l.SIGNATURES["bliss_neighbor_layer"]) + 5 == 20
    assert _l.lib.bliss_wneighbor_layer.restype is C.c_int
    assert "bliss_wneighbor_scratch_bytes" in _l.SPECIAL_SIGNATURES
    assert len(_l.lib.bliss_wneighbor_scratch_bytes.argtypes) == 3 and _l.lib.bliss_wneighbor_scratch_bytes.restype is C.c_int64
    assert (_l.WN_RAW, _l.WN_EXP3) == (0, 1)


def test_scratch_bytes():
    lib, E = _lib().lib, _lib().EINVAL
    f = lib.bliss_wneighbor_scratch_bytes
    assert f(0, 4, 4) == E and f(10, 0, 4) == E and f(-1, 4, 4) == E and f(10, -2, 4) == E and f(10, 4, -1) == E
    assert f(10, 4, 2 ** 31) == E                                    # int32 edge positions
    for v in (1, 32 * 1024, 32 * 1024 + 1, 32 * 1024 + 37, 6000):
        words = -(-(-(-v // 32)) // 1024) * 1024                     # the bitmap, whole tiles of 1024 words
        prev_s = 0
        for cap_s in (1, 7, 1025):
            prev_e = 0
            for n_edges in (0, 1, 9, 4096):
                n = f(v, cap_s, n_edges)
                # tickets, bitmap, tile counts, a two-word record per seed, a staged key per position
                assert n % 16 == 0 and n >= 4 * (16 + words + words // 1024 + 2 * cap_s + n_edges)
                assert n >= lib.bliss_neighbor_scratch_bytes(v, cap_s)
                assert n >= prev_e                                   # monotone in every argument
                prev_e = n
            assert prev_e >= prev_s
            prev_s = prev_e
    prev = 0
    for v in range(1, 200000, 997):                                  # monotone in |V|
        n = f(v, 7, 9)
        assert n >= prev
        prev = n


def test_layer_refuses_bad_arguments_before_any_launch():
    _l = _lib()
    lib, E = _l.lib, _l.EINVAL
    buf = (C.c_int64 * 64)()                                         # 16-byte aligned stand-in for every device pointer
    p = C.addressof(buf)
    assert p % 16 == 0

    def call(g=None, seeds=p, n_seeds=1, n_dev=0, cap_s=4, fanout=2, ov=0, step=p, bump=1, mode=0, prob=p, eta=0.4, ome=0.6,
             keys_out=0, ws=None, out=None, scratch=p, **kw):
        gg = _l.Graph(p, p, 0, 10, 100) if g is None else g
        w = _l.LayerWs() if ws is None else ws
        if ws is None:
            w.counts, w.seg_ptr, w.kept_nid, w.kept_map, w.cap_k = p, p, p, p, 8
        o = _l.BlockOut(p, p, p, p, p, p, p, 0, 0, 0, 16) if out is None else out
        for k, v in kw.items():
            setattr(w if hasattr(w, k) else o, k, v)
        return lib.bliss_wneighbor_layer(C.byref(gg) if g != 0 else None, seeds, n_seeds, n_dev, cap_s, fanout, ov, 5, step, 0, bump,
                                         mode, prob, eta, ome, keys_out, C.byref(w) if ws != 0 else None,
                                         C.byref(o) if out != 0 else None, scratch, 0)

    for mode in (0, 1):
        kw = dict(mode=mode)
        assert call(g=0, **kw) == E and call(ws=0, **kw) == E and call(out=0, **kw) == E
        assert call(seeds=0, **kw) == E and call(scratch=0, **kw) == E
        assert call(cap_s=0, **kw) == E and call(cap_s=-3, **kw) == E
        assert call(fanout=0, **kw) == E
        assert call(prob=0, **kw) == E and call(prob=p + 1, **kw) == E            # the probabilities: NULL, misaligned bf16
        assert call(keys_out=p + 2, **kw) == E and call(ov=p + 1, bump=0, **kw) == E   # misaligned uint32 arrays
    for mode in (-1, 2, 2 ** 31 - 1, -2 ** 31):
        assert call(mode=mode) == E
    assert call(mode=1, eta=-0.1) == E and call(mode=1, ome=-0.5) == E and call(mode=1, eta=float("nan")) == E
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


def test_keywords_of_the_samplers():
    _lib()
    import torch

    import bliss_gnn_amd as bg
    from bliss_gnn_amd.fit import BanditNeighborSampler, NeighborSampler, make_sampler
    assert bg.BanditNeighborSampler is BanditNeighborSampler and issubclass(BanditNeighborSampler, bg.BanditLadiesSampler)
    s = NeighborSampler([4, 4], draw="device", prob="w")
    assert s.prob == "w" and s.draw == "device" and NeighborSampler([4]).prob is None
    assert NeighborSampler([4], prob=None, draw="host").prob is None
    with pytest.raises(NotImplementedError):                         # (the keyword used to be swallowed: a uniform draw)
        NeighborSampler([4, 4], prob="w")
    with pytest.raises(NotImplementedError):
        NeighborSampler([4, 4], draw="host", prob=torch.ones(3))
    b = BanditNeighborSampler([5, 3], eta=0.2, model="gat", seed=9)
    assert b.draw == "device" and b.eta == 0.2 and b.model == "gat" and b.fanouts == [5, 3] and b.nodes_per_layer == [5, 3]
    assert b.draw_step() == 0 and b.exp3_weights is None and b._engine is None
    b.reset_draw(seed=3, step=17)
    assert b.draw_step() == 17
    for name in ("sample_blocks", "sample_blocks_static", "finish_static", "check_errors", "exp3"):
        assert callable(getattr(b, name))
    assert BanditNeighborSampler([4]).eta == 0.4 and BanditNeighborSampler([4]).T == 5000
    m = make_sampler("neighbor-exp3", [4, 3], eta=0.3, model="gat")
    assert type(m) is BanditNeighborSampler and m.eta == 0.3 and m.model == "gat" and m.fanouts == [4, 3]
    assert type(make_sampler("neighbor", [4])) is NeighborSampler    # (the other names are unchanged)
    assert type(make_sampler("bandit", [4])) is bg.BanditLadiesSampler
    with pytest.raises(ValueError):
        make_sampler("neighbor-exp", [4])
