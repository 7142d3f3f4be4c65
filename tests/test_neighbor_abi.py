"""CPU suite: the device-side neighbor sampler's entry points are exported and bound, refuse bad arguments before any launch
(no GPU is touched), and the ``draw=`` keyword reaches ``fit.NeighborSampler``."""
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
    for n in ("bliss_neighbor_layer", "bliss_neighbor_scratch_bytes"):
        assert hasattr(raw, n), n
    assert len(_l.SIGNATURES["bliss_neighbor_layer"]) == 15
    assert "bliss_neighbor_scratch_bytes" in _l.SPECIAL_SIGNATURES
    assert len(_l.lib.bliss_neighbor_scratch_bytes.argtypes) == 2 and _l.lib.bliss_neighbor_scratch_bytes.restype is C.c_int64


def test_scratch_bytes():
    lib, E = _lib().lib, _lib().EINVAL
    assert lib.bliss_neighbor_scratch_bytes(0, 4) == E and lib.bliss_neighbor_scratch_bytes(10, 0) == E
    for v in (1, 32 * 1024, 32 * 1024 + 1, 6000):
        words = -(-(-(-v // 32)) // 1024) * 1024                     # the bitmap, whole tiles of 1024 words
        n = lib.bliss_neighbor_scratch_bytes(v, 7)
        assert n % 16 == 0 and n >= 4 * (16 + words + words // 1024)


def test_layer_refuses_bad_arguments_before_any_launch():
    _l = _lib()
    lib, E = _l.lib, _l.EINVAL
    buf = (C.c_int64 * 64)()                                         # 16-byte aligned stand-in for every device pointer
    p = C.addressof(buf)
    assert p % 16 == 0

    def call(g=None, seeds=p, n_seeds=1, n_dev=0, cap_s=4, fanout=2, ov=0, step=p, bump=1, ws=None, out=None, scratch=p, **kw):
        gg = _l.Graph(p, p, 0, 10, 100) if g is None else g
        w = _l.LayerWs() if ws is None else ws
        if ws is None:
            w.counts, w.seg_ptr, w.kept_nid, w.kept_map, w.cap_k = p, p, p, p, 8
        o = _l.BlockOut(p, p, p, p, p, p, p, 0, 0, 0, 16) if out is None else out
        for k, v in kw.items():
            setattr(w if hasattr(w, k) else o, k, v)
        return lib.bliss_neighbor_layer(C.byref(gg) if g != 0 else None, seeds, n_seeds, n_dev, cap_s, fanout, ov, 5, step, 0, bump,
                                        C.byref(w) if ws != 0 else None, C.byref(o) if out != 0 else None, scratch, 0)

    assert call(g=0) == E and call(ws=0) == E and call(out=0) == E
    assert call(seeds=0) == E and call(scratch=0) == E
    assert call(cap_s=0) == E and call(cap_s=-3) == E
    assert call(fanout=0) == E
    assert call(g=_l.Graph(p, p, 0, 10, 2 ** 31)) == E               # int32 edge positions
    assert call(g=_l.Graph(0, p, 0, 10, 100)) == E and call(g=_l.Graph(p, 0, 0, 10, 100)) == E
    assert call(scratch=p + 8) == E                                  # misaligned scratch
    assert call(n_seeds=-1, n_dev=0) == E                            # a device-side count needs its pointer
    assert call(step=0) == E and call(step=0, ov=p, bump=1) == E     # the hash and the bump need the step counter
    for field in ("counts", "seg_ptr", "kept_nid", "kept_map", "indptr", "src", "dst", "pos", "eid", "edge_weights", "q_ij"):
        assert call(**{field: 0}) == E, field
    assert call(cap_k=0) == E


def test_draw_keyword_of_the_neighbor_sampler():
    _lib()
    from bliss_gnn_amd.fit import NeighborSampler, make_sampler
    assert NeighborSampler([4, 4]).draw == "host"
    assert make_sampler("neighbor", [4]).draw == "host"
    assert make_sampler("neighbor", [4], draw="device").draw == "device"
    s = NeighborSampler([4, 4], seed=9, draw="device")
    assert s.draw_step() == 0 and s._engine is None and s.nodes_per_layer == [4, 4]
    s.reset_draw(seed=3, step=17)
    assert s.draw_step() == 17
    with pytest.raises(ValueError):
        NeighborSampler([4], draw="bogus")
    with pytest.raises(NotImplementedError):
        NeighborSampler([4]).sample_blocks_static(None, None)
