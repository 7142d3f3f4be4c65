"""CPU suite: the entry points of the draws with replacement (csrc/replace_draw.hip) are exported and bound,
refuse bad arguments before any launch (no GPU is touched), and the samplers check their ``replace`` / ``draw`` keywords."""
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
    for n in ("bliss_neighbor_replace_layer", "bliss_neighbor_replace_scratch_bytes", "bliss_multinomial_draw_replace",
              "bliss_multinomial_draw_replace_scratch_bytes"):
        assert hasattr(raw, n), n
    # bliss_neighbor_layer's arguments + prob_pos, picks_out; bliss_multinomial_draw's without cand_nid and keys, + picks_out
    assert len(_l.SIGNATURES["bliss_neighbor_replace_layer"]) == len(_l.SIGNATURES["bliss_neighbor_layer"]) + 2 == 17
    assert len(_l.SIGNATURES["bliss_multinomial_draw_replace"]) == len(_l.SIGNATURES["bliss_multinomial_draw"]) - 1 == 13
    assert _l.lib.bliss_neighbor_replace_layer.restype is C.c_int and _l.lib.bliss_multinomial_draw_replace.restype is C.c_int
    for n, k in (("bliss_neighbor_replace_scratch_bytes", 2), ("bliss_multinomial_draw_replace_scratch_bytes", 1)):
        assert n in _l.SPECIAL_SIGNATURES
        assert len(getattr(_l.lib, n).argtypes) == k and getattr(_l.lib, n).restype is C.c_int64
    assert _l.NR_MAX_FANOUT == 1024
    text = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "bliss_gnn.h")).read()
    assert "#define BLISS_NR_MAX_FANOUT 1024" in text


def test_scratch_bytes():
    lib, E = _lib().lib, _lib().EINVAL
    f = lib.bliss_neighbor_replace_scratch_bytes
    assert f(0, 4) == E and f(10, 0) == E and f(-1, 4) == E and f(10, -2) == E
    for v in (1, 32 * 1024, 32 * 1024 + 1, 6000, 250000):
        words = -(-(-(-v // 32)) // 1024) * 1024                     # the bitmap, whole tiles of 1024 words
        n = f(v, 7)
        assert n % 16 == 0 and n >= 4 * (16 + words + words // 1024) and n == f(v, 100000)   # (nothing is sized by cap_s)
        assert n == lib.bliss_neighbor_scratch_bytes(v, 7)           # the uniform draw's words: one scratch could serve both
    m = lib.bliss_multinomial_draw_replace_scratch_bytes
    assert m(0) == E and m(-5) == E
    prev = 0
    for c in (1, 7, 1024, 1025, 20000, 250000):
        n = m(c)
        # a header, 256 maxima, an inclusive prefix per 1024-candidate chunk, a prefix per candidate: all but the maxima 64-bit
        assert n % 16 == 0 and n >= 8 * (3 + 128 + -(-c // 1024) + c) and n > prev
        prev = n


def test_neighbor_replace_layer_refuses_bad_arguments_before_any_launch():
    _l = _lib()
    lib, E = _l.lib, _l.EINVAL
    buf = (C.c_int64 * 64)()                                         # 16-byte aligned stand-in for every device pointer
    p = C.addressof(buf)
    assert p % 16 == 0

    def call(g=None, seeds=p, n_seeds=1, n_dev=0, cap_s=4, fanout=2, r_ov=0, step=p, bump=1, prob=0, picks=0, ws=None, out=None,
             scratch=p, **kw):
        gg = _l.Graph(p, p, 0, 10, 100) if g is None else g
        w = _l.LayerWs() if ws is None else ws
        if ws is None:
            w.counts, w.seg_ptr, w.kept_nid, w.kept_map, w.cap_k = p, p, p, p, 8
        o = _l.BlockOut(p, p, p, p, p, p, p, 0, 0, 0, 16) if out is None else out
        for k, v in kw.items():
            setattr(w if hasattr(w, k) else o, k, v)
        return lib.bliss_neighbor_replace_layer(C.byref(gg) if g != 0 else None, seeds, n_seeds, n_dev, cap_s, fanout, r_ov, 5, step, 0,
                                                bump, prob, picks, C.byref(w) if ws != 0 else None, C.byref(o) if out != 0 else None,
                                                scratch, 0)

    for prob in (0, p):                                              # uniform and with probabilities
        kw = dict(prob=prob)
        assert call(g=0, **kw) == E and call(ws=0, **kw) == E and call(out=0, **kw) == E
        assert call(seeds=0, **kw) == E and call(scratch=0, **kw) == E
        assert call(cap_s=0, **kw) == E and call(cap_s=-3, **kw) == E
        assert call(fanout=0, **kw) == E                             # the fanout limit: 1 .. BLISS_NR_MAX_FANOUT, or negative
        assert call(fanout=1025, **kw) == E and call(fanout=2 ** 31 - 1, **kw) == E
    assert call(prob=p + 1) == E                                     # alignment to the element size: bf16 ...
    assert call(r_ov=p + 4, bump=0) == E and call(r_ov=p + 1) == E   # ... uint64 ...
    assert call(picks=p + 2) == E and call(picks=p + 1) == E         # ... int32
    assert call(g=_l.Graph(p, p, 0, 10, 2 ** 31)) == E               # int32 edge positions
    assert call(g=_l.Graph(p, p, 0, 10, -1)) == E and call(g=_l.Graph(p, p, 0, 0, 100)) == E
    assert call(g=_l.Graph(0, p, 0, 10, 100)) == E and call(g=_l.Graph(p, 0, 0, 10, 100)) == E
    assert call(scratch=p + 8) == E                                  # misaligned scratch
    assert call(n_seeds=-1, n_dev=0) == E                            # a device-side count needs its pointer
    assert call(step=0) == E and call(step=0, bump=0) == E           # the hash needs the step counter ...
    assert call(step=0, r_ov=p, bump=1) == E                         # ... and so does the bump
    for field in ("counts", "seg_ptr", "kept_nid", "kept_map", "indptr", "src", "dst", "pos", "eid", "edge_weights", "q_ij"):
        assert call(**{field: 0}) == E, field
    assert call(cap_k=0) == E and call(cap_b=-1) == E


def test_multinomial_draw_replace_refuses_bad_arguments_before_any_launch():
    _l = _lib()
    lib, E = _l.lib, _l.EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def call(pb=p, counts=p, cap_c=8, fanout=4, r_ov=0, step=p, bump=1, scratch=p, drawn=p, picks=0):
        return lib.bliss_multinomial_draw_replace(pb, counts, cap_c, fanout, r_ov, 5, step, 0, bump, scratch, drawn, picks, 0)

    assert call(pb=0) == E and call(counts=0) == E and call(scratch=0) == E and call(drawn=0) == E
    assert call(fanout=-1) == E and call(cap_c=0) == E and call(cap_c=-4) == E
    assert call(scratch=p + 8) == E                                  # misaligned scratch
    assert call(step=0) == E and call(step=0, bump=0) == E           # the hash needs the step counter ...
    assert call(step=0, r_ov=p, bump=1) == E                         # ... and so does the bump
    assert call(r_ov=p + 4) == E and call(picks=p + 2) == E and call(drawn=p + 2) == E


def test_keywords_of_the_samplers():
    _lib()
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.fit import (BanditLaborSampler, BanditNeighborSampler, LaborSampler, NeighborSampler, make_sampler)
    FAN = [8, 4]
    for cls in (bg.LadiesSampler, bg.BanditLadiesSampler):
        s = cls(FAN, draw="device-replace")
        assert s.draw == "device" and s.replace is True              # every draw == "device" check holds for it
        assert cls(FAN, draw="device").replace is False and cls(FAN).replace is False
        assert cls(FAN, replace=True).draw == "host"                 # (the host draw: torch.multinomial with replacement)
        with pytest.raises(NotImplementedError, match="device-replace"):     # the old refusal stands and names the spelling
            cls(FAN, replace=True, draw="device")
        with pytest.raises(ValueError):
            cls(FAN, draw="device-replaced")
    for cls in (bg.PoissonLadiesSampler, bg.PoissonBanditLadiesSampler):
        with pytest.raises(ValueError, match="device-replace"):
            cls(FAN, draw="device-replace")
    s = NeighborSampler(FAN, draw="device", replace=True)
    assert s.replace is True and s.draw == "device" and s.prob is None
    assert NeighborSampler(FAN, draw="device", replace=True, prob="w").prob == "w"
    assert NeighborSampler(FAN).replace is False and NeighborSampler(FAN, draw="device").replace is False
    assert NeighborSampler([1024, -1], draw="device", replace=True).fanouts == [1024, -1]
    with pytest.raises(NotImplementedError, match="replace"):        # (the keyword used to be swallowed: a draw without replacement)
        NeighborSampler(FAN, replace=True)
    with pytest.raises(NotImplementedError, match="replace"):
        NeighborSampler(FAN, draw="host", replace=True)
    for fan in ([8, 1025], [0, 4]):
        with pytest.raises(ValueError, match="1024"):
            NeighborSampler(fan, draw="device", replace=True)
    with pytest.raises(ValueError):
        NeighborSampler(FAN, draw="device-replace")
    assert LaborSampler(FAN).replace is False
    for cls in (BanditNeighborSampler, BanditLaborSampler):
        with pytest.raises(NotImplementedError, match="at most once per block"):
            cls(FAN, replace=True)
        assert cls(FAN, replace=False).draw == "device"
    for name, cls in (("ladies", bg.LadiesSampler), ("bandit", bg.BanditLadiesSampler)):
        m = make_sampler(name, FAN, draw="device", replace=True)
        assert type(m) is cls and m.draw == "device" and m.replace is True
        with pytest.raises(ValueError, match="draw='device'"):
            make_sampler(name, FAN, replace=True)
        assert make_sampler(name, FAN, draw="device").replace is False
    m = make_sampler("neighbor", FAN, draw="device", replace=True)
    assert type(m) is NeighborSampler and m.replace is True
    with pytest.raises(NotImplementedError):
        make_sampler("neighbor", FAN, replace=True)                  # (draw="host": the sampler's own refusal)
    for name in ("poisson-ladies", "poisson-bandit", "poisson-bandit-keyed", "labor", "labor-2", "neighbor-exp3", "labor-exp3", "full"):
        with pytest.raises(ValueError, match="replace"):
            make_sampler(name, FAN, draw="device", replace=True)
        make_sampler(name, FAN)                                      # (the names themselves are unchanged)
