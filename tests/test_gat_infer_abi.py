"""CPU suite: bliss_gat_infer_fwd (GATv2 full-neighbour inference off the CSC) is exported, bound, and
validates its arguments on the host -- a refused call launches nothing, so this runs without a GPU."""
import ctypes as C

import pytest


def _args(lib_mod, buf):
    """A descriptor every check passes (never launched here: each test breaks one field first)."""
    p = (C.addressof(buf) + 15) & ~15                          # 16-byte aligned inside the buffer
    t = lib_mod.GatInfer()
    t.indptr, t.indices, t.row0, t.n_rows, t.n_edges = p, p, 0, 4, 1000
    t.feat, t.feat_stride, t.attn, t.heads, t.head_dim, t.negative_slope = p, 64, p, 4, 16, 0.2
    t.res, t.res_stride, t.act = p, 64, 1
    t.out, t.out_stride = p, 64
    t.wg_row, t.n_wg_dev, t.cap_wg, t.row_ws, t.seg_part, t.err = p, p, 4 + 1000 // 256, p, p, p
    return t, p


@pytest.fixture(scope="module")
def env():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    buf = (C.c_int64 * 66)()
    return _lib, buf


def test_symbol_is_exported_and_bound(env):
    _lib, _ = env
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "bliss_gat_infer_fwd")
    assert _lib.SIGNATURES["bliss_gat_infer_fwd"] == [C.POINTER(_lib.GatInfer), C.c_void_p]
    assert _lib.lib.bliss_gat_infer_fwd.argtypes == [C.POINTER(_lib.GatInfer), C.c_void_p]
    # the struct as the header lays it out: 8-byte members aligned, 22 fields
    assert C.sizeof(_lib.GatInfer) == 160 and _lib.GatInfer.n_edges.offset == 24 and _lib.GatInfer.err.offset == 152


def _call(_lib, t):
    return _lib.lib.bliss_gat_infer_fwd(C.byref(t), 0)


def test_null_descriptor(env):
    _lib, _ = env
    assert _lib.lib.bliss_gat_infer_fwd(None, 0) == _lib.EINVAL


@pytest.mark.parametrize("field", ["indptr", "indices", "feat", "out", "attn"])
def test_null_pointers(env, field):
    _lib, buf = env
    t, _ = _args(_lib, buf)
    setattr(t, field, None)
    assert _call(_lib, t) == _lib.EINVAL


@pytest.mark.parametrize("heads,dim", [(0, 16), (9, 16), (4, 0), (8, 129), (2, 258), (1, 257), (8, 132)])
def test_heads_and_unsupported_shapes(env, heads, dim):
    """heads outside 1 .. 8; (H, D) beyond bliss_gat_fused_supported: more than 256 columns with head_dim % 4 != 0, more than 1024."""
    _lib, buf = env
    t, _ = _args(_lib, buf)
    t.heads, t.head_dim = heads, dim
    t.feat_stride = t.out_stride = t.res_stride = 2048
    if heads > 0 and dim > 0:
        assert not _lib.lib.bliss_gat_fused_supported(heads, dim) or heads > 8
    assert _call(_lib, t) == _lib.EINVAL


def test_negative_counts_and_edge_limit(env):
    _lib, buf = env
    for field, value in (("n_rows", -1), ("row0", -1), ("n_edges", -1), ("n_edges", 2 ** 31), ("n_edges", 2 ** 40), ("act", 2), ("act", -1)):
        t, _ = _args(_lib, buf)
        setattr(t, field, value)
        assert _call(_lib, t) == _lib.EINVAL, (field, value)


def test_alignment_and_strides(env):
    _lib, buf = env
    for field in ("feat", "out", "res", "attn"):                       # bf16 data at an odd address
        t, p = _args(_lib, buf)
        setattr(t, field, p + 1)
        assert _call(_lib, t) == _lib.EINVAL, field
    for field in ("feat_stride", "out_stride", "res_stride"):          # a row shorter than heads * head_dim
        t, p = _args(_lib, buf)
        setattr(t, field, 63)
        assert _call(_lib, t) == _lib.EINVAL, field
    t, p = _args(_lib, buf)
    t.indptr = p + 4                                                   # int64 offsets not 8-byte aligned
    assert _call(_lib, t) == _lib.EINVAL
    t, p = _args(_lib, buf)
    t.indices = p + 2
    assert _call(_lib, t) == _lib.EINVAL
    # a width above 256 runs on 8-byte loads: feat / attn 8-byte aligned and the row stride a multiple of 4
    for field, value in (("feat", 4), ("attn", 2), ("feat_stride", 1026)):
        t, p = _args(_lib, buf)
        t.heads, t.head_dim = 4, 256
        t.feat_stride = t.out_stride = t.res_stride = 1024
        setattr(t, field, (p + value) if field != "feat_stride" else value)
        assert _call(_lib, t) == _lib.EINVAL, field


def test_scratch_is_checked_when_there_are_rows(env):
    _lib, buf = env
    for field in ("wg_row", "n_wg_dev", "row_ws", "seg_part"):
        t, p = _args(_lib, buf)
        setattr(t, field, None)
        assert _call(_lib, t) == _lib.EINVAL, field
    t, p = _args(_lib, buf)
    t.wg_row = p + 8                                                   # 16-byte descriptors
    assert _call(_lib, t) == _lib.EINVAL
    t, p = _args(_lib, buf)
    t.cap_wg = 4 + 1000 // 256 - 1                                     # one below n_rows + n_edges / segment
    assert _call(_lib, t) == _lib.EINVAL


def test_empty_range_launches_nothing(env):
    """n_rows = 0 returns 0 without touching a device (there is none here) and without scratch."""
    _lib, buf = env
    t, _ = _args(_lib, buf)
    t.n_rows, t.n_edges = 0, 0
    t.wg_row = t.n_wg_dev = t.row_ws = t.seg_part = t.err = None
    assert _call(_lib, t) == 0
