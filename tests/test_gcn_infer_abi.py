"""CPU suite: bliss_gcn_infer_src_norms / bliss_gcn_infer_spmm (GCN full-neighbour inference off the CSC)
are exported, bound, and validate their arguments on the host -- a refused call launches nothing, so this runs without a GPU."""
import ctypes as C

import pytest


def _args(lib_mod, buf):
    """A descriptor both calls accept (never launched here: each test breaks one field first)."""
    p = (C.addressof(buf) + 15) & ~15                          # 16-byte aligned inside the buffer
    t = lib_mod.GcnInfer()
    t.indptr, t.indices, t.n_nodes, t.batch_size = p, p, 1000, 128
    t.row0, t.n_rows, t.edge0, t.n_edges, t.ns = 256, 384, 5000, 7000, p
    t.t_indptr, t.t_edge, t.temp, t.temp_bytes = p, p, p, 1 << 30
    t.h, t.h_stride, t.dim, t.out, t.out_stride = p, 64, 64, p, 64
    return t, p


@pytest.fixture(scope="module")
def env():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    buf = (C.c_int64 * 66)()
    return _lib, buf


CALLS = ("bliss_gcn_infer_src_norms", "bliss_gcn_infer_spmm")


def test_symbols_are_exported_and_bound(env):
    _lib, _ = env
    raw = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert hasattr(raw, name)
        assert _lib.SIGNATURES[name] == [C.POINTER(_lib.GcnInfer), C.c_void_p]
        assert getattr(_lib.lib, name).argtypes == [C.POINTER(_lib.GcnInfer), C.c_void_p]
    assert hasattr(raw, "bliss_gcn_infer_chunk_edges")
    # the struct as the header lays it out: 8-byte members aligned, 18 fields
    G = _lib.GcnInfer
    assert C.sizeof(G) == 128 and len(G._fields_) == 18
    assert (G.row0.offset, G.edge0.offset, G.n_edges.offset, G.ns.offset, G.temp_bytes.offset) == (24, 32, 40, 48, 80)
    assert (G.h.offset, G.dim.offset, G.out.offset, G.out_stride.offset) == (88, 104, 112, 120)


def test_chunk_length_is_the_block_paths(env):
    _lib, _ = env
    for n in (0, 1, 15, 16, 17, 49999, 50000, 50001, 199999, 200000, 200001, 2 ** 31 - 1):
        assert _lib.lib.bliss_gcn_infer_chunk_edges(n) == _lib.lib.bliss_spmm_chunk_edges(n), n


@pytest.mark.parametrize("call", CALLS)
def test_null_descriptor_and_graph_pointers(env, call):
    _lib, buf = env
    fn = getattr(_lib.lib, call)
    assert fn(None, 0) == _lib.EINVAL
    for field in ("indptr", "indices", "ns"):
        t, _ = _args(_lib, buf)
        setattr(t, field, None)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field


@pytest.mark.parametrize("call", CALLS)
def test_counts_batches_and_the_edge_limit(env, call):
    _lib, buf = env
    fn = getattr(_lib.lib, call)
    bad = (("n_nodes", 0), ("n_nodes", -5), ("batch_size", 0), ("batch_size", -1), ("row0", -128), ("n_rows", -1), ("n_rows", 1000),
           ("row0", 255), ("row0", 257),                     # a range starts on a batch boundary ...
           ("n_rows", 383), ("n_rows", 385),                 # ... and ends on one (or at the last node)
           ("edge0", -1), ("n_edges", -1), ("n_edges", 2 ** 31), ("n_edges", 2 ** 40))
    for field, value in bad:
        t, _ = _args(_lib, buf)
        setattr(t, field, value)
        assert fn(C.byref(t), 0) == _lib.EINVAL, (field, value)


@pytest.mark.parametrize("call", CALLS)
def test_alignment_of_the_graph_arrays(env, call):
    _lib, buf = env
    fn = getattr(_lib.lib, call)
    for field, off in (("indptr", 4), ("indices", 2), ("ns", 2)):
        t, p = _args(_lib, buf)
        setattr(t, field, p + off)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field


def test_src_norms_scratch(env):
    _lib, buf = env
    fn = _lib.lib.bliss_gcn_infer_src_norms
    for field in ("t_indptr", "t_edge", "temp"):
        t, p = _args(_lib, buf)
        setattr(t, field, None)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field
        t, p = _args(_lib, buf)
        setattr(t, field, p + 2)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field
    for nbytes in (0, 3 * 7000 * 4):                                     # below the three key / value arrays alone
        t, p = _args(_lib, buf)
        t.temp_bytes = nbytes
        assert fn(C.byref(t), 0) == _lib.EINVAL, nbytes


def test_spmm_rows_and_strides(env):
    _lib, buf = env
    fn = _lib.lib.bliss_gcn_infer_spmm
    for field, value in (("h", None), ("out", None), ("dim", 0), ("dim", -4), ("h_stride", 63), ("out_stride", 63)):
        t, p = _args(_lib, buf)
        setattr(t, field, value)
        assert fn(C.byref(t), 0) == _lib.EINVAL, (field, value)
    for field in ("h", "out"):                                          # bf16 data at an odd address
        t, p = _args(_lib, buf)
        setattr(t, field, p + 1)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field


@pytest.mark.parametrize("call", CALLS)
def test_empty_range_launches_nothing(env, call):
    """n_rows = 0 returns 0 without touching a device (there is none here) and without scratch."""
    _lib, buf = env
    t, _ = _args(_lib, buf)
    t.n_rows, t.n_edges = 0, 0
    t.ns = t.t_indptr = t.t_edge = t.temp = None
    t.temp_bytes = 0
    assert getattr(_lib.lib, call)(C.byref(t), 0) == 0


def test_a_range_may_end_at_the_last_node(env):
    """row0 + n_rows == n_nodes closes the short last batch (without edges there is nothing to launch: 0); one row less cuts it."""
    _lib, buf = env
    t, _ = _args(_lib, buf)
    t.row0, t.n_rows, t.n_edges = 896, 104, 0
    assert _lib.lib.bliss_gcn_infer_src_norms(C.byref(t), 0) == 0
    t.n_rows = 103
    assert _lib.lib.bliss_gcn_infer_src_norms(C.byref(t), 0) == _lib.EINVAL
