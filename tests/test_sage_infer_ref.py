"""CPU suite: SAGE.inference(path="csc") without a GPU.

tests/sage_infer_ref.py, the NumPy restatement of the two reductions of csrc/sage_infer.hip, equals a plain per-edge loop on the
multigraph of gcn_infer_ref at batch sizes 1, 7, 60 and 100; a designed row shows that the chunk order is part of the mean's
contract.  bliss_sage_infer_spmm is exported, bound, and validates its arguments on the host -- a refused call launches nothing.
SAGE.INFERENCE_PATHS and csc_refusal answer without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import gcn_infer_ref as gref
import sage_infer_ref as ref


def _feats(V, dim, seed=1):
    x = torch.randn(V, dim, generator=torch.Generator().manual_seed(seed)).bfloat16().float().numpy()
    x[3, 0], x[5, 0] = -0.0, 0.0                                         # signed zeros among the values
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("bs", [1, 7, 60, 100])
def test_mean_restatement_equals_the_edge_loop(bs):
    ip, ix = gref.small_multigraph()
    h = _feats(60, 5)
    got, want = ref.mean_f32(ip, ix, bs, h), ref.mean_edge_loop(ip, ix, bs, h)
    assert np.array_equal(_bits(got), _bits(want))
    deg = np.diff(ip)
    assert not got[deg == 0].any() and not np.signbit(got[deg == 0]).any()          # rows without edges: +0
    f64 = np.zeros((60, 5))
    np.add.at(f64, gref.edge_dst(ip), h[ix].astype(np.float64))
    f64 /= np.maximum(deg, 1)[:, None]
    assert np.abs(got - f64).max() <= 2.0 ** -7 * np.abs(h).max()                  # (sanity: it is the mean)


@pytest.mark.parametrize("bs", [1, 7, 60, 100])
def test_max_restatement_equals_the_edge_loop(bs):
    ip, ix = gref.small_multigraph()
    h = _feats(60, 5)
    got, want = ref.max_f32(ip, ix, h), ref.max_edge_loop(ip, ix, h)
    assert np.array_equal(_bits(got), _bits(want))
    deg = np.diff(ip)
    seg = np.full((60, 5), -np.inf)
    np.maximum.at(seg, gref.edge_dst(ip), h[ix].astype(np.float64))
    assert np.array_equal(got[deg > 0].astype(np.float64), seg[deg > 0]) and not _bits(got[deg == 0]).any()
    assert bs >= 1                                                                  # (the batch structure does not enter the value)


def test_signed_zeros():
    """-0.0 then +0.0 in one row: the first edge wins the max; the mean starts from +0 and is +0."""
    ip = np.array([0, 2, 4], dtype=np.int64)
    ix = np.array([0, 1, 1, 0], dtype=np.int32)
    h = np.array([[-0.0], [0.0]], dtype=np.float32)
    mx = ref.max_f32(ip, ix, h)
    assert _bits(mx)[0, 0] == 0x80000000 and _bits(mx)[1, 0] == 0
    assert not _bits(ref.mean_f32(ip, ix, 2, h)).any()
    assert np.array_equal(_bits(mx), _bits(ref.max_edge_loop(ip, ix, h)))
    assert np.array_equal(_bits(ref.mean_f32(ip, ix, 2, h)), _bits(ref.mean_edge_loop(ip, ix, 2, h)))


def test_the_designed_row_needs_the_chunk_order():
    ip, ix, h = ref.designed_graph()
    r = ref.DESIGNED_ROW
    deg = int(ip[r + 1] - ip[r])
    assert deg >= 40 and int(ip[r]) % 16 != 0                                       # at least 40 edges, starting mid-chunk
    for bs in (2, 4, 100):
        assert gref.batch_chunks(ip, bs)[0] == 16 and int(gref.batch_table(ip, bs)[1][0]) == 0
    terms = h[ix[ip[r]:ip[r + 1]], 0]
    plain = np.add.accumulate(terms, dtype=np.float32)[-1]
    assert plain == 0.0                                                             # edge order: every 1.0 is absorbed by 2^24
    rule = ref.mean_f32(ip, ix, 4, h)
    want = gref.rbf(np.array([np.float32(28.0) * (np.float32(1.0) / np.float32(40.0))], dtype=np.float32))[0]
    assert rule[r, 0] == want and rule[r, 1] == 1.0
    assert np.array_equal(_bits(rule), _bits(ref.mean_edge_loop(ip, ix, 4, h)))
    flat = ref.mean_f32(ip, ix, 4, h, chunks=False)                                 # a restatement that ignores the chunks ...
    assert flat[r, 0] == 0.0 and _bits(flat)[r, 0] != _bits(rule)[r, 0]             # ... rounds to other bf16 bits: it fails here
    with pytest.raises(AssertionError):
        assert np.array_equal(_bits(flat), _bits(ref.mean_edge_loop(ip, ix, 4, h)))
    others = [i for i in range(4) if i != r]
    assert np.array_equal(_bits(flat[others]), _bits(rule[others]))                 # rows inside one chunk do not care


# ---------------------------------------------------------------------------------------------- the C ABI
def _args(lib_mod, buf):
    """A descriptor the call accepts (never launched here: each test breaks one field first)."""
    p = (C.addressof(buf) + 15) & ~15                          # 16-byte aligned inside the buffer
    t = lib_mod.SageInfer()
    t.indptr, t.indices, t.n_nodes, t.batch_size = p, p, 1000, 128
    t.row0, t.n_rows, t.edge0, t.n_edges, t.reduce = 256, 384, 5000, 7000, 0
    t.h, t.h_stride, t.dim, t.out, t.out_stride = p, 64, 64, p, 64
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
    assert hasattr(raw, "bliss_sage_infer_spmm")
    assert _lib.SIGNATURES["bliss_sage_infer_spmm"] == [C.POINTER(_lib.SageInfer), C.c_void_p]
    assert _lib.lib.bliss_sage_infer_spmm.argtypes == [C.POINTER(_lib.SageInfer), C.c_void_p]
    assert (_lib.SAGE_INFER_MEAN, _lib.SAGE_INFER_MAX) == (0, 1)
    # the struct as the header lays it out: 8-byte members aligned, 14 fields
    G = _lib.SageInfer
    assert C.sizeof(G) == 96 and len(G._fields_) == 14
    assert (G.row0.offset, G.edge0.offset, G.n_edges.offset, G.reduce.offset) == (24, 32, 40, 48)
    assert (G.h.offset, G.h_stride.offset, G.dim.offset, G.out.offset, G.out_stride.offset) == (56, 64, 72, 80, 88)


def test_null_descriptor_and_pointers(env):
    _lib, buf = env
    fn = _lib.lib.bliss_sage_infer_spmm
    assert fn(None, 0) == _lib.EINVAL
    for field in ("indptr", "indices", "h", "out"):
        t, _ = _args(_lib, buf)
        setattr(t, field, None)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field


def test_counts_batches_edges_reduce_and_strides(env):
    _lib, buf = env
    fn = _lib.lib.bliss_sage_infer_spmm
    bad = (("n_nodes", 0), ("n_nodes", -5), ("batch_size", 0), ("batch_size", -1), ("row0", -128), ("n_rows", -1), ("n_rows", 1000),
           ("row0", 1024),                                   # past n_nodes
           ("row0", 255), ("row0", 257),                     # a range starts on a batch boundary ...
           ("n_rows", 383), ("n_rows", 385),                 # ... and ends on one (or at the last node)
           ("edge0", -1), ("n_edges", -1), ("n_edges", 2 ** 31), ("n_edges", 2 ** 40),
           ("reduce", -1), ("reduce", 2),
           ("dim", 0), ("dim", -4), ("h_stride", 63), ("out_stride", 63))
    for field, value in bad:
        t, _ = _args(_lib, buf)
        setattr(t, field, value)
        assert fn(C.byref(t), 0) == _lib.EINVAL, (field, value)


def test_alignment_of_the_graph_arrays(env):
    _lib, buf = env
    fn = _lib.lib.bliss_sage_infer_spmm
    for field, off in (("indptr", 4), ("indices", 2)):
        t, p = _args(_lib, buf)
        setattr(t, field, p + off)
        assert fn(C.byref(t), 0) == _lib.EINVAL, field


@pytest.mark.parametrize("reduce", [0, 1])
def test_empty_range_launches_nothing(env, reduce):
    """n_rows = 0 returns 0 without touching a device (there is none here)."""
    _lib, buf = env
    t, _ = _args(_lib, buf)
    t.n_rows, t.n_edges, t.reduce = 0, 0, reduce
    assert _lib.lib.bliss_sage_infer_spmm(C.byref(t), 0) == 0
    t.row0, t.n_rows = 896, 0                                # the empty range in front of the last batch
    assert _lib.lib.bliss_sage_infer_spmm(C.byref(t), 0) == 0


def test_a_range_may_end_at_the_last_node_only_whole(env):
    _lib, buf = env
    t, _ = _args(_lib, buf)
    t.row0, t.n_rows = 896, 103                              # one row short of the last node: cuts the last batch
    assert _lib.lib.bliss_sage_infer_spmm(C.byref(t), 0) == _lib.EINVAL


# ---------------------------------------------------------------------------------------------- the model's interface
def _sage(*a, **kw):
    from bliss_gnn_amd.model import SAGE
    return SAGE(*a, **kw)


def test_inference_paths_and_the_unknown_path(env):
    from bliss_gnn_amd.model import SAGE
    assert SAGE.INFERENCE_PATHS == ("chunks", "blocks", "csc", "auto")
    assert SAGE.csc_max_edges == 1 << 23 and SAGE.csc_spmm_edges == 2 ** 31 - 1 and SAGE.last_inference_path is None
    model = _sage(8, 4, 3, 2, torch.relu, 0.5)
    with pytest.raises(ValueError, match="nope"):
        model.inference(None, path="nope")
    assert model.training and model.last_inference_path is None


class _CpuGraph:
    device = torch.device("cpu")


def test_csc_refusal_on_the_cpu(env):
    x = torch.zeros(10, 8)
    why = _sage(8, 4, 3, 2, torch.relu, 0.5).csc_refusal(_CpuGraph(), x, 128)
    assert why is not None and "bf16" in why and "GPU" in why
    why = _sage(8, 4, 3, 2, torch.relu, 0.5, aggregator_type="pool").csc_refusal(_CpuGraph(), x, 128)
    assert why is not None and 'transforms="tile"' in why
    why = _sage(8, 4, 3, 2, torch.relu, 0.5, transforms="tile", aggregator_type="pool").csc_refusal(_CpuGraph(), x, 128)
    assert why is not None and "bf16" in why and "GPU" in why
    assert "batch_size" in _sage(8, 4, 3, 2, torch.relu, 0.5).csc_refusal(_CpuGraph(), x, 0)


def test_nn_wrapper_checks_its_arguments(env):
    from bliss_gnn_amd.nn import sage_infer_spmm
    ip, ix = torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    h, out = torch.zeros(4, 3, dtype=torch.bfloat16), torch.zeros(4, 3, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="reduce"):
        sage_infer_spmm(ip, ix, 2, 0, 4, 0, 0, h, out, reduce="sum")
    with pytest.raises(ValueError, match="int64 indptr"):
        sage_infer_spmm(ip.int(), ix, 2, 0, 4, 0, 0, h, out)
    with pytest.raises(NotImplementedError, match="GPU"):
        sage_infer_spmm(ip, ix, 2, 0, 4, 0, 0, h, out)
