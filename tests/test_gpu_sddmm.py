"""GPU suite (-m gpu): the per-edge dot product kernel k_sddmm_dot (csrc/sddmm.hip) against its
restatement tests/sddmm_ref.py.

Every result is held to two checks: BIT-EQUAL to ``sddmm_ref.dot_f32``, which adds the fp32 products in the order the kernel's
header writes down (a lane's 8-column groups in ascending order from +0, the 16 lane sums as a balanced tree of neighbours, then
the coefficient, one rounding), and within ``sddmm_ref.k(dim)`` = bounds.dense_k(dim + 2) of the fp64 value: ``dim`` fp32 products
and sums, the coefficient product and the reciprocal, each counted at 2^-16 of a 2^-8 unit of the magnitude coef * sum |a| |b|,
and 1 ulp for the one rounding to bf16 (an fp32 output is held to the same bound, which it meets with room).

Shapes: bounds.edge_shape_spec() (degrees 0, 1, 2, 15-17, 63-65, 255-257, 512, 513, 1500, a hub of 12 000; ~27 K edges, so
32-edge runs) at dim 1, 3, 4, 8, 41, 64, 128, 136, 256, 260 -- the scalar, 8-byte and 16-byte forms, one, two and three steps per
quad, a last step of 8 and of 4 columns -- contiguous and column-sliced (row stride dim + 3, base 2 bytes off: the scalar form);
blocks of exactly 1 .. 257 edges (a quad's and a 16-edge run's boundaries); a capacity-padded block with NaN rows and garbage
winners past the live counts."""
import pytest
import torch

import bounds
import sddmm_ref as ref

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 8, 41, 64, 128, 136, 256, 260)
SMALL_B = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
MODES = (ref.SUM, ref.MEAN, ref.SELF, ref.MAX)


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _sddmm(blk, a, b, mode, arg=None, out_fp32=False, counts="block"):
    from bliss_gnn_amd import ops
    if counts == "block":
        counts = getattr(blk, "_counts_dev", None) if blk._nnz_ptr else None
    return ops.sddmm(blk.src, blk.dst, blk.indptr, a, b, arg, counts, mode, out_fp32)


def _args(blk, b, seed):
    """The winner tables of the project's own max-reduce on ``b``: unweighted and weighted."""
    from bliss_gnn_amd.nn import max_aggregate
    gen = torch.Generator().manual_seed(seed)
    w = (torch.rand(blk.num_edges(), generator=gen) + 0.25).bfloat16().to(b.device)
    bc = b.contiguous()
    return [max_aggregate(blk, bc, None, return_arg=True)[1], max_aggregate(blk, bc, w, return_arg=True)[1]]


def _check(spec, got, a, b, mode, arg, what, out_fp32=False, live=None):
    B, dim = spec.B if live is None else live, a.shape[1]
    assert got.dtype == (torch.float32 if out_fp32 else torch.bfloat16)
    want = ref.dot_f32(spec, a, b, mode, arg, live=live, out_fp32=out_fp32)
    assert torch.equal(_bits(got[:B]), _bits(want)), (what, int((_bits(got[:B]) != _bits(want)).sum()))
    val, mag = ref.terms(spec, a, b, mode, arg, live=live)
    return bounds.assert_within(got[:B], val, mag, *ref.k(dim), what)


def _all_modes(spec, blk, dim, seed, layouts=(False, True), dtypes=(False, True)):
    worst = 0.0
    for sliced in layouts:
        a, b = ref.operands(spec, dim, seed, blk.device, sliced=sliced)
        assert (a.stride(0) > dim and a.data_ptr() % 4 == 2) == sliced
        for mode in MODES:
            for arg in (_args(blk, b, seed) if mode == ref.MAX else [None]):
                for out_fp32 in dtypes:
                    got = _sddmm(blk, a, b, mode, arg, out_fp32)
                    assert got.shape == (spec.B,)
                    worst = max(worst, _check(spec, got, a, b, mode, arg, (dim, sliced, mode, out_fp32), out_fp32))
    return worst


@pytest.fixture(scope="module")
def edge(cuda):
    spec = bounds.edge_shape_spec()
    return spec, bounds.to_block(spec, cuda)


@pytest.mark.parametrize("dim", DIMS)
def test_edge_shapes_bit_equal_and_within_bound(edge, dim):
    spec, blk = edge
    print(dim, _all_modes(spec, blk, dim, 100 + dim))


@pytest.mark.parametrize("B", SMALL_B)
def test_quad_and_run_boundaries(cuda, B):
    spec = bounds.from_degrees([B // 2, 0, B - B // 2], 40, seed=B, n_unused=3)
    blk = bounds.to_block(spec, cuda)
    assert spec.B == B
    for dim in (64, 41):
        _all_modes(spec, blk, dim, 7 * B + dim, layouts=(False,), dtypes=(False,))


@pytest.mark.parametrize("dim", (64, 41))
def test_padded_block_reads_nothing_past_the_live_counts(edge, dim):
    spec, exact = edge
    dev = exact.device
    pad = bounds.padded_block(spec, dev)
    Sc, Kc, cap = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    a0, b0 = ref.operands(spec, dim, 31 + dim, dev)
    a = torch.full((Sc, dim), float("nan"), dtype=torch.bfloat16, device=dev)
    b = torch.full((Kc, dim), float("nan"), dtype=torch.bfloat16, device=dev)
    a[: spec.S], b[: spec.K] = a0, b0
    arg0 = _args(exact, b0, dim)[1]
    arg = torch.randint(0, cap, (Sc, dim), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    arg[: spec.S] = arg0
    zero_counts = torch.zeros(10, dtype=torch.int32, device=dev)
    for mode in MODES:
        for out_fp32 in (False, True):
            m_arg = (arg0, arg) if mode == ref.MAX else (None, None)
            want = _sddmm(exact, a0, b0, mode, m_arg[0], out_fp32)
            got = _sddmm(pad, a, b, mode, m_arg[1], out_fp32)
            assert got.shape == (cap,)
            assert torch.equal(_bits(got[: spec.B]), _bits(want)), (mode, out_fp32)
            assert not bool(_bits(got[spec.B:]).any()), (mode, out_fp32)                  # +0, bit for bit
            none = _sddmm(pad, a, b, mode, m_arg[1], out_fp32, counts=zero_counts)        # live count 0
            assert none.shape == (cap,) and not bool(_bits(none).any()), (mode, out_fp32)
            _check(spec, got, a, b, mode, m_arg[1], ("padded", mode, out_fp32), out_fp32, live=spec.B)


def test_max_specials(cuda):
    """Destination 0: edge 0 (source 1) wins every column, edge 1 (source 2) none, edge 2 is edge 0's parallel twin -- the lowest
    edge wins the tie, the twin gets exactly +0.  Destination 1 has no edges.  Also: a column-sliced int32 winner table."""
    from bliss_gnn_amd.nn import max_aggregate
    spec = bounds.Spec(3, 2, torch.tensor([0, 3, 3]), torch.tensor([1, 2, 1]), torch.tensor([0, 0, 0]))
    blk = bounds.to_block(spec, cuda)
    dim = 64
    a, b = ref.operands(spec, dim, 5, cuda)
    b[1], b[2] = b[1].abs() + 4, -b[2].abs() - 4
    _, arg = max_aggregate(blk, b, None, return_arg=True)
    assert bool((arg[0] == 0).all()) and bool((arg[1] == -1).all())
    got = _sddmm(blk, a, b, ref.MAX, arg)
    full = _sddmm(blk, a, b, ref.SUM)
    assert torch.equal(_bits(got[:1]), _bits(full[:1])) and not bool(_bits(got[1:]).any())
    _check(spec, got, a, b, ref.MAX, arg, "specials")
    wide = torch.full((2, dim + 3), -7, dtype=torch.int32, device=cuda)
    wide[:, 1:1 + dim] = arg
    assert torch.equal(_bits(_sddmm(blk, a, b, ref.MAX, wide[:, 1:1 + dim])), _bits(got))


def test_two_runs_give_the_same_bits(edge):
    spec, blk = edge
    a, b = ref.operands(spec, 256, 77, blk.device)
    arg = _args(blk, b, 3)[1]
    for mode in MODES:
        m_arg = arg if mode == ref.MAX else None
        assert torch.equal(_bits(_sddmm(blk, a, b, mode, m_arg)), _bits(_sddmm(blk, a, b, mode, m_arg)))


def test_u_dot_v_through_apply_edges(edge):
    from bliss_gnn_amd import function as fn
    spec, blk = edge
    a, b = ref.operands(spec, 41, 13, blk.device)
    with blk.local_scope():
        blk.srcdata["h"], blk.dstdata["g"] = b, a
        blk.apply_edges(fn.u_dot_v("h", "g", "score"))
        got = blk.edata["score"]
    assert got.shape == (spec.B, 1) and got.dtype == torch.bfloat16 and not got.requires_grad
    _check(spec, got.reshape(-1), a, b, ref.SUM, None, "u_dot_v")
