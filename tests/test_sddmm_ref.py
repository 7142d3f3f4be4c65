"""CPU checks around the per-edge dot product (csrc/sddmm.hip): the torch restatement of tests/sddmm_ref.py
against a plain Python loop, the bound against planted faults, the C entry point's refusals, the profiler's name table, the
``fn.u_dot_v`` descriptor and the refusal list of ``explain.edge_gradients``.

The bound: |got - ref| <= 1 ulp_bf16(ref) + (dim + 2) * 2^-16 * 2^-8 * mag (sddmm_ref.k = bounds.dense_k(dim + 2)): ``dim`` fp32
products and sums each within 2^-24 relative of the running magnitude, the coefficient product and the reciprocal one more each
(counted at 2^-16 of a 2^-8 unit like every fp32 term of bounds.dense_k, a generous over-count), and the one rounding to bf16.
The planted faults are far outside it on positive operands: a dropped column moves a sum of ``dim`` terms of similar size by
about 1 / dim of its magnitude (>= 2^-6 at dim 41, against a bound of about 2^-8), the neighbour's degree changes the
coefficient by a factor of at least 3 / 2 on the hand block."""
import ctypes as C

import pytest
import torch

import bounds
import sddmm_ref as ref

MODES = (ref.SUM, ref.MEAN, ref.SELF, ref.MAX)


def hand_block():
    """3 destinations of in-degree 0, 3 and 2; destination 1 has the parallel edges 3 -> 1 twice; source 2 sends nothing."""
    indptr = torch.tensor([0, 0, 3, 5])
    src = torch.tensor([3, 3, 4, 0, 1])
    dst = torch.tensor([1, 1, 1, 2, 2])
    return bounds.Spec(5, 3, indptr, src, dst)


def hand_arg(spec, dim, seed):
    """A winner table as bliss_spmm_max_fwd leaves it: per (row, column) one of the row's edges, -1 for the row without edges."""
    gen = torch.Generator().manual_seed(seed)
    arg = torch.full((spec.S, dim), -1, dtype=torch.int32)
    for r in range(spec.S):
        lo, hi = int(spec.indptr[r]), int(spec.indptr[r + 1])
        if hi > lo:
            arg[r] = torch.randint(lo, hi, (dim,), generator=gen).to(torch.int32)
    return arg


@pytest.mark.parametrize("dim", [1, 11, 128, 140])
@pytest.mark.parametrize("mode", MODES)
def test_restatement_equals_the_loop_on_the_hand_block(mode, dim):
    spec = hand_block()
    a, b = ref.operands(spec, dim, 3 + dim, "cpu")
    arg = hand_arg(spec, dim, 5) if mode == ref.MAX else None
    want = ref.loop_ref(spec, a, b, mode, arg)
    val, mag = ref.terms(spec, a, b, mode, arg)
    assert torch.allclose(val, want, rtol=0, atol=1e-12)
    assert bool((mag >= val.abs() - 1e-12).all())
    got32 = ref.dot_f32(spec, a, b, mode, arg, out_fp32=True)
    assert got32.dtype == torch.float32 and got32.shape == (spec.B,)
    assert bool(((got32.double() - want).abs() <= (dim + 2) * 2.0 ** -24 * mag + 1e-30).all())
    got = ref.dot_f32(spec, a, b, mode, arg)
    assert got.dtype == torch.bfloat16
    bounds.assert_within(got, val, mag, *ref.k(dim), "restatement")


def test_restatement_is_the_documented_order():
    """One edge, dim 136 (two steps: lanes 0 and 1 own a second group... lane 0 only): the lane sums and the tree by hand."""
    spec = bounds.Spec(1, 1, torch.tensor([0, 1]), torch.tensor([0]), torch.tensor([0]))
    a, b = ref.operands(spec, 136, 9, "cpu")
    prod = (a.float() * b.float())[0]
    lanes = []
    for lane in range(16):
        acc = torch.zeros((), dtype=torch.float32)
        for g in range(lane, 17, 16):
            for c in range(8 * g, 8 * g + 8):
                acc = acc + prod[c]
        lanes.append(acc)
    p = lanes
    tree = ((((p[15] + p[14]) + (p[13] + p[12])) + ((p[11] + p[10]) + (p[9] + p[8])))
            + (((p[7] + p[6]) + (p[5] + p[4])) + ((p[3] + p[2]) + (p[1] + p[0]))))
    assert torch.equal(ref.dot_f32(spec, a, b, ref.SUM, out_fp32=True), tree.reshape(1))


@pytest.mark.parametrize("fault,mode", [("drop_col", ref.SUM), ("drop_col", ref.MAX), ("wrong_deg", ref.MEAN), ("wrong_deg", ref.SELF)])
def test_planted_fault_is_outside_the_bound(fault, mode):
    spec, dim = hand_block(), 41
    a, b = ref.operands(spec, dim, 17, "cpu")
    a, b = a.abs() + 0.5, b.abs() + 0.5                        # no cancellation: the fault cannot hide
    arg = None
    if mode == ref.MAX:
        arg = torch.full((spec.S, dim), -1, dtype=torch.int32)
        arg[1], arg[2] = 0, 3                                   # edges 0 and 3 win every column of their rows
    val, mag = ref.terms(spec, a, b, mode, arg)
    bounds.assert_within(ref.dot_f32(spec, a, b, mode, arg), val, mag, *ref.k(dim), "sound")
    bad, _ = ref.terms(spec, a, b, mode, arg, fault=fault)
    with pytest.raises(AssertionError):
        bounds.assert_within(bad, val, mag, *ref.k(dim), fault)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from bliss_gnn_amd import _lib
    lib, E = _lib.lib, _lib.EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def call(src=p, dst=p, indptr=p, nnz=4, a=p, a_stride=8, b=p, b_stride=8, arg=p, arg_stride=8, dim=8, mode=_lib.SDDMM_SUM, out=p):
        return lib.bliss_sddmm_dot(src, dst, indptr, 0, nnz, a, a_stride, b, b_stride, arg, arg_stride, dim, mode, out, 0, 0)

    for name in ("src", "dst", "a", "b", "out"):
        assert call(**{name: 0}) == E, name
    assert call(indptr=0, mode=_lib.SDDMM_MEAN) == E and call(indptr=0, mode=_lib.SDDMM_SELF) == E
    assert call(arg=0, mode=_lib.SDDMM_MAX) == E
    assert call(nnz=-1) == E and call(dim=0) == E and call(dim=-3) == E
    assert call(a_stride=7) == E and call(b_stride=7) == E and call(arg_stride=7, mode=_lib.SDDMM_MAX) == E
    assert call(mode=4) == E and call(mode=-1) == E
    # nnz == 0: nothing to do, whatever the pointers -- 0 without a launch (this machine may have no GPU)
    assert call(nnz=0) == 0 and call(nnz=0, src=0, dst=0, a=0, b=0, out=0) == 0
    assert (_lib.SDDMM_SUM, _lib.SDDMM_MEAN, _lib.SDDMM_SELF, _lib.SDDMM_MAX) == (ref.SUM, ref.MEAN, ref.SELF, ref.MAX)


def test_profiler_names_the_kernel_and_keeps_the_pinned_positions():
    from bliss_gnn_amd import _lib
    n = _lib.lib.bliss_prof_kernel_count()
    names = [_lib.lib.bliss_prof_kernel_name(i).decode() for i in range(n)]
    assert names.count("k_sddmm_dot") == 1
    assert names[-3:] == ["k_sddmm_dot", "k_spmm_max_bwd_relu", "k_spmm_max_bwd_relu_fixup"]
    assert names.index("k_spmm_max_bwd") == 26


def test_u_dot_v_descriptor():
    from bliss_gnn_amd import function as fn
    m = fn.u_dot_v("h", "g", "score")
    assert (m.kind, m.lhs, m.rhs, m.out) == ("u_dot_v", "h", "g", "score")


def test_apply_edges_names_both_builtins_when_it_refuses():
    from bliss_gnn_amd import function as fn
    blk = bounds.to_block(hand_block(), "cpu")
    with pytest.raises(NotImplementedError, match="u_add_v.*u_dot_v"):
        blk.apply_edges(fn.u_mul_e("h", "w", "m"))


def test_edge_gradients_refuses_what_does_not_differentiate():
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import explain
    from bliss_gnn_amd.model import GATv2, GCN, SAGE
    assert bg.edge_gradients is explain.edge_gradients
    refused = [(SAGE(8, 8, 3, 2, torch.relu, 0.0, transforms="tile", aggregator_type="pool"), "tile"),
               (SAGE(8, 8, 3, 2, torch.relu, 0.0, transforms="tile", aggregator_type="gcn"), "tile"),
               (GCN(8, 8, 3, 2, torch.relu, 0.0, transforms="tile"), "tile"),
               (GCN(8, 8, 3, 2, torch.relu, 0.0, transforms="wide"), "wide"),
               (GATv2(2, 8, 4, 3, [2, 1], torch.relu, 0.0, 0.0, 0.2, False), "identically zero"),
               (torch.nn.Linear(2, 2), "Linear")]
    for model, word in refused:
        assert word in explain.refusal(model)
        with pytest.raises(NotImplementedError, match=word):
            explain.edge_gradients(model, [], None, lambda y: y.sum())       # refused before anything is touched
    for model in (SAGE(8, 8, 3, 2, torch.relu, 0.0), SAGE(8, 8, 3, 2, torch.relu, 0.0, aggregator_type="pool"),
                  SAGE(8, 8, 3, 2, torch.relu, 0.0, aggregator_type="gcn"), SAGE(8, 8, 3, 2, torch.relu, 0.0, transforms="tile"),
                  GCN(8, 8, 3, 2, torch.relu, 0.0)):
        assert explain.refusal(model) is None


def test_sddmm_is_forward_only():
    """The op's registered autograd formula raises, naming the op (no second derivative)."""
    from bliss_gnn_amd import ops
    with pytest.raises(NotImplementedError, match="bliss::sddmm"):
        ops._sddmm_no_grad(None, None)
