"""CPU suite: tests/gcn_ref.py (the restatement of csrc/gcn.hip) against itself -- the rounded
restatement (``sim=True``: fp32 norms and coefficients, one bf16 rounding) passes the constants the GPU suite holds the kernels
to, and every planted fault fails them:

    one edge missing from a destination row;  one edge missing from a source row;  ns of the hub source taken as 1;
    nd of a degree-0 row not clamped;  a 16-edge chunk of the 1500-edge row dropped;  the dropout scale missing in the backward;
    db including the first row past the count.

Constants: GCN_SPMM_K = (1, 0.25) for the SpMM (one rounding; the fp32 sum of at most 16 384 terms), dense_k(rows + chunks) for
db.  The data are positive where a fault has to be seen (no cancellation hides a lost term).  The keyed mask of a row does not
change when the row count does."""
import numpy as np
import pytest
import torch

import gcn_ref as ref
from bounds import EDGE_DEGREES, HUB_DEGREE, assert_within, dense_k, edge_shape_spec
from gat_glue_ref import keep_mask
from gat_glue_ref import rbf as rbf_np

DIM = 16


@pytest.fixture(scope="module")
def case():
    spec = edge_shape_spec()
    gen = torch.Generator().manual_seed(4)
    h = (torch.rand(spec.K, DIM, generator=gen) + 0.25).bfloat16()
    g = (torch.rand(spec.S, DIM, generator=gen) + 0.25).bfloat16()
    w = (torch.rand(spec.B, generator=gen) + 0.5).bfloat16()
    return spec, h, g, w


def _check(spec, h, w, by_src, fault=None):
    got, _ = ref.spmm_terms(spec.src, spec.dst, spec.S, spec.K, h, w, by_src=by_src, sim=True, fault=fault)
    want, mag = ref.spmm_terms(spec.src, spec.dst, spec.S, spec.K, h, w, by_src=by_src)
    return assert_within(got, want, mag, *ref.GCN_SPMM_K, "gcn spmm")


@pytest.mark.parametrize("weights", [True, False])
def test_rounded_restatement_passes(case, weights):
    spec, h, g, w = case
    assert _check(spec, h, w if weights else None, False) <= 1.0
    assert _check(spec, g, w if weights else None, True) <= 1.0


def test_norms_are_fp32_sqrt_and_one_division(case):
    spec = case[0]
    ns, nd = ref.norms(spec.src, spec.dst, spec.K, spec.S, sim=True)
    ns64, nd64 = ref.norms(spec.src, spec.dst, spec.K, spec.S)
    assert float(nd[0]) == 1.0 and float(ns[-1]) == 1.0                       # a row without in-edges, a source that never sends
    assert float((ns / ns64 - 1).abs().max()) <= 2.0 ** -23 and float((nd / nd64 - 1).abs().max()) <= 2.0 ** -23
    assert float(nd[EDGE_DEGREES.index(16)]) == 0.25 and float(nd[EDGE_DEGREES.index(256)]) == 0.0625


def _row_of_degree(spec, d):
    return int((spec.in_degrees() == d).nonzero()[0])


def test_fault_one_edge_missing_from_a_destination_row(case):
    spec, h, g, w = case
    e = int(spec.indptr[_row_of_degree(spec, 17)]) + 5
    with pytest.raises(AssertionError, match="over the bound"):
        _check(spec, h, w, False, fault={"drop_edges": [e]})


def test_fault_one_edge_missing_from_a_source_row(case):
    spec, h, g, w = case
    outdeg = spec.out_degrees()
    j = int(((outdeg >= 10) & (outdeg <= 40)).nonzero()[0])
    e = int((spec.src == j).nonzero()[3])
    with pytest.raises(AssertionError, match="over the bound"):
        _check(spec, g, w, True, fault={"drop_edges": [e]})


def test_fault_ns_of_the_hub_source_taken_as_one(case):
    spec, h, g, w = case
    hub = int(spec.out_degrees().argmax())
    assert int(spec.out_degrees()[hub]) > 3000
    for by_src, t in ((False, h), (True, g)):
        with pytest.raises(AssertionError, match="over the bound"):
            _check(spec, t, w, by_src, fault={"ns_one": hub})


def test_fault_nd_of_a_degree_0_row_not_clamped(case):
    spec, h, g, w = case
    assert int(spec.in_degrees()[0]) == 0
    with pytest.raises(AssertionError, match="over the bound"):
        _check(spec, h, w, False, fault={"nd_unclamped": True})                 # inf * 0: a NaN row


def test_fault_16_edge_chunk_of_the_1500_edge_row_dropped(case):
    spec, h, g, w = case
    r = _row_of_degree(spec, 1500)
    e0 = (int(spec.indptr[r]) + 700) // 16 * 16
    with pytest.raises(AssertionError, match="over the bound"):
        _check(spec, h, w, False, fault={"drop_edges": list(range(e0, e0 + 16))})


def test_hub_row_holds_the_constant(case):
    spec, h, g, w = case
    r = _row_of_degree(spec, HUB_DEGREE)
    got, _ = ref.spmm_terms(spec.src, spec.dst, spec.S, spec.K, h, w, sim=True)
    want, mag = ref.spmm_terms(spec.src, spec.dst, spec.S, spec.K, h, w)
    assert assert_within(got[r], want[r], mag[r], *ref.GCN_SPMM_K, "hub row") <= 1.0


# ------------------------------------------------------------------------------------------------ epilogue
ROWS, LIVE, WIDTH, P, SEED = 65, 64, 16, 0.5, 1234


def _epi_case():
    rng = np.random.default_rng(7)
    a = rbf_np(rng.standard_normal((ROWS, WIDTH)).astype(np.float32))
    bias = rbf_np(rng.standard_normal(WIDTH).astype(np.float32) * 0.1)
    dout = rbf_np((rng.random((ROWS, WIDTH)) + 0.25).astype(np.float32))
    return a, bias, dout


def _db_check(fault, relu=True):
    a, bias, dout = _epi_case()
    out = ref.epilogue_fwd(a, bias, relu, P, SEED, 3, LIVE)
    _, want, mag = ref.epilogue_bwd(dout, out, relu, P, SEED, 3, LIVE)
    _, got, _ = ref.epilogue_bwd(dout, out, relu, P, SEED, 3, LIVE, fault=fault)
    got = rbf_np(got.astype(np.float32))
    return assert_within(torch.from_numpy(got), torch.from_numpy(want), torch.from_numpy(mag), *dense_k(LIVE + LIVE // 32 + 1), "db")


def test_epilogue_restatement_passes_and_rows_past_the_count_are_zero():
    a, bias, dout = _epi_case()
    out = ref.epilogue_fwd(a, bias, True, P, SEED, 3, LIVE)
    din, _, _ = ref.epilogue_bwd(dout, out, True, P, SEED, 3, LIVE)
    assert not out[LIVE:].any() and not din[LIVE:].any()
    assert np.array_equal(din[:LIVE] != 0, out[:LIVE] > 0)                      # (dout > 0 everywhere)
    kept = out[:LIVE] > 0
    assert np.array_equal(din[:LIVE][kept], rbf_np(dout[:LIVE] * np.float32(2.0))[kept])
    assert _db_check(None) <= 1.0


def test_fault_dropout_scale_missing_in_the_backward():
    with pytest.raises(AssertionError, match="over the bound"):
        _db_check({"no_drop_scale": True})
    a, bias, dout = _epi_case()
    out = ref.epilogue_fwd(a, bias, True, P, SEED, 3, LIVE)
    good, _, _ = ref.epilogue_bwd(dout, out, True, P, SEED, 3, LIVE)
    bad, _, _ = ref.epilogue_bwd(dout, out, True, P, SEED, 3, LIVE, fault={"no_drop_scale": True})
    with pytest.raises(AssertionError, match="over the bound"):                # per element: 1 ulp against a factor of 2
        assert_within(torch.from_numpy(bad), torch.from_numpy(good), torch.from_numpy(np.abs(good)), 1, 0.0, "din")


def test_fault_db_including_the_first_row_past_the_count():
    """(Without the ReLU: with it the row's stored output is zero and masks the row's gradient.)"""
    assert _db_check(None, relu=False) <= 1.0
    with pytest.raises(AssertionError, match="over the bound"):
        _db_check({"db_extra_rows": 1}, relu=False)


def test_a_rows_mask_does_not_depend_on_the_row_count():
    for width in (7, 16, 256):
        small = keep_mask(33, width, 0.1, SEED, 5)
        assert np.array_equal(small, keep_mask(65, width, 0.1, SEED, 5)[:33])
        assert np.array_equal(small, keep_mask(4096, width, 0.1, SEED, 5)[:33])
        assert not np.array_equal(small, keep_mask(33, width, 0.1, SEED, 6))    # another launch, another mask
        assert 0.8 < small.mean() < 0.97
    a, bias, _ = _epi_case()
    for live in (1, 33, 64):
        assert np.array_equal(ref.epilogue_fwd(a, bias, True, 0.1, SEED, 2, live)[:live], ref.epilogue_fwd(a, bias, True, 0.1, SEED, 2, ROWS)[:live])


# ------------------------------------------------------------------------------------------------ the layer formula
def test_layer_terms_are_the_two_product_orders():
    """rst of layer_terms == the SpMM restatement around the product in either order (fp64), and its gradients are the mirrored
    formulas: d x = spmm_bwd(g) W^T = spmm_bwd(g W^T), d W = x^T spmm_bwd(g) = spmm_fwd(x)^T g, d b = sum g."""
    spec = edge_shape_spec()
    gen = torch.Generator().manual_seed(8)
    fin, fout = 12, 5
    x = torch.randn(spec.K, fin, generator=gen).bfloat16()
    W = (torch.randn(fin, fout, generator=gen) * 0.3).bfloat16()
    b = torch.randn(fout, generator=gen).bfloat16()
    w = (torch.rand(spec.B, generator=gen) + 0.5).bfloat16()
    g = torch.randn(spec.S, fout, generator=gen).bfloat16()
    T = ref.layer_terms(spec.src, spec.dst, spec.S, spec.K, x, W, b, w, g)
    sp = lambda t, by_src: ref.spmm_terms(spec.src, spec.dst, spec.S, spec.K, t, w, by_src=by_src)[0]
    Wd, xd, gd = W.double(), x.double(), g.double()
    close = lambda u, v: float((u - v).abs().max()) <= 1e-9 * (1 + float(v.abs().max()))
    assert close(sp(xd @ Wd, False) + b.double(), T["rst"]) and close(sp(xd, False) @ Wd + b.double(), T["rst"])
    assert close(sp(gd, True) @ Wd.t(), T["d_x"]) and close(sp(gd @ Wd.t(), True), T["d_x"])
    assert close(xd.t() @ sp(gd, True), T["d_W"]) and close(sp(xd, False).t() @ gd, T["d_W"])
    assert close(gd.sum(0), T["d_b"])
    assert bool((T["mag_rst"] >= T["rst"].abs() - 1e-9).all()) and bool((T["mag_d_x"] >= T["d_x"].abs() - 1e-9).all())
    assert bool((T["mag_d_W"] >= T["d_W"].abs() - 1e-9).all())
