"""CPU suite: what the GPU checks of tests/test_gpu_wide_gemm.py catch (as tests/test_bounds.py shows for the narrow kernels), on
the same operands (tests/wide_cases.py).  A panel walk can go wrong at a seam: the 16-step that ends panel 0 (k 1008 .. 1023) or
the one that opens panel 1 (k 1024 .. 1039) never multiplied, a seam column dropped, staged by both panels, or the second panel
staged from panel 0's columns again.  The fp64 bound fails on the first two at K = 1433; the exact one-hot probe fails on each of
the last three -- and both hold on the kernel's own restatement (fp32 accumulation, one rounding)."""
import pytest
import torch

from bounds import assert_within, dense_k, gemm_terms, rbf
from wide_cases import PANEL, fwd_inputs, one_hot_rows, rand, seam_cols, seam_fault

F32 = torch.float32
K, N, M = 1433, 256, 33                                   # a dense case of test_wide_single_product_against_fp64


def _ops():
    c = fwd_inputs(K, N, M)
    return dict(a1=c["a1"][:M], w1=c["w1"], bias=c["b"]), c["n_terms"]


def test_the_restatement_of_the_dense_case_is_within_its_bound():
    o, n_terms = _ops()
    ref, mag = gemm_terms(**o)
    got = rbf(gemm_terms(**o, acc=F32)[0])
    assert n_terms == K + 1 and assert_within(got, ref, mag, *dense_k(n_terms), "wide gemm restated") <= 1


@pytest.mark.parametrize("k0", [PANEL - 16, PANEL])
def test_a_dropped_seam_kstep_fails_the_dense_bound(k0):
    """One MFMA k-step of one 32 x 32 tile skipped on either side of the first seam: elements of that tile leave the bound (and
    only that tile's)."""
    o, n_terms = _ops()
    ref, mag = gemm_terms(**o)
    got = rbf(gemm_terms(**o, acc=F32, fault={"drop_kstep": (0, 0, k0)})[0])
    with pytest.raises(AssertionError, match="over the bound"):
        assert_within(got, ref, mag, *dense_k(n_terms), "wide gemm, k-step %d dropped" % k0)
    assert assert_within(got[:, 32:], ref[:, 32:], mag[:, 32:], *dense_k(n_terms), "the other tiles") <= 1
    assert assert_within(got[32:], ref[32:], mag[32:], *dense_k(n_terms), "the other row tile") <= 1


def _probe(K_, fault):
    """The seam probe's own assertion on the CPU: the rows whose output bits differ from W[:, c]^T."""
    a, col = one_hot_rows(K_, 70)
    w = rand(torch.Generator().manual_seed(K_), 41, K_)
    out = seam_fault(a, w, fault)
    want = w[:, col].t().contiguous()
    bad = (out.view(torch.int16) != want.view(torch.int16)).any(1).nonzero().reshape(-1).tolist()
    return bad, col


@pytest.mark.parametrize("K_", [1025, 1433, 2049])
def test_the_seam_probe_holds_on_a_sound_walk_and_fails_on_each_seam_fault(K_):
    assert PANEL - 1 in seam_cols(K_) and PANEL in seam_cols(K_) and K_ - 1 in seam_cols(K_) and 0 in seam_cols(K_)
    assert (2 * PANEL in seam_cols(K_)) == (K_ > 2 * PANEL)
    bad, _ = _probe(K_, None)
    assert bad == []
    for fault in ("drop", "dup", "panel0"):
        bad, col = _probe(K_, fault)
        assert bad, fault
        hit = sorted(set(int(col[r]) for r in bad))
        if fault == "panel0":
            # rows probing a column of panel 1 read nothing (their one sits in columns panel 0 does not have); rows probing
            # column j of panel 0 also see W[:, PANEL + j] where panel 1 has that column
            assert PANEL in hit and all(c >= PANEL or c + PANEL < K_ for c in hit), hit
        else:
            assert hit == [PANEL], (fault, hit)             # exactly the rows that probe the seam column


def test_the_probe_with_a_bias_is_exact_in_the_kernels_arithmetic():
    """bf16(float(W[n, c]) + float(b[n])): the fp32 accumulator holds W[n, c] exactly (one non-zero term), the bias is added in
    fp32 and the sum rounded once -- the restatement gives those bits."""
    a, col = one_hot_rows(1433, 70)
    gen = torch.Generator().manual_seed(5)
    w, b = rand(gen, 41, 1433), rand(gen, 41)
    got = rbf(gemm_terms(a, w, bias=b, acc=F32)[0]).to(torch.bfloat16)
    want = (w[:, col].t().float() + b.float()[None, :]).to(torch.bfloat16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
