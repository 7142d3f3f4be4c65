"""CPU suite: the NumPy restatement of the GATv2 glue kernels (tests/gat_glue_ref.py) -- the keyed mask's
law, its independence of the row count, and the rounding points against torch's bf16 tensor ops."""
import numpy as np
import pytest
import torch

import gat_glue_ref as ref


def _bf(t):
    return torch.from_numpy(np.ascontiguousarray(t)).bfloat16()


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_rate_and_scale(p):
    rows, width = 256, 256                                                       # 2^16 elements
    keep = ref.keep_mask(rows, width, p, seed=1234, ctr=3)
    n = keep.size
    rate = keep.mean()
    assert n == 2 ** 16 and abs(rate - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5, (p, rate)
    x = np.ones((rows, width), np.float32)
    out, pre = ref.glue_fwd(x, None, 1, width, 0, False, p=p, seed=1234, ctr=3)
    assert np.array_equal(pre, x) and np.array_equal(out != 0, keep)
    want = float(_bf(np.float32([1.0 / (1.0 - np.float32(p))]))[0])               # 1 / (1 - p), rounded as the product is
    assert np.all(out[keep] == np.float32(want))
    assert not np.array_equal(keep, ref.keep_mask(rows, width, p, seed=1234, ctr=4))     # the next launch draws another mask


def test_a_rows_mask_does_not_depend_on_the_row_count():
    small = ref.keep_mask(37, 24, 0.3, seed=9, ctr=5)
    for rows in (38, 64, 512):
        assert np.array_equal(ref.keep_mask(rows, 24, 0.3, seed=9, ctr=5)[:37], small)
    x = np.random.default_rng(0).standard_normal((64, 24)).astype(np.float32)
    x = ref.rbf(x)
    a, _ = ref.glue_fwd(x[:37], None, 1, 24, 0, False, p=0.3, seed=9, ctr=5)
    b, _ = ref.glue_fwd(x, None, 1, 24, 0, False, p=0.3, seed=9, ctr=5, n_live=37)   # a capacity of 64 rows, 37 live
    assert np.array_equal(a, b[:37]) and not b[37:].any()


@pytest.mark.parametrize("H,D,mean", [(1, 7, True), (2, 8, False), (2, 8, True), (4, 16, False), (4, 16, True), (3, 5, False)])
def test_rounding_points_are_those_of_the_bf16_tensor_ops(H, D, mean):
    """p = 0: add, ELU, flatten / mean(1) and their autograd on torch's CPU bf16 kernels, bit for bit (up to four heads the fp32
    sum is sequential either way; the derivative of ELU is taken from its input, as torch's out-of-place elu takes it)."""
    rng = np.random.default_rng(H * 100 + D)
    n = 19
    rst, res = ref.rbf(rng.standard_normal((n, H * D)).astype(np.float32) * 2), ref.rbf(rng.standard_normal((n, H * D)).astype(np.float32))
    width = D if mean else H * D
    dout = ref.rbf(rng.standard_normal((n, width)).astype(np.float32))
    out, pre = ref.glue_fwd(rst, res, H, D, 1, mean)
    din = ref.glue_bwd(dout, rst, res, H, D, 1, mean)
    a, b = _bf(rst).requires_grad_(True), _bf(res).requires_grad_(True)
    y = torch.nn.functional.elu(a + b).view(n, H, D)
    z = y.mean(1) if mean else y.flatten(1)
    z.backward(_bf(dout))
    assert np.array_equal(out, pre) and torch.equal(_bf(out), z.detach())
    assert torch.equal(_bf(din), a.grad) and torch.equal(a.grad, b.grad)
    e = ref.rbf(rng.standard_normal((50, H)).astype(np.float32))
    assert torch.equal(_bf(ref.head_mean(e)), _bf(e).mean(1))


def test_rows_past_the_count_are_zero_and_unread():
    rng = np.random.default_rng(1)
    rst = ref.rbf(rng.standard_normal((9, 16)).astype(np.float32))
    bad = rst.copy()
    bad[5:] = np.nan
    for mean in (False, True):
        a, _ = ref.glue_fwd(rst, rst, 2, 8, 1, mean, p=0.2, seed=3, ctr=1, n_live=5)
        b, _ = ref.glue_fwd(bad, bad, 2, 8, 1, mean, p=0.2, seed=3, ctr=1, n_live=5)
        assert np.array_equal(a, b) and not a[5:].any() and a[:5].any()
        d = ref.glue_bwd(a, bad, bad, 2, 8, 1, mean, p=0.2, seed=3, ctr=1, n_live=5)
        assert np.isfinite(d).all() and not d[5:].any()
