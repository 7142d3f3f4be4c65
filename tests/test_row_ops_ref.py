"""CPU suite: tests/row_ops_ref.py against itself and against fp64 -- the restated row norm lies inside its
derived interval, the designed rows catch the planted faults through the very assertion the GPU suite makes (row_ops_ref.assert_norms),
the order-sensitive search delivers, random rows do not (which is why the designed rows exist), and the dropout hash is a fair coin."""
import numpy as np
import pytest
import torch

import row_ops_ref as R

DIMS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 602, 1433, 4100]


def _paths(dim):
    return ("vec4", "scalar") if dim % 4 == 0 else ("scalar",)


@pytest.mark.parametrize("dim", DIMS)
def test_the_restatement_lies_inside_the_interval(dim):
    """Both orders, on randn rows and on rows scaled by 2^-30 .. 2^30 (products down to 2^-60 * randn^2: inside the domain)."""
    gen = torch.Generator().manual_seed(dim)
    x = torch.randn(2000, dim, generator=gen)
    k = torch.randint(-30, 31, (2000, 1), generator=gen)
    for rows in (x, x * (2.0 ** k.double()).float()):
        bits = R.bits_of(rows.bfloat16())
        lo, hi = R.embed_norm_interval(bits)
        assert (lo <= hi).all() and float((lo == hi).mean()) > 0.99          # the interval is one bf16 value almost everywhere
        for path in _paths(dim):
            R.assert_norms(R.embed_norm_bits(bits, path), bits, path, ("restatement", dim))


def _storage(rows, stride):
    """rows [n, dim] laid out with ``stride``: the padding columns hold row_ops_ref.PAD, as on the GPU."""
    full = np.full((rows.shape[0], stride), R.bf_bits(R.PAD), dtype=np.uint16)
    full[:, : rows.shape[1]] = rows
    return full


def _faulty(rows, path, fault, stride):
    dim = rows.shape[1]
    if fault == "tail":                                                       # the loop stops at the last FULL group of columns
        group = 256 if path == "vec4" else 64
        return R.embed_norm_bits(rows[:, : dim // group * group], path)
    if fault == "stride":                                                     # `stride` where `dim` belongs: the padding is summed
        return R.embed_norm_bits(_storage(rows, stride), path)
    assert fault == "butterfly"                                               # s += s[lane ^ 1] is skipped
    return R.embed_norm_bits(rows, path, butterfly=R.BUTTERFLY[:-1])


@pytest.mark.parametrize("fault", ["tail", "stride", "butterfly"])
@pytest.mark.parametrize("dim", [2, 3, 5, 7, 8, 63, 65, 252, 255, 257, 260, 516, 602, 1433, 4100])
def test_planted_faults_fail_the_gpu_suites_assertion(dim, fault):
    """assert_norms on the designed rows -- what test_gpu_row_ops.py runs on the device's answer -- refuses each fault, at every
    dim where the fault changes what is read, in launches of 777 rows and (the planted last-column rows alone) of 5 and of 1; the
    skipped butterfly step drops the odd lanes, which takes the random rows of the large launch to see at every dim."""
    bits, dom = R.designed_rows(dim)
    for n in (777,) if fault == "butterfly" else (1, 5, 777):
        rows, d = R.rows_for(n, bits, dom)
        for path in _paths(dim):
            stride = dim + 4 if path == "vec4" else dim + 1
            got = _faulty(rows, path, fault, stride)
            with pytest.raises(AssertionError):
                R.assert_norms(got, rows, path, (dim, fault), d)
            R.assert_norms(R.embed_norm_bits(rows, path), rows, path, (dim, "sound"), d)      # and passes the sound restatement


def test_a_wrong_order_fails_on_the_order_sensitive_rows_only():
    rows = R.order_sensitive_rows(256, 8, 0)
    with pytest.raises(AssertionError):
        R.assert_norms(R.embed_norm_bits(rows, "scalar"), rows, "vec4", "order")
    bits, dom = R.designed_rows(256)
    R.assert_norms(R.embed_norm_bits(bits, "scalar"), bits, "vec4", "order", dom)             # the other 777 rows cannot tell


@pytest.mark.parametrize("dim", [64, 256, 600, 1432, 2048, 4100])
def test_order_sensitive_rows_are_found(dim):
    rows = R.order_sensitive_rows(dim, 8, 0)
    assert rows.shape == (8, dim) and rows.dtype == np.uint16 and (rows < 0x7F80).all()       # non-negative, finite
    v, s = R.embed_norm_bits(rows, "vec4"), R.embed_norm_bits(rows, "scalar")
    assert (v != s).all()
    lo, hi = R.embed_norm_interval(rows)
    assert (lo < hi).all()                                                    # they sit on a rounding midpoint: both answers are in
    for got, path in ((v, "vec4"), (s, "scalar")):
        R.assert_norms(got, rows, path, dim)
    assert R.order_sensitive_rows(dim, 8, 0) is rows                          # cached


def test_random_rows_cannot_tell_the_orders_apart():
    """200 000 randn bf16 rows at dim 256 (numpy's default_rng(0)): the two orders disagree on 0 rows (measured: 0), and the vec4
    order differs from the once-rounded fp64 norm on at most 2.  Other streams measured: default_rng(1 .. 5) gave 2, 1, 1, 1, 0
    disagreeing rows and torch's manual_seed(256) gave 1 -- about 4 per million, so the 777 randn rows of the older 'same bits as
    embed_norm' assertions meet one with probability 0.3 %: they pass for either order."""
    rng = np.random.default_rng(0)
    differ = off = 0
    for _ in range(4):
        bits = R.f2bf(rng.standard_normal((50_000, 256)).astype(np.float32))
        v, s = R.embed_norm_bits(bits, "vec4"), R.embed_norm_bits(bits, "scalar")
        differ += int((v != s).sum())
        x = R.f32_of(bits).astype(np.float64)
        exact = R.rbf64(np.sqrt((x * x).sum(axis=1)))
        off += int((R.f32_of(v) != exact).sum())
    print("orders differ on", differ, "rows; vec4 differs from rbf(fp64) on", off)
    assert differ == 0 and off <= 2


# ---------------------------------------------------------------------------------------------------------------- the dropout hash
N_IDX = 1 << 20
HASH_KEYS = [(0, 0), (0xFFFFFFFF, 7), (123, 1), (5, 0xFFFFFFFE), (0x9E3779B1, 1000)]


@pytest.mark.parametrize("seed,ctr", HASH_KEYS)
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5, 0.9])
def test_drop_hash_is_a_bernoulli_source(p, seed, ctr):
    """keep = drop_hash >= uint32(p 2^32) over 2^20 indices: the keep count, the joint keeps with the next launch counter, the
    joint keeps of adjacent indices (a 1-dependent sequence: Var = (N-1) q^2 (1-q^2) + 2 (N-2) (q^3 - q^4)) each within 5 sigma of
    an ideal coin with q = 1 - thresh / 2^32; the per-column keep counts of a 256-column matrix within 6 sigma, all 256 of them.
    Worst measured over these 20 cases: 2.14 sigma for a single statistic, 4.25 for the maximum over the columns."""
    thr = np.uint32(R.drop_threshold(p))
    q = 1.0 - float(thr) / 2.0 ** 32
    idx = np.arange(N_IDX)
    k0 = R.drop_hash(seed, ctr, idx) >= thr
    k1 = R.drop_hash(seed, (ctr + 1) & 0xFFFFFFFF, idx) >= thr
    N = N_IDX
    z = {
        "keep": (k0.sum() - N * q) / np.sqrt(N * q * (1 - q)),
        "ctr, ctr + 1": ((k0 & k1).sum() - N * q * q) / np.sqrt(N * q * q * (1 - q * q)),
        "adjacent": ((k0[1:] & k0[:-1]).sum() - (N - 1) * q * q) / np.sqrt((N - 1) * q * q * (1 - q * q) + 2 * (N - 2) * (q ** 3 - q ** 4)),
    }
    rows = N // 256
    zc = (k0.reshape(rows, 256).sum(axis=0) - rows * q) / np.sqrt(rows * q * (1 - q))
    print(p, seed, ctr, {k: round(float(v), 2) for k, v in z.items()}, "columns", round(float(np.abs(zc).max()), 2))
    for what, v in z.items():
        assert abs(v) <= 5.0, (what, v)
    assert np.abs(zc).max() <= 6.0


def test_drop_hash_wraps_like_uint32():
    """Index 2^32 + i is index i, and a scalar gives what the array gives."""
    i = np.array([0, 1, 255, 0xFFFFFFFF], dtype=np.int64)
    assert np.array_equal(R.drop_hash(9, 3, i + (1 << 32)), R.drop_hash(9, 3, i))
    assert R.drop_hash(9, 3, np.array([255]))[0] == R.drop_hash(9, 3, i)[2]
    assert R.drop_hash(9, 3, i).dtype == np.uint32 and len(set(R.drop_hash(9, 3, np.arange(1000)).tolist())) == 1000


# ---------------------------------------------------------------------------------------------------------------- the epilogue
def test_sage_epilogue_ref_at_p0_is_torchs_relu_of_the_sum():
    gen = torch.Generator().manual_seed(3)
    for dim in (1, 41, 256):
        a, b = torch.randn(300, dim, generator=gen).bfloat16(), torch.randn(300, dim, generator=gen).bfloat16()
        a[0], b[0] = 3.0e38, 3.0e38                                           # overflows to inf
        out, keep, norm = R.sage_epilogue_ref(a, b, 0.0, 0, 0)
        want = torch.relu(a + b)
        assert np.array_equal(out, R.bits_of(want)) and keep.all()
        assert np.array_equal(norm, R.embed_norm_bits(want, R.norm_path(dim, dim, 0)))
        assert norm[0] == 0x7F80


def test_sage_epilogue_ref_dropout_and_backward():
    gen = torch.Generator().manual_seed(4)
    a, b = torch.randn(64, 40, generator=gen).bfloat16(), torch.randn(64, 40, generator=gen).bfloat16()
    out0, _, _ = R.sage_epilogue_ref(a, b, 0.0, 0, 0)
    for p in (0.1, 0.5, 0.9):
        out, keep, _ = R.sage_epilogue_ref(a, b, p, 11, 5)
        want = (R.f32_of(out0) * (np.float32(1) / (np.float32(1) - np.float32(p)))).astype(np.float32)
        assert np.array_equal(out[keep], R.f2bf(want)[keep]) and (out[~keep] == 0).all()
        assert abs(keep.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / keep.size)
        assert np.array_equal(keep, R.drop_hash(11, 5, np.arange(64 * 40)).reshape(64, 40) >= np.uint32(R.drop_threshold(p)))
        g = torch.randn(64, 40, generator=gen).bfloat16()
        din = R.sage_epilogue_bwd_ref(g, out, p)
        pos = R.f32_of(out) > 0
        assert (din[~pos] == 0).all() and np.array_equal(din[pos], R.bits_of((g.float() * float(R.drop_scale(p))).bfloat16())[pos])
    nan_out = np.array([[0x7FC0, 0x8000, 0x0000, 0x3F80]], dtype=np.uint16)   # NaN, -0, +0, 1
    assert R.sage_epilogue_bwd_ref(torch.full((1, 4), 2.0).bfloat16(), nan_out, 0.0).tolist() == [[0, 0, 0, 0x4000]]


def test_norm_path_is_the_launchers_rule():
    assert R.norm_path(256, 256, 0) == "vec4" and R.norm_path(256, 260, 8) == "vec4"
    assert R.norm_path(256, 257, 0) == "scalar" and R.norm_path(256, 256, 2) == "scalar" and R.norm_path(256, 256, 4) == "scalar"
    assert R.norm_path(255, 256, 0) == "scalar"
