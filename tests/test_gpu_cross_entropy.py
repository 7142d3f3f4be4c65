"""GPU suite: the one-launch single-label loss (csrc/loss.hip: k_cross_entropy; nn.CrossEntropyLoss) per element against fp64 at
the shapes where such kernels break, on every route that reaches it.

The yardstick is bounds.ce_terms in float64 on the same bf16 logits (bf16(a + b) for the two-addend routes):

    gradient   |got - ref| <= 1 ulp_bf16(ref) + k 2^-24 / denom,   k = 17 + 3 ln(n_cls) + ceil(n_cls / 64)     every element
    loss       |got - ref| <= k_loss 2^-24 mag_loss,   k_loss = 3 ln(n_cls) + ceil(n_cls / 64) + 13 + ceil(n_rows / 256) + 12
               mag_loss = (1/denom) sum_r (|m_r| + |log s_r| + |x_{r,y}|);  one bf16 ulp on top where forward() casts to bf16

Gradient.  The kernel computes, all in fp32, t = x - m, e = __expf(t) = v_exp(fl(t log2 e)), s = sum e, inv = 1 / s, p = e inv,
(p - onehot) inv_n, and rounds once to bf16.  The final rounding is half a bf16 spacing of the fp32 value, which may sit one
binade above ref: 1 ulp_bf16(ref).  Before it, in units of 2^-24 / denom (p <= 1 everywhere):
  - the exponential of one class: its argument carries the rounding of x - m, of the product with log2 e and of the constant
    log2 e itself (3 |t| 2^-24 relative to e in all), the instruction one ulp (2): (3 |t| + 2) e^-|t| <= 2.2 at most;
  - the sum: the same errors weighted by p_j, sum_j p_j (3 t_j + 2) = 3 (H(p) - ln s) + 2 <= 3 ln(n_cls) + 2 (the entropy
    bound), plus one rounding per addition along the longest chain, a lane's ceil(n_cls / 64) strided terms and the 6 steps
    of the wave's tree; it reaches p_c as p_c times that, p_c <= 1;
  - the reciprocal (2), the product e inv (1), the subtraction p - 1 (exact for p >= 1/2, half a unit below), the product
    with inv_n (1) and inv_n = fl(1 / denom) itself (2): 6.5.
  2.2 + 3 ln(n_cls) + 2 + ceil(n_cls / 64) + 6 + 6.5 < k.  A p below the smallest normal fp32 number is flushed to 0 by the
exponential instruction: an absolute error below 2^-126 / denom, far inside the absolute term, which is what absorbs it (the
ulp term of such an element is 2^-133).  At |t| > 87 the exponential is 0 outright, the same way.
  The label element of a confident row is where the absolute term matters: p - 1 cancels to -(1 - p_y), whose bf16 spacing
is tiny while the fp32 error of p_y stays at 2^-24 scale.  Orientation: the fp32 restatement on the CPU stays under 0.76 of
1 ulp + 2^-22 / denom (a k of 4) over all cases below; the derived k is the one asserted.

Loss.  A row's m + log s - x_y: the relative error of s above becomes an absolute error of log s (3 ln(n_cls) + 2 +
ceil(n_cls / 64) + 6), __logf is v_log times ln 2 (3 relative to |log s|), m + . and . - x_y round once each (2, relative to the
row's magnitudes): 3 ln(n_cls) + ceil(n_cls / 64) + 13 against a row magnitude |m| + |log s| + |x_y| that is at least 1 on
average in every batch here (ln n_cls alone for near-equal logits; |m| and |x_y| otherwise).  The last workgroup's sum adds
ceil(n_rows / 256) terms per thread, 6 tree steps, 4 partial sums, and the product with inv_n and inv_n itself: + ceil(n_rows /
256) + 12.  All row terms are >= 0 up to rounding, so the sum's roundings are relative to mag_loss.

Non-finite logits.  -inf is a legitimate logit (a masked class) and takes its limit: probability and gradient exactly 0 on a
class that is not the label; on the label the loss is +inf and the element -1 / n.  The float64 reference would give NaN there
(inf - inf), so ce_terms evaluates -inf at -1e4, whose exponential is exactly 0.  +inf, NaN and a row of -inf only give torch
itself NaN over the whole row (established here on the CPU in fp32 for each batch, then asserted of the kernel in kind): that
one row per batch is asserted NaN element by element instead of being held to the bound, the loss is NaN, and no other row's
gradient moves by a bit.
Because such a batch has no finite loss to hold to the bound, every such batch also runs without the plant, where both bounds
apply in full.

A label outside [0, n_cls) (torch: a device assert; -100, torch's ignore_index, is NOT implemented and is refused like any
other) sets the error word, gives the row no loss term and no one-hot -- the gradient row is softmax / n, the divisor stays
n -- and CrossEntropyLoss.check_errors() raises and clears the word.

Measured on the MI355X, worst ratio to the bound per shape over scales 1, 3, 20, plain and confident rows, all five routes --
gradient / loss:
    (256, 41)  0.500 / 0.393    (1000, 100) 0.500 / 0.405    (7, 1000)  0.499 / 0.427    (32, 3)   0.500 / 0.408
    (1, 1)     0     / 0        (5, 2)      0.475 / 0.354    (300, 63)  0.500 / 0.425    (300, 64) 0.500 / 0.386
    (300, 65)  0.500 / 0.424    (33, 128)   0.498 / 0.365    (33, 129)  0.498 / 0.482    (4096, 7) 0.500 / 0.234
    (4097, 7)  0.500 / 0.209    (9001, 3)   0.500 / 0.412
i.e. the worst gradient element is always the final rounding's own half ulp -- the fast __expf / __logf forms and the p - 1
cancellation on confident rows stay inside the absolute term, so they are kept -- and the loss uses under half of its count.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

from bounds import CE_SHAPES, assert_within, ce_case, ce_check, ce_terms   # noqa: E402

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plain(x, y, state, d_stride=None, extra_rows=0, fill=9.0):
    """bliss_cross_entropy called directly: logits x (any row stride), gradient rows ``d_stride`` apart in a buffer of
    n + extra_rows rows filled with ``fill``.  Returns (loss [1], the whole gradient buffer, row losses)."""
    from bliss_gnn_amd import _lib
    n, c = x.shape
    assert x.stride(1) == 1
    d_stride = c if d_stride is None else d_stride
    dx = torch.full((n + extra_rows, d_stride), fill, dtype=torch.bfloat16, device=x.device)
    rows = torch.full((n,), -7.0, dtype=torch.float32, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.bliss_cross_entropy(x.data_ptr(), x.stride(0), y.data_ptr(), n, c, rows.data_ptr(), dx.data_ptr(), d_stride,
                                            loss.data_ptr(), state.data_ptr(), state.data_ptr() + 4, _stream()), "bliss_cross_entropy")
    torch.cuda.synchronize()
    return loss, dx, rows


def _masked(a, b, table, ids, lo, n_dev, denom, state):
    """bliss_cross_entropy_masked called directly on a capacity of a.shape[0] rows.  Returns (loss [1], gradient, row losses)."""
    from bliss_gnn_amd import _lib
    cap, C = a.shape
    dx = torch.full((cap, C), 9.0, dtype=torch.bfloat16, device=a.device)
    rows = torch.full((cap,), -7.0, dtype=torch.float32, device=a.device)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib.bliss_cross_entropy_masked(a.data_ptr(), a.stride(0), 0 if b is None else b.data_ptr(), 0 if b is None else b.stride(0),
                                                   table.data_ptr(), table.shape[0], ids.data_ptr(), lo, cap, n_dev.data_ptr(), denom, C,
                                                   rows.data_ptr(), dx.data_ptr(), dx.stride(0), loss.data_ptr(), state.data_ptr(),
                                                   state.data_ptr() + 4, _stream()), "bliss_cross_entropy_masked")
    torch.cuda.synchronize()
    return loss, dx, rows


def _clean(state):
    """Ticket and error word both 0."""
    return int(state[0]) == 0 and int(state[1]) == 0


@pytest.mark.parametrize("confident", [False, True])
@pytest.mark.parametrize("scale", [1, 3, 20])
@pytest.mark.parametrize("shape", CE_SHAPES)
def test_loss_and_gradient_per_element_vs_fp64(cuda, shape, scale, confident):
    """Every route to the kernel on one batch: forward() + backward() (and the same loss bits from a no-grad call),
    backward_from, backward_from_parts (two addends, labels gathered inside), and the masked entry point with and without the
    second addend.  Every gradient element and the loss within the bounds; ticket and error word 0 after each."""
    from bliss_gnn_amd.nn import CrossEntropyLoss
    n, c = shape
    what = "%s x%d%s" % (shape, scale, " confident" if confident else "")
    xc, yc = ce_case(shape, scale, confident, 11 + 7 * scale + confident)
    y = yc.to(cuda)
    lf = CrossEntropyLoss()
    # forward + backward
    x = xc.to(cuda).requires_grad_(True)
    loss = lf(x, y)
    assert loss.dtype == torch.bfloat16 and loss.dim() == 0
    loss.backward()
    assert x.grad.dtype == torch.bfloat16 and _clean(lf._state)
    ce_check(loss.detach(), x.grad, x.detach(), y, float(n), what + " forward", loss_bf16=True)
    with torch.no_grad():
        assert torch.equal(lf(x, y).view(torch.int16), loss.detach().view(torch.int16)) and _clean(lf._state)
    # backward_from
    x1 = xc.to(cuda).requires_grad_(True)
    l1 = lf.backward_from(x1, y)
    assert l1.dtype == torch.float32 and _clean(lf._state)
    ce_check(l1, x1.grad, x1.detach(), y, float(n), what + " backward_from")
    assert torch.equal(x1.grad.view(torch.int16), x.grad.view(torch.int16))
    # backward_from_parts: logits = bf16(a + b), labels = table[ids]
    gen = torch.Generator().manual_seed(5 + n + c)
    a = xc.to(cuda).requires_grad_(True)
    b = (torch.randn(n, c, generator=gen) * scale * 0.25).bfloat16().to(cuda).requires_grad_(True)
    V = n + 13
    ids = torch.randperm(V, generator=gen)[:n].to(torch.int32).to(cuda)
    table = torch.randint(0, c, (V,), generator=gen).to(cuda)
    table[ids.long()] = y
    l2 = lf.backward_from_parts(a, b, table, ids)
    assert _clean(lf._state) and torch.equal(a.grad, b.grad)
    ce_check(l2, a.grad, a.detach(), y, float(n), what + " backward_from_parts", x2=b.detach())
    # the masked entry point, every row valid, a divisor of its own
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    n_dev = torch.tensor([n], dtype=torch.int32, device=cuda)
    denom = float(2 * n + 3)
    for second in (None, b.detach()):
        lm, dxm, _ = _masked(a.detach(), second, table, ids + 1000, 1000, n_dev, denom, state)
        assert _clean(state)
        ce_check(lm, dxm, a.detach(), y, denom, what + " masked" + ("" if second is None else " two addends"), x2=second)


def test_non_unit_incoming_gradient(cuda):
    """(loss * 0.5).backward(): 0.5 x the gradient, to one more bf16 rounding."""
    from bliss_gnn_amd.nn import CrossEntropyLoss
    x, y = ce_case((300, 65), 3, False, 3)
    y = y.to(cuda)
    x1, x2 = x.to(cuda).requires_grad_(True), x.to(cuda).requires_grad_(True)
    lf = CrossEntropyLoss()
    lf(x1, y).backward()
    (lf(x2, y) * 0.5).backward()
    want = 0.5 * x1.grad.double()
    assert_within(x2.grad, want, torch.zeros_like(want), 1, 0.0, "0.5 x gradient")


@pytest.mark.parametrize("shape", [(300, 65), (33, 129), (5, 2), (1, 1), (4097, 7)])
def test_views_and_strides(cuda, shape):
    """Logits that are a column slice of a wider tensor (row stride > n_cls, base aligned to 2 bytes only) through the module, and
    by direct call a gradient buffer whose rows are further apart than n_cls: the same bits as the contiguous call, and every
    sentinel -- the columns beyond n_cls of each row, every row past the last -- unchanged bit for bit."""
    from bliss_gnn_amd.nn import CrossEntropyLoss
    n, c = shape
    xc, yc = ce_case(shape, 3, False, 31)
    y = yc.to(cuda)
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    l0, d0, r0 = _plain(xc.to(cuda), y, state)
    ce_check(l0, d0, xc.to(cuda), y, float(n), "%s contiguous" % (shape,))
    wide = torch.full((n, c + 3), 77.0, dtype=torch.bfloat16, device=cuda)
    wide[:, 1:1 + c] = xc.to(cuda)
    x = wide[:, 1:1 + c]
    assert x.stride(0) == c + 3 and x.data_ptr() % 4 == 2 and x.stride(1) == 1
    lf = CrossEntropyLoss()
    xr = x.detach().requires_grad_(True)
    l1 = lf.backward_from(xr, y)
    assert _clean(lf._state)
    assert torch.equal(l1.view(torch.int32).reshape(1), l0.view(torch.int32)) and torch.equal(xr.grad.view(torch.int16), d0.view(torch.int16))
    xf = x.detach().requires_grad_(True)
    lf(xf, y).backward()
    assert torch.equal(xf.grad.view(torch.int16), d0.view(torch.int16))
    # direct call: strided logits AND a strided gradient buffer with sentinels
    l2, d2, r2 = _plain(x, y, state, d_stride=c + 5, extra_rows=3, fill=-3.0)
    assert _clean(state)
    sentinel = torch.full((1,), -3.0, dtype=torch.bfloat16, device=cuda).view(torch.int16)
    assert torch.equal(l2.view(torch.int32), l0.view(torch.int32)) and torch.equal(r2.view(torch.int32), r0.view(torch.int32))
    assert torch.equal(d2[:n, :c].contiguous().view(torch.int16), d0.view(torch.int16))
    assert bool((d2[:n, c:].contiguous().view(torch.int16) == sentinel).all()) and bool((d2[n:].view(torch.int16) == sentinel).all())
    assert bool((wide[:, 0] == 77.0).all()) and bool((wide[:, 1 + c:] == 77.0).all())


# ------------------------------------------------------------------------------------------------ non-finite logits
def _off_label(y, r, c, k=1):
    return (int(y[r]) + k) % c


@pytest.mark.parametrize("shape", [(32, 3), (33, 129), (300, 65)])
def test_minus_inf_logits_take_their_limit(cuda, shape):
    """-inf on classes that are not the label: gradient exactly 0 there, the rest of the row and the loss within the bounds.
    -inf on the label: loss +inf, that element -1 / n within the bound.  The same batch without the plants: both bounds."""
    n, c = shape
    xc, yc = ce_case(shape, 3, False, 41)
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    y = yc.to(cuda)
    l, d, _ = _plain(xc.to(cuda), y, state)
    ce_check(l, d, xc.to(cuda), y, float(n), "%s without plants" % (shape,))
    x1 = xc.clone()
    spots = [(3, _off_label(yc, 3, c)), (7, _off_label(yc, 7, c, 2)), (n - 1, _off_label(yc, n - 1, c))]
    for r, k in spots:
        x1[r, k] = -float("inf")
    l, d, _ = _plain(x1.to(cuda), y, state)
    assert _clean(state) and bool(torch.isfinite(l)) and bool(torch.isfinite(d.float()).all())
    for r, k in spots:
        assert float(d[r, k]) == 0.0
    ce_check(l, d, x1.to(cuda), y, float(n), "%s -inf off the label" % (shape,))
    x2 = x1.clone()
    x2[5, int(yc[5])] = -float("inf")
    l, d, rows = _plain(x2.to(cuda), y, state)
    assert _clean(state) and float(l) == float("inf") and float(rows[5]) == float("inf") and bool(torch.isfinite(d.float()).all())
    ce_check(l, d, x2.to(cuda), y, float(n), "%s -inf on the label" % (shape,))
    assert abs(float(d[5, int(yc[5])]) + 1.0 / n) <= 2.0 ** -8 / n


@pytest.mark.parametrize("kind", ["+inf", "+inf on the label", "row of -inf", "nan", "nan on the label"])
@pytest.mark.parametrize("shape", [(32, 3), (33, 129)])
def test_plus_inf_nan_and_empty_rows_agree_with_torch_in_kind(cuda, shape, kind):
    """What torch.nn.functional.cross_entropy gives in fp32 on the CPU for the planted batch (NaN over the planted row and in the
    loss, every other row finite) is what the kernel gives: NaN exactly where torch has NaN, confined to that row's gradient and
    the scalar loss; all other rows within the bound and bit-equal to the unplanted batch's.  The unplanted batch: both bounds in
    full."""
    n, c = shape
    xc, yc = ce_case(shape, 3, False, 43)
    r = 6
    x1 = xc.clone()
    if kind == "+inf":
        x1[r, _off_label(yc, r, c)] = float("inf")
    elif kind == "+inf on the label":
        x1[r, int(yc[r])] = float("inf")
    elif kind == "row of -inf":
        x1[r] = -float("inf")
    elif kind == "nan":
        x1[r, _off_label(yc, r, c)] = float("nan")
    else:
        x1[r, int(yc[r])] = float("nan")
    xt = x1.float().requires_grad_(True)
    lt = torch.nn.functional.cross_entropy(xt, yc)
    lt.backward()
    nan_t = torch.isnan(xt.grad)
    assert bool(nan_t[r].all()) and int(nan_t.sum()) == c and bool(torch.isnan(lt))          # what torch does, established
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    y = yc.to(cuda)
    l0, d0, _ = _plain(xc.to(cuda), y, state)
    ce_check(l0, d0, xc.to(cuda), y, float(n), "%s without the plant" % (shape,))
    l, d, rows = _plain(x1.to(cuda), y, state)
    assert _clean(state)
    assert torch.equal(torch.isnan(d.float()).cpu(), nan_t) and bool(torch.isnan(l))
    assert bool(torch.isfinite(rows[torch.arange(n, device=cuda) != r]).all())
    ce_check(l, d, x1.to(cuda), y, float(n), "%s %s, other rows" % (shape, kind), skip_rows=[r])
    keep = torch.arange(n, device=cuda) != r
    assert torch.equal(d[keep].view(torch.int16), d0[keep].view(torch.int16))               # no other row moved


# ------------------------------------------------------------------------------------------------ labels out of range
@pytest.mark.parametrize("shape", [(300, 65), (4097, 7)])
def test_labels_out_of_range_raise_the_word_and_check_errors(cuda, shape):
    """y = -1, n_cls and -100 on three rows: the error word is set, those rows' loss terms are 0 and their gradient rows the
    softmax alone, every other row within the bound with the divisor the kernel uses (n, the refused rows included);
    check_errors() raises naming labels out of range and clears the word; the next launch on the same state with good labels is
    within both bounds and leaves the word 0."""
    from bliss_gnn_amd.nn import BCEWithLogitsLoss, CrossEntropyLoss
    n, c = shape
    xc, yc = ce_case(shape, 3, False, 47)
    bad_rows = [2, n // 2, n - 1]
    yb = yc.clone()
    yb[bad_rows[0]], yb[bad_rows[1]], yb[bad_rows[2]] = -1, c, -100
    lf = CrossEntropyLoss()
    lf.check_errors()                                            # no state yet: nothing to report
    x = xc.to(cuda).requires_grad_(True)
    loss = lf.backward_from(x, yb.to(cuda))
    assert int(lf._state[0]) == 0 and int(lf._state[1]) != 0
    ce_check(loss, x.grad, x.detach(), yb.to(cuda), float(n), "%s with three refused rows" % (shape,))
    _, _, rows = _plain(xc.to(cuda), yb.to(cuda), lf._state)
    assert not rows[bad_rows].any() and bool((rows[[1, 3, n - 2]] > 0).all())
    with pytest.raises(RuntimeError, match="labels out of range"):
        lf.check_errors()
    assert _clean(lf._state)
    lf.check_errors()                                            # cleared: silent
    x = xc.to(cuda).requires_grad_(True)
    loss = lf.backward_from(x, yc.to(cuda))
    assert _clean(lf._state)
    ce_check(loss, x.grad, x.detach(), yc.to(cuda), float(n), "%s good labels after the refused ones" % (shape,))
    lf.check_errors()
    # the multi-label module's word: a label id outside the target table (backward_from_parts)
    bl = BCEWithLogitsLoss()
    bl.check_errors()
    a = xc.to(cuda).requires_grad_(True)
    b = torch.zeros_like(a).requires_grad_(True)
    table = torch.zeros(n + 5, c, dtype=torch.float32, device=cuda)
    ids = torch.arange(n, dtype=torch.int32, device=cuda)
    bl.backward_from_parts(a, b, table, ids)
    bl.check_errors()
    assert _clean(bl._state)


# ------------------------------------------------------------------------------------------------ the masked form
@pytest.mark.parametrize("cap,C", [(96, 41), (4100, 7)])
def test_masked_form_row_counts_and_ids(cuda, cap, C):
    """bliss_cross_entropy_masked with *n_rows_dev = 0, 1, cap - 1, cap, cap + 5 and -3 (clamped to [0, cap]): padding rows get
    exactly +0 gradient rows and a row loss of 0 although they hold NaN logits and ids outside the table (which raise nothing);
    the loss divides by `denom`; the valid rows are within both bounds; an id outside the table on a VALID row raises the word,
    and that row has no loss term and no one-hot."""
    gen = torch.Generator().manual_seed(3)
    lo, n_table, denom = 1000, 500, 512.0
    a0 = (torch.randn(cap, C, generator=gen) * 3).bfloat16()
    b = (torch.randn(cap, C, generator=gen) * 3).bfloat16().to(cuda)
    table = torch.randint(0, C, (n_table,), generator=gen).to(cuda)
    ids0 = torch.randint(lo, lo + n_table, (cap,), generator=gen).to(torch.int32)
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    for n_dev in (0, 1, cap - 1, cap, cap + 5, -3):
        n = max(0, min(n_dev, cap))
        a, ids = a0.clone(), ids0.clone()
        a[n:] = float("nan")
        ids[n:] = torch.tensor([7, lo + n_table, -5, 2 ** 31 - 1], dtype=torch.int32).repeat(cap)[:cap - n]     # (another rank's nodes)
        a, ids = a.to(cuda), ids.to(cuda)
        nd = torch.tensor([n_dev], dtype=torch.int32, device=cuda)
        y = torch.full((cap,), -1, dtype=torch.int64, device=cuda)
        y[:n] = table[ids[:n].long() - lo]
        for second in (b, None):
            loss, dx, rows = _masked(a, second, table, ids, lo, nd, denom, state)
            what = "masked cap %d n_rows_dev %d%s" % (cap, n_dev, "" if second is None else " two addends")
            assert _clean(state), what
            assert not dx[n:].view(torch.int16).any() and not rows[n:].view(torch.int32).any(), what
            if n == 0:
                assert float(loss) == 0.0
            a_ref = torch.where(torch.isnan(a), torch.zeros_like(a), a)                      # (padding rows: never read)
            ce_check(loss, dx, a_ref, y, denom, what, x2=second, n_valid=n)
    # ids outside the table on valid rows
    n = cap - 7
    a, ids = a0.to(cuda), ids0.clone()
    ids[5], ids[9], ids[n - 1] = lo + n_table, lo - 1, -4
    ids = ids.to(cuda)
    y = torch.full((cap,), -1, dtype=torch.int64, device=cuda)
    good = torch.ones(n, dtype=torch.bool, device=cuda)
    good[[5, 9, n - 1]] = False
    y[:n][good] = table[ids[:n][good].long() - lo]
    loss, dx, rows = _masked(a, b, table, ids, lo, torch.tensor([n], dtype=torch.int32, device=cuda), denom, state)
    assert int(state[0]) == 0 and int(state[1]) == 2                # (BLISS_ERR_CAP_CAND)
    state.zero_()
    assert not rows[[5, 9, n - 1]].any()
    ce_check(loss, dx, a, y, denom, "masked cap %d with three ids outside the table" % cap, x2=b, n_valid=n)


# ------------------------------------------------------------------------------------------------ ticket and determinism
def test_ticket_returns_to_zero_and_loss_bits_repeat(cuda):
    """One state tensor, 40 launches in a row with 1, 5, 4097, 256 and 9001 rows in turn (1, 2, 1024, 64 and 1024 workgroups: the
    ticket is taken by grids of every size, the full one included, and the rows of the second and third trip of the grid-stride
    loop enter the row-ordered sum): the ticket is 0 after each launch, every repeat of an input gives the loss and gradient
    bits of its first launch, each within both bounds; a 9001-row launch straight after a 1-row launch gives those bits too."""
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    counts = [1, 5, 4097, 256, 9001]
    data, first = {}, {}
    for n in counts:
        x, y = ce_case((n, 3), 3, False, 53 + n)
        data[n] = (x.to(cuda), y.to(cuda))
    for i in range(40):
        n = counts[i % len(counts)]
        x, y = data[n]
        loss, dx, _ = _plain(x, y, state)
        assert _clean(state), (i, n)
        if n not in first:
            ce_check(loss, dx, x, y, float(n), "launch %d, %d rows" % (i, n))
            first[n] = (loss.clone(), dx.clone())
        else:
            assert torch.equal(loss.view(torch.int32), first[n][0].view(torch.int32)), (i, n)
            assert torch.equal(dx.view(torch.int16), first[n][1].view(torch.int16)), (i, n)
    _plain(*data[1], state)
    loss, dx, _ = _plain(*data[9001], state)
    assert _clean(state)
    assert torch.equal(loss.view(torch.int32), first[9001][0].view(torch.int32)) and torch.equal(dx.view(torch.int16), first[9001][1].view(torch.int16))
