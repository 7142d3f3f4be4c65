"""The micro-F1 rule of include/bliss_gnn.h (bliss_f1_multiclass / bliss_f1_multilabel) restated in NumPy, and the seeded
inputs the metric tests share (tests/test_metrics_ref.py on the CPU, tests/test_gpu_metrics.py on the GPU).

The rule (normative):

  single-label  The prediction of a row is the FIRST index of its largest logit.  A NaN logit counts as larger than
                everything and the first NaN wins.  +0 and -0 are equal.  A row of -inf predicts 0.  A correct row adds
                tp += 1, a wrong row fp += 1 and fn += 1, every counted row n += 1.  A label outside [0, n_cls) raises the
                error flag and the row is left out of all four counts.
  multi-label   hit = x > 0, y = target > 0.5, counted per (row, class) pair, n += n_cls per row.  NaN is no hit on both sides,
                x = +-0 is no hit.  (x > 0 is sigmoid(x) > 0.5 exactly; an fp32 sigmoid rounds to 0.5 for 0 < x < 2^-23.)
  Only the first min(max(n_valid, 0), n_rows) rows count.  micro-F1 = 2 tp / max(2 tp + fp + fn, 1).

Every function takes torch CPU tensors (bf16 or fp32 logits) and returns ((tp, fp, fn, n), error_flag) as Python values.
"""
import numpy as np
import torch


def _f32(x):
    return x.detach().cpu().float().numpy()


def _n_valid(n_rows, n_valid):
    return n_rows if n_valid is None else min(max(int(n_valid), 0), n_rows)


def predict(x):
    """First index of the largest logit per row; NaN above everything, first NaN wins (np.argmax: first occurrence)."""
    x = _f32(x)
    nan = np.isnan(x)
    top = np.where(nan.any(1, keepdims=True), nan, x == np.where(nan, -np.inf, x).max(1, keepdims=True))
    return top.argmax(1)


def multiclass_counts(x, y, n_valid=None):
    n_rows, n_cls = x.shape
    y = y.detach().cpu().numpy().astype(np.int64)
    rows = np.arange(n_rows) < _n_valid(n_rows, n_valid)
    bad = rows & ((y < 0) | (y >= n_cls))
    rows = rows & ~bad
    right = rows & (predict(x) == y)
    tp, wrong = int(right.sum()), int((rows & ~right).sum())
    return (tp, wrong, wrong, int(rows.sum())), bool(bad.any())


def multilabel_counts(x, t, n_valid=None):
    n_rows, n_cls = x.shape
    rows = (np.arange(n_rows) < _n_valid(n_rows, n_valid))[:, None]
    hit, pos = _f32(x) > 0, _f32(t) > 0.5
    return (int((hit & pos & rows).sum()), int((hit & ~pos & rows).sum()), int((~hit & pos & rows).sum()),
            int(rows.sum()) * n_cls), False


def micro_f1(counts):
    tp, fp, fn, _ = counts
    return 2.0 * tp / max(2.0 * tp + fp + fn, 1.0)


# ------------------------------------------------------------------------------------------------------------- inputs
TINY = 2.0 ** -30                                          # a hit by the rule; an fp32 sigmoid of it is exactly 0.5
MULTICLASS_SHAPES = [(1, 1), (5, 2), (32, 3), (300, 63), (300, 64), (300, 65), (33, 128), (33, 129), (7, 1000)]
MULTILABEL_SHAPES = [(1, 1), (33, 5), (300, 63), (300, 64), (300, 65), (4097, 5), (9001, 3), (40, 121)]


def multiclass_case(rows, classes, scale=1.0, seed=0, bad_labels=False):
    """bf16 logits N(0, 1) * scale and int64 labels (about half of them the rule's own prediction), with planted rows when the
    shape has room (rows >= 16): all logits equal; a tie between the first and last class; NaN first, last and twice; +inf;
    all -inf; +-0 pairs; +inf ahead of a NaN.  ``bad_labels``: rows 10..12 get the labels -1, n_cls and -100."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + classes)
    x = (torch.randn(rows, classes, generator=g) * scale).bfloat16()
    nan, inf, last = float("nan"), float("inf"), classes - 1
    planted = rows >= 16
    if planted:
        x[0, :] = 1.5
        x[1, :] = -1.0; x[1, 0] = 3.0; x[1, last] = 3.0
        x[2, 0] = nan
        x[3, last] = nan
        x[4, classes // 2] = nan; x[4, last] = nan
        x[5, last] = inf
        x[6, :] = -inf
        x[7, :] = -1.0; x[7, 0] = -0.0; x[7, last] = 0.0
        x[8, :] = -1.0; x[8, 0] = 0.0; x[8, last] = -0.0
        x[9, 0] = inf; x[9, last] = nan
    y = torch.randint(0, classes, (rows,), generator=g)
    own = torch.from_numpy(predict(x))
    take = torch.rand(rows, generator=g) < 0.5
    y[take] = own[take]
    if planted:
        y[:10] = own[:10]                                 # the rule calls every planted row correct: a changed rule loses them
        if bad_labels:
            y[10], y[11], y[12] = -1, classes, -100
    return x, y


def multilabel_case(rows, classes, seed=0, tiny=True):
    """bf16 logits N(0, 1), fp32 targets in {0, 1} (40 % ones), with planted pairs when there is room (>= 32 pairs): x = 0, -0,
    NaN, +-inf (each under a 1 and under a 0 target), targets of exactly 0.5, and -- ``tiny`` -- x = 2^-30 under a 1 target."""
    g = torch.Generator().manual_seed(2000 * seed + 7 * rows + classes)
    x = torch.randn(rows, classes, generator=g).bfloat16()
    t = (torch.rand(rows, classes, generator=g) < 0.4).float()
    if rows * classes >= 32:
        xf, tf = x.view(-1), t.view(-1)
        vals = [0.0, -0.0, float("nan"), float("inf"), -float("inf")]
        for k, v in enumerate(vals):
            xf[2 * k], tf[2 * k] = v, 1.0
            xf[2 * k + 1], tf[2 * k + 1] = v, 0.0
        xf[10], tf[10] = 1.0, 0.5
        xf[11], tf[11] = -1.0, 0.5
        if tiny:
            xf[12], tf[12] = TINY, 1.0
    return x, t


def smallest_nonzero(x):
    a = np.abs(_f32(x))
    a = a[(a > 0) & np.isfinite(a)]
    return float(a.min()) if a.size else float("inf")
