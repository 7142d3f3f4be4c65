"""CPU suite: the NumPy restatement of the micro-F1 rule (tests/metrics_ref.py) that the GPU tests compare the kernels with is
itself checked here: against fit.micro_f1 and torch.argmax on the GPU tests' own seeded inputs, and by planting faults into
copies of it -- each fault must change the counts on those inputs, or the inputs would not notice a kernel with that fault."""
import numpy as np
import pytest
import torch

import metrics_ref as ref

SC_CASES = [(r, c, s) for (r, c) in ref.MULTICLASS_SHAPES for s in (1.0, 20.0)] + [(4096, 7, 1.0), (4097, 7, 20.0), (9001, 3, 1.0)]


def _sum(cs):
    return tuple(int(v) for v in np.sum(np.array(cs, dtype=np.int64), axis=0))


def test_restatement_is_fit_micro_f1_single_label():
    from bliss_gnn_amd.fit import micro_f1
    for r, c, s in SC_CASES:
        x, y = ref.multiclass_case(r, c, s, seed=1)
        (tp, fp, fn, n), flagged = ref.multiclass_counts(x, y)
        assert not flagged and n == r and fp == fn == r - tp
        for xx in (x, x.float()):                                      # torch.argmax: first of the largest, NaN first -- bf16 and fp32
            assert np.array_equal(ref.predict(x), xx.argmax(1).numpy()), (r, c, s, xx.dtype)
        assert micro_f1(x.float(), y) == pytest.approx(ref.micro_f1((tp, fp, fn, n)), abs=1e-6)
        assert micro_f1(x.float(), y) == float(np.float32(tp) / np.float32(r))


def test_restatement_is_fit_micro_f1_multi_label():
    from bliss_gnn_amd.fit import micro_f1
    for r, c in ref.MULTILABEL_SHAPES:
        x, t = ref.multilabel_case(r, c, seed=1, tiny=False)
        assert ref.smallest_nonzero(x) >= 2.0 ** -20                   # (what lets an fp32 sigmoid agree with x > 0)
        counts, _ = ref.multilabel_counts(x, t)
        assert counts[3] == r * c
        assert micro_f1(x.float(), t, multilabel=True) == ref.micro_f1(counts), (r, c)


def test_the_documented_difference_to_an_fp32_sigmoid():
    from bliss_gnn_amd.fit import micro_f1
    x = torch.tensor([[ref.TINY]]).bfloat16()
    assert float(x) == ref.TINY
    t = torch.ones(1, 1)
    assert ref.multilabel_counts(x, t)[0] == (1, 0, 0, 1)              # the rule: x > 0 is a hit
    assert float(torch.sigmoid(x.float())) == 0.5                      # the fp32 sigmoid rounds to 0.5: fit.micro_f1 sees no hit
    assert micro_f1(x.float(), t, multilabel=True) == 0.0 and ref.micro_f1((1, 0, 0, 1)) == 1.0


# ---------------------------------------------------------------------------------------------------- planted faults
def _multiclass_faulty(x, y, n_valid=None, fault=None):
    n_rows, n_cls = x.shape
    xf, yy = ref._f32(x), y.numpy().astype(np.int64)
    nan = np.isnan(xf)
    if fault == "nan_skipped":
        top = xf == np.where(nan, -np.inf, xf).max(1, keepdims=True)
        top = np.where(top.any(1, keepdims=True), top, np.arange(n_cls)[None, :] == 0)
    else:
        top = np.where(nan.any(1, keepdims=True), nan, xf == np.where(nan, -np.inf, xf).max(1, keepdims=True))
    guess = n_cls - 1 - top[:, ::-1].argmax(1) if fault == "ties_last" else top.argmax(1)
    rows = np.arange(n_rows) < (n_rows if fault == "padding_counted" else ref._n_valid(n_rows, n_valid))
    bad = rows & ((yy < 0) | (yy >= n_cls))
    if fault != "bad_label_wrong":
        rows = rows & ~bad
    right = rows & (guess == yy)
    tp, wrong = int(right.sum()), int((rows & ~right).sum())
    return (tp, wrong, wrong, int(rows.sum()))


def _multilabel_faulty(x, t, n_valid=None, fault=None):
    n_rows, n_cls = x.shape
    rows = (np.arange(n_rows) < (n_rows if fault == "padding_counted" else ref._n_valid(n_rows, n_valid)))[:, None]
    xf = ref._f32(x)
    hit, pos = (xf >= 0) if fault == "ge_zero" else (xf > 0), ref._f32(t) > 0.5
    n = int(rows.sum()) * (1 if fault == "n_per_row" else n_cls)
    return (int((hit & pos & rows).sum()), int((hit & ~pos & rows).sum()), int((~hit & pos & rows).sum()), n)


def _sc_inputs():
    for r, c, s in SC_CASES:
        if r >= 16:
            x, y = ref.multiclass_case(r, c, s, seed=1, bad_labels=True)
            yield x, y, r - 5


def _ml_inputs():
    for r, c in ref.MULTILABEL_SHAPES:
        if r * c >= 32 and r > 5:
            x, t = ref.multilabel_case(r, c, seed=1)
            yield x, t, r - 5


def test_copies_without_a_fault_are_the_restatement():
    for x, y, nv in _sc_inputs():
        assert _multiclass_faulty(x, y, nv) == ref.multiclass_counts(x, y, nv)[0]
    for x, t, nv in _ml_inputs():
        assert _multilabel_faulty(x, t, nv) == ref.multilabel_counts(x, t, nv)[0]


@pytest.mark.parametrize("fault", ["ties_last", "nan_skipped", "padding_counted", "bad_label_wrong"])
def test_every_planted_fault_changes_the_single_label_counts(fault):
    for x, y, nv in _sc_inputs():                                      # on EVERY planted input, not just in total
        assert _multiclass_faulty(x, y, nv, fault) != ref.multiclass_counts(x, y, nv)[0], (fault, tuple(x.shape))


@pytest.mark.parametrize("fault", ["ge_zero", "padding_counted", "n_per_row"])
def test_every_planted_fault_changes_the_multi_label_counts(fault):
    for x, t, nv in _ml_inputs():
        if fault == "n_per_row" and x.shape[1] == 1:
            continue
        assert _multilabel_faulty(x, t, nv, fault) != ref.multilabel_counts(x, t, nv)[0], (fault, tuple(x.shape))


def test_device_side_row_count_is_clamped():
    x, y = ref.multiclass_case(40, 5, seed=2)
    full = ref.multiclass_counts(x, y)[0]
    assert ref.multiclass_counts(x, y, 45)[0] == full and ref.multiclass_counts(x, y, -3)[0] == (0, 0, 0, 0)
    assert ref.multiclass_counts(x, y, 1)[0][3] == 1
