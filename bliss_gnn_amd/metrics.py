"""Micro-F1 kept on the device (csrc/metrics.hip): ``train_acc`` / ``val_acc`` of the reference
(torchmetrics Multiclass / MultilabelF1Score(average='micro'), train_lightning.py:68-70, updated per batch at :143 and
:179-203) as four int64 counts {tp, fp, fn, n} that every ``update`` ADDS to with one launch and nothing reads back until
``compute``.  The rule is the header's (include/bliss_gnn.h: bliss_f1_multiclass / bliss_f1_multilabel):

  single-label  prediction = first index of the row's largest logit, NaN above everything (first NaN wins), +0 == -0, a row of
                -inf predicts 0; correct: tp += 1, wrong: fp += 1 and fn += 1, n += 1 per counted row; a label outside
                [0, n_cls) sets the error word and the row is in no count.
  multi-label   per (row, class) pair hit = x > 0, y = target > 0.5; NaN and +-0 are no hit; n += n_cls per counted row.
                (``fit.micro_f1`` thresholds an fp32 sigmoid at 0.5, which differs only for 0 < x < ~2^-23.)
"""
import torch

from . import _lib

ERR_LABEL = 2                                              # BLISS_ERR_CAP_CAND: the bit the loss kernels use for the same condition


def _stream():
    return torch.cuda.current_stream().cuda_stream


def micro_f1_from_counts(counts, multilabel=False, device=None):
    """The float ``fit.micro_f1`` returns for predictions with these counts, bit for bit.  Multi-label: the same double
    expression on the same integers.  Single-label: ``fit.micro_f1`` takes the fp32 ``mean`` of n indicator values on the
    predictions' device, whose rounding is the device's (a product with 1/n on the GPU, a quotient on the CPU); the same
    reduction over an indicator vector holding tp ones reproduces it (its sum is an exact integer in any order)."""
    tp, fp, fn, n = (int(c) for c in counts)
    if multilabel:
        return 2.0 * tp / max(2.0 * tp + fp + fn, 1.0)
    if n <= 0:
        return 0.0
    return float((torch.arange(n, device=device) < tp).float().mean())


class MicroF1:
    """``MicroF1(multilabel=False)``: ``update`` only enqueues; ``compute`` is the one read-back.

    ``update(pred, labels)``: logits [n, n_cls] against labels (int64 [n], or fp32 [n, n_cls] when multi-label).
    ``update(pred, label_table=t, label_ids=i)``: row r's label is ``t[i[r]]`` (int32 ids), never gathered.
    ``row_ids`` (int32): row r reads ``pred[row_ids[r]]`` -- ``pred[nid]`` of a full-graph prediction, never sliced.
    ``n_rows_dev`` (int32 tensor on the device): only the first ``min(max(n_rows_dev, 0), n)`` rows count.

    bf16 logits on the GPU with unit column stride take the kernel; any other input takes torch ops that implement the same
    rule on the input's device (the counterpart of ``_eligible`` in the loss modules)."""

    def __init__(self, multilabel=False):
        self.multilabel = bool(multilabel)
        self._counts = self._err = None
        self._seen = (0, 0, 0, 0)

    # -- state ------------------------------------------------------------------------------------------------------------
    def _state_on(self, device):
        if self._counts is None or self._counts.device != device:
            if self._counts is not None and any(self.counts()):
                raise ValueError("MicroF1 holds counts on %s; reset() before updating from %s" % (self._counts.device, device))
            self._counts = torch.zeros(4, dtype=torch.int64, device=device)          # tp, fp, fn, n
            self._err = torch.zeros(1, dtype=torch.int32, device=device)
        return self._counts, self._err

    def counts(self):
        """(tp, fp, fn, n) as Python ints: one read-back."""
        if self._counts is None:
            return (0, 0, 0, 0)
        return tuple(int(v) for v in self._counts.tolist())

    def delta(self):
        """The counts added since the previous ``delta()`` / ``reset()`` (one read-back): the last batch's, when called after
        every update."""
        cur = self.counts()
        out = tuple(c - s for c, s in zip(cur, self._seen))
        self._seen = cur
        return out

    def compute(self):
        tp, fp, fn, _ = self.counts()
        return 2.0 * tp / max(2.0 * tp + fp + fn, 1.0)

    def reset(self):
        if self._counts is not None:
            self._counts.zero_()
        self._seen = (0, 0, 0, 0)

    def check_errors(self):
        """Read the error word, clear it, and raise if a label (or a label / row id) was out of range: those rows were counted
        nowhere.  One tiny read-back: call it where the loop synchronises anyway."""
        if self._err is None:
            return
        word = int(self._err.item())
        if word:
            self._err.zero_()
            raise RuntimeError("MicroF1: labels out of range -- a class index outside [0, n_classes), a label id outside the label "
                               "table or a row id outside the prediction (error 0x%x, %s); the rows concerned are in no count"
                               % (word, _lib.err_string(word)))

    # -- update -----------------------------------------------------------------------------------------------------------
    def _eligible(self, pred, labels, table, ids, row_ids, n_rows_dev):
        dev = pred.device
        lab = labels if labels is not None else table
        ok = (pred.is_cuda and pred.dtype == torch.bfloat16 and pred.dim() == 2 and pred.stride(1) == 1 and pred.numel() > 0
              and lab.device == dev and lab.is_contiguous() and not lab.requires_grad)
        if self.multilabel:
            ok = ok and lab.dtype == torch.float32 and lab.dim() == 2 and lab.shape[1] == pred.shape[1]
        else:
            ok = ok and lab.dtype == torch.int64 and lab.dim() == 1
        for t in (ids, row_ids):
            ok = ok and (t is None or (t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == dev))
        return bool(ok and (n_rows_dev is None or (n_rows_dev.dtype == torch.int32 and n_rows_dev.device == dev and n_rows_dev.numel() == 1)))

    def update(self, pred, labels=None, *, label_table=None, label_ids=None, row_ids=None, n_rows_dev=None):
        if (labels is None) == (label_table is None or label_ids is None) or (labels is not None and (label_table is not None or label_ids is not None)):
            raise ValueError("MicroF1.update takes either labels or (label_table, label_ids)")
        if pred.dim() != 2:
            raise ValueError("MicroF1.update: logits must be [rows, classes]")
        pred = pred.detach()
        n_rows = int(row_ids.numel()) if row_ids is not None else int(pred.shape[0])
        n_lab = int(labels.shape[0]) if labels is not None else int(label_ids.numel())
        if n_lab != n_rows:
            raise ValueError("MicroF1.update: %d labels for %d rows" % (n_lab, n_rows))
        if self.multilabel and (labels if labels is not None else label_table).shape[-1] != pred.shape[1]:
            raise ValueError("MicroF1.update: multi-label targets must have one column per class")
        counts, err = self._state_on(pred.device)
        if n_rows == 0:
            return
        if not self._eligible(pred, labels, label_table, label_ids, row_ids, n_rows_dev):
            return self._update_torch(pred, labels, label_table, label_ids, row_ids, n_rows_dev, n_rows)
        n_cls = int(pred.shape[1])
        fn = _lib.lib.bliss_f1_multilabel if self.multilabel else _lib.lib.bliss_f1_multiclass
        p = lambda t: 0 if t is None else t.data_ptr()
        _lib.check(fn(pred.data_ptr(), max(int(pred.stride(0)), n_cls), int(pred.shape[0]), p(row_ids), p(labels), p(label_table),
                      0 if label_table is None else int(label_table.shape[0]), p(label_ids), n_rows, p(n_rows_dev), n_cls,
                      counts.data_ptr(), err.data_ptr(), _stream()),
                   "bliss_f1_multilabel" if self.multilabel else "bliss_f1_multiclass")

    def _update_torch(self, pred, labels, table, ids, row_ids, n_rows_dev, n_rows):
        """The rule in torch ops on ``pred``'s device; like the kernel it only enqueues (masks, no data-dependent shapes)."""
        dev, n_cls = pred.device, int(pred.shape[1])
        ok = torch.ones(n_rows, dtype=torch.bool, device=dev)
        if n_rows_dev is not None:
            ok &= torch.arange(n_rows, device=dev) < n_rows_dev.to(dev).reshape(()).clamp(0, n_rows)
        bad = torch.zeros(n_rows, dtype=torch.bool, device=dev)

        def pick(src, idx):
            nonlocal bad
            idx = idx.to(dev).long()
            out = (idx < 0) | (idx >= src.shape[0])
            bad = bad | out
            return src.to(dev)[idx.masked_fill(out | ~ok, 0)]

        x = (pick(pred, row_ids) if row_ids is not None else pred).float()
        y = pick(table, ids) if labels is None else labels.to(dev)
        if self.multilabel:
            hit, pos = x > 0, y.float() > 0.5
            rows = (ok & ~bad)[:, None]
            c = [(hit & pos & rows).sum(), (hit & ~pos & rows).sum(), (~hit & pos & rows).sum(), rows.sum() * n_cls]
        else:
            y = y.long()
            bad = bad | (y < 0) | (y >= n_cls)
            nan = torch.isnan(x)
            top = torch.where(nan.any(1, keepdim=True), nan, x == x.masked_fill(nan, -float("inf")).max(1, keepdim=True).values)
            col = torch.arange(n_cls, device=dev).expand(n_rows, n_cls)
            guess = col.masked_fill(~top, n_cls).min(1).values                       # the FIRST of the largest
            rows = ok & ~bad
            right = (guess == y) & rows
            wrong = (rows & ~right).sum()
            c = [right.sum(), wrong, wrong, rows.sum()]
        self._counts += torch.stack(c).to(torch.int64)
        self._err |= ((bad & ok).any().to(torch.int32) * ERR_LABEL)
