"""CPU suite: the micro-F1 entry points (csrc/metrics.hip) are exported, bound and validate their arguments on the host (a
refused call launches nothing, so this runs without a GPU); MicroF1 on CPU tensors takes the torch-op route of the same rule."""
import ctypes as C

import pytest
import torch

import metrics_ref as ref

NAMES = ("bliss_f1_multiclass", "bliss_f1_multilabel")


def test_symbols_are_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n]) == 14
        assert getattr(_lib.lib, n).argtypes is not None
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.metrics import MicroF1
    assert bg.MicroF1 is MicroF1
    hdr = open(__graft_entry__.ROOT + "/include/bliss_gnn.h").read()
    assert "#define BLISS_F1_MAX_WORKGROUPS %d" % _lib.F1_MAX_WORKGROUPS in hdr


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_refuse_bad_arguments_before_any_launch(name):
    from bliss_gnn_amd import _lib
    fn, E = getattr(_lib.lib, name), _lib.EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    # (logits, stride, n_pred_rows, row_ids, labels, label_table, n_table, label_ids, n_rows, n_rows_dev, n_cls, counts, err, stream)
    direct = [p, 8, 4, 0, p, 0, 0, 0, 4, 0, 3, p, p, 0]
    table = [p, 8, 4, p, 0, p, 9, p, 4, p, 3, p, p, 0]
    for good in (direct, table):
        for i in (0, 11, 12):                                                              # null logits, counts, err
            a = list(good); a[i] = 0
            assert fn(*a) == E, i
        for i, v in ((10, 0), (10, -2), (8, -1), (1, 2), (2, -1), (6, -1)):                # n_cls <= 0, n_rows < 0, stride < n_cls, ...
            a = list(good); a[i] = v
            assert fn(*a) == E, (i, v)
    a = list(direct); a[4] = 0
    assert fn(*a) == E                                                                     # neither labels nor (table, ids)
    a = list(table); a[5] = 0
    assert fn(*a) == E                                                                     # ids without a table
    a = list(table); a[7] = 0
    assert fn(*a) == E                                                                     # a table without ids
    a = list(table); a[4] = p
    assert fn(*a) == E                                                                     # both forms
    a = list(direct); a[8] = 0
    assert fn(*a) == 0                                                                     # no rows: nothing launched, no error


@pytest.mark.parametrize("multilabel", [False, True])
def test_cpu_tensors_take_the_torch_route_of_the_same_rule(multilabel):
    from bliss_gnn_amd.metrics import MicroF1, micro_f1_from_counts
    m, want = MicroF1(multilabel), [0, 0, 0, 0]
    for i, (r, c) in enumerate([(300, 65), (33, 5), (40, 121)]):
        x, y = ref.multilabel_case(r, c, seed=i) if multilabel else ref.multiclass_case(r, c, 20.0, seed=i)
        got, _ = (ref.multilabel_counts if multilabel else ref.multiclass_counts)(x, y)
        want = [a + b for a, b in zip(want, got)]
        m.update(x if i else x.float(), y)                                                 # (fp32 and bf16 logits)
        assert list(m.counts()) == want
    assert m.compute() == ref.micro_f1(want)
    assert list(m.delta()) == want and m.delta() == (0, 0, 0, 0)
    m.check_errors()
    # (table, ids) with repeats, row_ids over a wider prediction, a device-side row count
    g = torch.Generator().manual_seed(5)
    x, y = ref.multilabel_case(64, 7, seed=9) if multilabel else ref.multiclass_case(64, 7, seed=9)
    ids = torch.randint(0, 64, (50,), generator=g).to(torch.int32)
    m.reset()
    m.update(x, label_table=y, label_ids=ids, row_ids=ids, n_rows_dev=torch.tensor([41], dtype=torch.int32))
    k = ids[:41].long()
    got, _ = (ref.multilabel_counts if multilabel else ref.multiclass_counts)(x[k], y[k])
    assert m.counts() == got
    assert micro_f1_from_counts(got, multilabel) == pytest.approx(ref.micro_f1(got), abs=1e-6)
    with pytest.raises(ValueError):
        m.update(x, y, label_table=y, label_ids=ids)
    with pytest.raises(ValueError):
        m.update(x)


def test_torch_route_flags_labels_out_of_range_and_leaves_the_rows_out():
    from bliss_gnn_amd.metrics import MicroF1
    x, y = ref.multiclass_case(40, 6, seed=3, bad_labels=True)
    want, flagged = ref.multiclass_counts(x, y)
    assert flagged and want[3] == 37
    m = MicroF1()
    m.update(x.float(), y)
    assert m.counts() == want
    with pytest.raises(RuntimeError, match="out of range"):
        m.check_errors()
    m.check_errors()                                                                       # raised once, then cleared
