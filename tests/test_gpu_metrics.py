"""GPU suite: the micro-F1 kernels (csrc/metrics.hip) behind metrics.MicroF1 against the NumPy restatement of their rule
(tests/metrics_ref.py).  Counts are integers: every comparison is exact equality."""
import functools

import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu


def _trip():
    from bliss_gnn_amd import _lib
    return _lib.F1_MAX_WORKGROUPS * _lib.F1_ROWS_PER_WORKGROUP                  # rows one trip of the single-label row loop takes


SC = [(r, c, s) for (r, c) in ref.MULTICLASS_SHAPES for s in (1.0, 20.0)]
SC_TRIPS = [(4096, 7, 1.0), (4097, 7, 20.0), (9001, 3, 1.0)]                    # cap x rows per workgroup, + 1, > 2 x that


@functools.lru_cache(maxsize=None)
def _sc(r, c, s, bad=False):
    x, y = ref.multiclass_case(r, c, s, seed=1, bad_labels=bad)
    return x, y, ref.multiclass_counts(x, y)


@functools.lru_cache(maxsize=None)
def _ml(r, c, tiny=True):
    x, t = ref.multilabel_case(r, c, seed=1, tiny=tiny)
    return x, t, ref.multilabel_counts(x, t)[0]


def _counts(multilabel, x, *a, **kw):
    from bliss_gnn_amd.metrics import MicroF1
    m = MicroF1(multilabel)
    m.update(x, *a, **kw)
    out = m.counts()
    m.check_errors()
    return out


ML_TRIP_SHAPE = (4200, 125)                                                    # the multi-label loop's third trip (pairs, not rows)


def test_trip_shapes_are_the_kernels_own():
    from bliss_gnn_amd import _lib
    assert _trip() == 4096 and SC_TRIPS[0][0] == _trip() and SC_TRIPS[1][0] == _trip() + 1 and SC_TRIPS[2][0] > 2 * _trip()
    pairs = _lib.F1_MAX_WORKGROUPS * _lib.F1_PAIRS_PER_WORKGROUP
    assert ML_TRIP_SHAPE[0] * ML_TRIP_SHAPE[1] > 2 * pairs


@pytest.mark.parametrize("r,c,s", SC + SC_TRIPS)
def test_single_label_counts_are_the_restatements(cuda, r, c, s):
    from bliss_gnn_amd.fit import micro_f1
    from bliss_gnn_amd.metrics import micro_f1_from_counts
    x, y, (want, flagged) = _sc(r, c, s)
    assert not flagged
    xd, yd = x.to(cuda), y.to(cuda)
    got = _counts(False, xd, yd)
    print(r, c, s, got, want)
    assert got == want
    assert micro_f1_from_counts(got, False, cuda) == micro_f1(xd.float(), yd)   # fit.micro_f1's own float, on its device


def test_single_label_out_of_range_labels_are_flagged_and_left_out(cuda):
    from bliss_gnn_amd.metrics import MicroF1
    for r, c in ((40, 6), (4097, 7)):
        x, y, (want, flagged) = _sc(r, c, 1.0, True)
        assert flagged and want[3] == r - 3 and y[10] == -1 and y[11] == c and y[12] == -100
        m = MicroF1()
        m.update(x.to(cuda), y.to(cuda))
        assert m.counts() == want                                              # bit 2 set; the rows are in no count
        assert int(m._err.item()) == 2
        with pytest.raises(RuntimeError, match="out of range"):
            m.check_errors()
        m.check_errors()                                                       # raised once, then cleared
        assert int(m._err.item()) == 0 and m.counts() == want


@pytest.mark.parametrize("r,c", ref.MULTILABEL_SHAPES + [ML_TRIP_SHAPE])
def test_multi_label_counts_are_the_restatements(cuda, r, c):
    from bliss_gnn_amd.fit import micro_f1
    from bliss_gnn_amd.metrics import micro_f1_from_counts
    x, t, want = _ml(r, c)                                                     # planted 0, -0, NaN, +-inf, 2^-30, targets of 0.5
    got = _counts(True, x.to(cuda), t.to(cuda))
    print(r, c, got, want)
    assert got == want and got[3] == r * c
    # without the planted 2^-30 the draw holds no nonzero |x| < 2^-20: an fp32 sigmoid, wherever its cut sits, agrees with x > 0
    x, t, want = _ml(r, c, False)
    assert ref.smallest_nonzero(x) >= 2.0 ** -20
    got = _counts(True, x.to(cuda), t.to(cuda))
    assert got == want
    assert micro_f1_from_counts(got, True, cuda) == micro_f1(x.to(cuda).float(), t.to(cuda), multilabel=True)


@pytest.mark.parametrize("multilabel", [False, True])
def test_entry_forms(cuda, multilabel):
    counts_of = ref.multilabel_counts if multilabel else ref.multiclass_counts
    g = torch.Generator().manual_seed(3)
    rows, wide_rows, c, wide_c, off, n_count = 700, 1000, 37, 64, 9, 650
    nan = float("nan")
    x, y = (ref.multilabel_case(wide_rows, c, seed=4) if multilabel else ref.multiclass_case(wide_rows, c, 20.0, seed=4))
    wide = torch.full((wide_rows, wide_c), nan).bfloat16()                       # NaN in every column outside the slice
    wide[:, off:off + c] = x
    wd, yd = wide.to(cuda), y.to(cuda)
    sl = wd[:, off:off + c]
    assert sl.stride(0) == wide_c != c and sl.stride(1) == 1
    want = counts_of(x, y)[0]
    assert _counts(multilabel, sl, yd) == want                                  # a column slice: stride != classes
    # (label_table, label_ids) with repeated ids against direct labels
    ids = torch.randint(0, wide_rows, (rows,), generator=g)
    ids[1] = ids[0]
    want = counts_of(x[ids], y[ids])[0]
    i32 = ids.to(torch.int32).to(cuda)
    assert _counts(multilabel, sl[ids.to(cuda)].contiguous(), yd[ids.to(cuda)].contiguous()) == want
    assert _counts(multilabel, sl[ids.to(cuda)].contiguous(), label_table=yd, label_ids=i32) == want
    # row_ids with repeats over the wider prediction, labels direct and through the table
    assert _counts(multilabel, sl, yd[ids.to(cuda)].contiguous(), row_ids=i32) == want
    assert _counts(multilabel, sl, label_table=yd, label_ids=i32, row_ids=i32) == want
    # NaN in every row beyond the counted rows; their ids point outside table and prediction
    pad_ids = i32.clone()
    pad_ids[n_count:] = 2 ** 30
    nd = torch.tensor([n_count], dtype=torch.int32, device=cuda)
    want = counts_of(x[ids[:n_count]], y[ids[:n_count]])[0]
    assert _counts(multilabel, sl, label_table=yd, label_ids=pad_ids, row_ids=pad_ids, n_rows_dev=nd) == want
    xn = sl[ids.to(cuda)].contiguous()
    xn[n_count:] = nan
    assert _counts(multilabel, xn, label_table=yd, label_ids=pad_ids, n_rows_dev=nd) == want


@pytest.mark.parametrize("multilabel", [False, True])
def test_device_side_row_count(cuda, multilabel):
    counts_of = ref.multilabel_counts if multilabel else ref.multiclass_counts
    cap = _trip()
    rows, c = cap + 2, 5
    x, y = ref.multilabel_case(rows, c, seed=6) if multilabel else ref.multiclass_case(rows, c, seed=6)
    ids = torch.randperm(rows, generator=torch.Generator().manual_seed(8))
    xs, table = x[ids], y.to(cuda)
    for v in (0, 1, cap - 1, cap, cap + 5, -3):
        n = min(max(v, 0), rows)
        want = counts_of(xs, y[ids], v)[0]
        assert want[3] == n * (c if multilabel else 1)
        xd, idd = xs.to(cuda).clone(), ids.to(torch.int32).to(cuda)
        xd[n:] = float("nan")                                                  # NaN padding rows, padding ids outside the table
        idd[n:] = 2 ** 30
        nd = torch.tensor([v], dtype=torch.int32, device=cuda)
        assert _counts(multilabel, xd, label_table=table, label_ids=idd, n_rows_dev=nd) == want, v


@pytest.mark.parametrize("multilabel", [False, True])
def test_forty_launches_accumulate_and_two_runs_are_bit_equal(cuda, multilabel):
    from bliss_gnn_amd.metrics import MicroF1
    counts_of = ref.multilabel_counts if multilabel else ref.multiclass_counts
    cases = []
    for i, r in enumerate((1, 5, 4097, 256, 9001)):
        x, y = ref.multilabel_case(r, 5, seed=20 + i) if multilabel else ref.multiclass_case(r, 5, seed=20 + i)
        cases.append((x.to(cuda), y.to(cuda), counts_of(x, y)[0]))
    runs = []
    for _ in range(2):
        m, total, seen = MicroF1(multilabel), [0, 0, 0, 0], []
        for k in range(40):
            xd, yd, c = cases[k % 5]
            m.update(xd, yd)
            total = [a + b for a, b in zip(total, c)]
            assert list(m.counts()) == total, k                                # added to, never overwritten
            assert m.delta() == c
            seen.append(m.counts())
        assert m.compute() == ref.micro_f1(total)
        runs.append(seen)
        m.reset()
        assert m.counts() == (0, 0, 0, 0)
    assert runs[0] == runs[1]


@pytest.mark.parametrize("multilabel", [False, True])
def test_captured_update_replays_over_changing_inputs(cuda, multilabel):
    from bliss_gnn_amd.metrics import MicroF1
    counts_of = ref.multilabel_counts if multilabel else ref.multiclass_counts
    r, c = 4097, 7
    batches = [ref.multilabel_case(r, c, seed=30 + i) if multilabel else ref.multiclass_case(r, c, seed=30 + i) for i in range(3)]
    xb, yb = batches[0][0].to(cuda).clone(), batches[0][1].to(cuda).clone()
    m, eager = MicroF1(multilabel), MicroF1(multilabel)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(xb, yb)                                                       # (warm-up: the state exists before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(xb, yb)
    assert m.counts() == (0, 0, 0, 0)                                          # the capture executed nothing
    total = [0, 0, 0, 0]
    for x, y in batches:
        xb.copy_(x.to(cuda)); yb.copy_(y.to(cuda))
        graph.replay()
        eager.update(x.to(cuda), y.to(cuda))
        total = [a + b for a, b in zip(total, counts_of(x, y)[0])]
        assert list(m.counts()) == total == list(eager.counts())
    m.check_errors()


@pytest.mark.parametrize("multilabel", [False, True])
def test_fp32_logits_take_the_torch_route_with_the_kernels_counts(cuda, multilabel):
    from bliss_gnn_amd.metrics import MicroF1
    for r, c in ((300, 65), (4097, 5)):
        x, y = _ml(r, c)[:2] if multilabel else _sc(r, c, 20.0, True)[:2]             # (single-label: with labels out of range)
        xd, yd = x.to(cuda), y.to(cuda)
        k, t = MicroF1(multilabel), MicroF1(multilabel)
        assert k._eligible(xd, yd, None, None, None, None) and not t._eligible(xd.float(), yd, None, None, None, None)
        k.update(xd, yd)
        t.update(xd.float(), yd)
        assert k.counts() == t.counts() and int(k._err.item()) == int(t._err.item()) == (0 if multilabel else 2)
        ids = torch.randint(0, r, (r + 10,), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(cuda)
        nd = torch.tensor([r - 7], dtype=torch.int32, device=cuda)
        k.reset(); t.reset()
        k.update(xd, label_table=yd, label_ids=ids, row_ids=ids, n_rows_dev=nd)
        t.update(xd.float(), label_table=yd, label_ids=ids, row_ids=ids, n_rows_dev=nd)
        assert k.counts() == t.counts()
