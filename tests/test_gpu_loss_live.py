"""GPU suite (-m gpu): bliss_cross_entropy_live / bliss_bce_logits_live (csrc/loss.hip) against the _sum entry
points called with n_rows = the live count -- bit for bit --, with rows past the live count planted with NaN logits and
out-of-range label ids, at n = 0, captured and replayed with the word changed in between, and their BLISS_EINVAL cases."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 64
CASES = [("ce", 3), ("ce", 47), ("bce", 1), ("bce", 3), ("bce", 47)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _problem(cuda, kind, n_cls, seed=0):
    """Two bf16 addends [CAP, n_cls], a label table of 200 rows and int32 ids into it."""
    gen = torch.Generator().manual_seed(100 * n_cls + seed)
    a = (torch.randn(CAP, n_cls, generator=gen) * 3).bfloat16().to(cuda)
    b = torch.randn(CAP, n_cls, generator=gen).bfloat16().to(cuda)
    ids = torch.randint(0, 200, (CAP,), generator=gen).to(torch.int32).to(cuda)
    if kind == "ce":
        table = torch.randint(0, n_cls, (200,), generator=gen).to(cuda)
    else:
        table = (torch.rand(200, n_cls, generator=gen) > 0.5).float().to(cuda)
    return a, b, table, ids


def _out(cuda, n_cls, rows=CAP):
    return dict(dx=torch.full((rows, n_cls), 7.0, dtype=torch.bfloat16, device=cuda), rows=torch.empty(rows, dtype=torch.float32, device=cuda),
                loss=torch.full((), -3.0, dtype=torch.float32, device=cuda), state=torch.zeros(2, dtype=torch.int32, device=cuda))


def _sum(kind, a, b, table, ids, n, o):
    from bliss_gnn_amd import _lib
    fn = _lib.lib.bliss_cross_entropy_sum if kind == "ce" else _lib.lib.bliss_bce_logits_sum
    return fn(a.data_ptr(), a.stride(0), 0 if b is None else b.data_ptr(), 0 if b is None else b.stride(0), table.data_ptr(),
              0 if ids is None else ids.data_ptr(), n, a.shape[1], o["rows"].data_ptr(), o["dx"].data_ptr(), o["dx"].stride(0),
              o["loss"].data_ptr(), o["state"].data_ptr(), o["state"].data_ptr() + 4, _st())


def _live(kind, a, b, table, ids, word, o, cap=CAP):
    from bliss_gnn_amd import _lib
    fn = _lib.lib.bliss_cross_entropy_live if kind == "ce" else _lib.lib.bliss_bce_logits_live
    return fn(a.data_ptr(), a.stride(0), 0 if b is None else b.data_ptr(), 0 if b is None else b.stride(0), table.data_ptr(),
              0 if ids is None else ids.data_ptr(), cap, 0 if word is None else word.data_ptr(), a.shape[1], o["rows"].data_ptr(),
              o["dx"].data_ptr(), o["dx"].stride(0), o["loss"].data_ptr(), o["state"].data_ptr(), o["state"].data_ptr() + 4, _st())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plant(a, b, ids, n):
    """Rows >= n: NaN logits in both addends and label ids far outside the table."""
    a, b, ids = a.clone(), b.clone(), ids.clone()
    a[n:], b[n:] = float("nan"), float("nan")
    ids[n:] = 2 ** 30
    return a, b, ids


@pytest.mark.parametrize("kind,n_cls", CASES)
@pytest.mark.parametrize("addend", [True, False])
def test_live_rows_are_the_sum_entry_points_bits(cuda, kind, n_cls, addend):
    a, b, table, ids = _problem(cuda, kind, n_cls)
    word = torch.zeros(1, dtype=torch.int32, device=cuda)
    for n in (1, 37, 64):
        want = _out(cuda, n_cls, n)
        assert _sum(kind, a[:n], b[:n] if addend else None, table, ids[:n], n, want) == 0
        pa, pb, pids = _plant(a, b, ids, n)
        got = _out(cuda, n_cls)
        word.fill_(n)
        assert _live(kind, pa, pb if addend else None, table, pids, word, got) == 0
        torch.cuda.synchronize()
        assert torch.equal(got["loss"], want["loss"]) and bool(torch.isfinite(got["loss"])), (n, got["loss"], want["loss"])
        assert torch.equal(_bits(got["dx"][:n]), _bits(want["dx"])), n
        assert bool((_bits(got["dx"][n:]) == 0).all()), n                      # exactly zero (+0), whatever the rows hold
        assert got["state"].tolist() == [0, 0] and want["state"].tolist() == [0, 0]
    # a word above the capacity is the capacity; a negative one is 0
    full = _out(cuda, n_cls)
    _sum(kind, a, b if addend else None, table, ids, CAP, full)
    got = _out(cuda, n_cls)
    word.fill_(CAP + 9)
    assert _live(kind, a, b if addend else None, table, ids, word, got) == 0
    assert torch.equal(got["loss"], full["loss"]) and torch.equal(_bits(got["dx"]), _bits(full["dx"]))
    word.fill_(-5)
    assert _live(kind, a, b if addend else None, table, ids, word, got) == 0
    assert float(got["loss"]) == 0.0 and bool((_bits(got["dx"]) == 0).all())


@pytest.mark.parametrize("kind,n_cls", CASES)
def test_no_live_row_gives_zero_loss_and_gradients(cuda, kind, n_cls):
    a, b, table, ids = _problem(cuda, kind, n_cls)
    pa, pb, pids = _plant(a, b, ids, 0)
    got = _out(cuda, n_cls)
    word = torch.zeros(1, dtype=torch.int32, device=cuda)
    assert _live(kind, pa, pb, table, pids, word, got) == 0
    torch.cuda.synchronize()
    assert float(got["loss"]) == 0.0 and bool((_bits(got["dx"]) == 0).all())
    assert not bool(torch.isnan(got["dx"].float()).any()) and got["state"].tolist() == [0, 0]


@pytest.mark.parametrize("kind,n_cls", [("ce", 47), ("bce", 3)])
def test_label_errors_are_those_of_the_sum_entry_points(cuda, kind, n_cls):
    """A class index outside [0, n_cls) in a LIVE row sets the same bit and gives the same bits as the _sum call (cross-entropy; the
    BCE _sum entry point checks no table bound, so it has no such case); one in a row past the live count is never seen."""
    a, b, table, ids = _problem(cuda, kind, n_cls)
    word = torch.full((1,), 37, dtype=torch.int32, device=cuda)
    if kind == "ce":
        table = table.clone()
        table[int(ids[5])] = n_cls + 3
        want, got = _out(cuda, n_cls, 37), _out(cuda, n_cls)
        _sum(kind, a[:37], b[:37], table, ids[:37], 37, want)
        _live(kind, a, b, table, ids, word, got)
        torch.cuda.synchronize()
        assert want["state"].tolist() == [0, 2] and got["state"].tolist() == [0, 2]
        assert torch.equal(got["loss"], want["loss"]) and torch.equal(_bits(got["dx"][:37]), _bits(want["dx"]))
        table[int(ids[5])] = 0
        live_ids = set(ids[:37].tolist())
        late = next(r for r in range(37, CAP) if int(ids[r]) not in live_ids)
        table[int(ids[late])] = -1                                              # only a row past the live count points at it
    got = _out(cuda, n_cls)
    _live(kind, a, b, table, ids, word, got)
    torch.cuda.synchronize()
    assert got["state"].tolist() == [0, 0]


@pytest.mark.parametrize("kind,n_cls", [("ce", 47), ("bce", 3)])
def test_one_captured_launch_serves_every_count(cuda, kind, n_cls):
    a, b, table, ids = _problem(cuda, kind, n_cls, seed=1)
    word = torch.full((1,), CAP, dtype=torch.int32, device=cuda)
    got = _out(cuda, n_cls)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _live(kind, a, b, table, ids, word, got) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _live(kind, a, b, table, ids, word, got) == 0
    for n in (37, 1, 64, 0, 37):
        word.fill_(n)
        got["dx"].fill_(5.0)
        graph.replay()
        fresh = _out(cuda, n_cls)
        assert _live(kind, a, b, table, ids, word, fresh) == 0
        torch.cuda.synchronize()
        assert torch.equal(got["loss"], fresh["loss"]) and torch.equal(_bits(got["dx"]), _bits(fresh["dx"])), n
        assert got["state"].tolist() == [0, 0]
        if n:
            want = _out(cuda, n_cls, n)
            _sum(kind, a[:n], b[:n], table, ids[:n], n, want)
            assert torch.equal(got["loss"], want["loss"]) and torch.equal(_bits(got["dx"][:n]), _bits(want["dx"]))
    del graph


@pytest.mark.parametrize("kind,n_cls", [("ce", 3), ("bce", 3)])
def test_invalid_arguments_are_refused_before_any_launch(cuda, kind, n_cls):
    from bliss_gnn_amd import _lib
    a, b, table, ids = _problem(cuda, kind, n_cls)
    word = torch.full((1,), 5, dtype=torch.int32, device=cuda)
    o = _out(cuda, n_cls)
    before = (o["dx"].clone(), o["loss"].clone())
    assert _live(kind, a, b, table, ids, None, o) == _lib.EINVAL               # no device word
    assert _live(kind, a, None, table, None, word, o) == _lib.EINVAL           # neither a second addend nor label ids (as _sum)
    assert _sum(kind, a, None, table, None, CAP, o) == _lib.EINVAL
    assert _live(kind, a, b, table, ids, word, o, cap=0) == _lib.EINVAL        # n_rows <= 0
    fn = _lib.lib.bliss_cross_entropy_live if kind == "ce" else _lib.lib.bliss_bce_logits_live
    args = [a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), table.data_ptr(), ids.data_ptr(), CAP, word.data_ptr(), n_cls,
            o["rows"].data_ptr(), o["dx"].data_ptr(), o["dx"].stride(0), o["loss"].data_ptr(), o["state"].data_ptr(),
            o["state"].data_ptr() + 4, _st()]
    for i in (0, 4, 9, 10, 12, 13, 14):                                         # logits, table, row_loss, dlogits, loss_out, ticket, err
        bad = list(args)
        bad[i] = 0
        assert fn(*bad) == _lib.EINVAL, i
    bad = list(args)
    bad[8] = 0                                                                  # n_cls <= 0
    assert fn(*bad) == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(o["dx"], before[0]) and torch.equal(o["loss"], before[1])


def test_modules_take_the_live_word(cuda):
    """nn.CrossEntropyLoss / nn.BCEWithLogitsLoss: forward, backward_from and backward_from_parts with n_rows_dev against the same
    calls on the first n rows; inputs the kernel does not take raise instead of falling back."""
    from bliss_gnn_amd.nn import BCEWithLogitsLoss, CrossEntropyLoss
    n = 37
    word = torch.full((1,), n, dtype=torch.int32, device=cuda)
    for kind, lf in (("ce", CrossEntropyLoss()), ("bce", BCEWithLogitsLoss())):
        a, b, table, ids = _problem(cuda, kind, 5)
        y = table[ids.long()]
        x = (a + b).detach()
        with torch.no_grad():
            assert torch.equal(lf(x, y, n_rows_dev=word), lf(x[:n], y[:n]))
        x1, x2 = x.clone().requires_grad_(), x[:n].clone().requires_grad_()
        l1, l2 = lf.backward_from(x1, y, n_rows_dev=word), lf.backward_from(x2, y[:n])
        assert torch.equal(l1, l2) and torch.equal(_bits(x1.grad[:n]), _bits(x2.grad)) and bool((_bits(x1.grad[n:]) == 0).all())
        a1, b1, a2, b2 = (t.clone().requires_grad_() for t in (a, b, a[:n], b[:n]))
        l1, l2 = lf.backward_from_parts(a1, b1, table, ids, n_rows_dev=word), lf.backward_from_parts(a2, b2, table, ids[:n].contiguous())
        assert torch.equal(l1, l2) and torch.equal(_bits(a1.grad[:n]), _bits(a2.grad)) and torch.equal(_bits(b1.grad), _bits(a1.grad))
        lf.check_errors()
        with pytest.raises(NotImplementedError):
            lf(x.float(), y, n_rows_dev=word)
        with pytest.raises(ValueError):
            lf(x, y, n_rows_dev=word.long())
