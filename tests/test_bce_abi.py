"""CPU suite: the multi-label loss (csrc/loss.hip: k_bce_logits) is exported, bound and validates its arguments on the host
(a refused call launches nothing, so this runs without a GPU); nn.BCEWithLogitsLoss falls back to torch's functional form for
what the kernel does not take; BLISS_FUSED_BCE=0 restores torch's module in the train loops."""
import ctypes as C

import torch

NAMES = ("bliss_bce_logits", "bliss_bce_logits_sum", "bliss_bce_logits_masked")


def test_symbols_are_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _lib.SIGNATURES
        assert getattr(_lib.lib, n).argtypes is not None
    assert len(_lib.SIGNATURES["bliss_bce_logits"]) == 12
    assert len(_lib.SIGNATURES["bliss_bce_logits_sum"]) == 15
    assert len(_lib.SIGNATURES["bliss_bce_logits_masked"]) == 19


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from bliss_gnn_amd import _lib
    lib, E = _lib.lib, _lib.EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    # bliss_bce_logits(logits, stride, targets, n_rows, n_cls, row_loss, dlogits, d_stride, loss_out, ticket, err, stream)
    good = [p, 8, p, 4, 3, p, p, 8, p, p, p, 0]
    for i in (0, 2, 5, 6, 8, 9, 10):                                                       # every pointer, null in turn
        a = list(good); a[i] = 0
        assert lib.bliss_bce_logits(*a) == E, i
    for i, v in ((3, 0), (3, -1), (4, 0), (4, -5)):                                        # n_rows <= 0, n_cls <= 0
        a = list(good); a[i] = v
        assert lib.bliss_bce_logits(*a) == E, (i, v)
    # bliss_bce_logits_sum(logits, stride, logits2, stride2, table, label_ids, n_rows, n_cls, row_loss, dlogits, d_stride, loss_out,
    #                      ticket, err, stream)
    good = [p, 8, p, 8, p, p, 4, 3, p, p, 8, p, p, p, 0]
    a = list(good); a[2] = 0; a[5] = 0
    assert lib.bliss_bce_logits_sum(*a) == E                                               # neither option given
    for i in (0, 4, 8, 9, 11, 12, 13):
        a = list(good); a[i] = 0
        assert lib.bliss_bce_logits_sum(*a) == E, i
    for i in (6, 7):
        a = list(good); a[i] = 0
        assert lib.bliss_bce_logits_sum(*a) == E, i
    # bliss_bce_logits_masked(logits, stride, logits2, stride2, table, n_table, label_ids, id_off, n_rows, n_rows_dev, denom, n_cls,
    #                         row_loss, dlogits, d_stride, loss_out, ticket, err, stream)
    good = [p, 8, 0, 0, p, 4, p, 0, 4, p, 12.0, 3, p, p, 8, p, p, p, 0]
    for i in (0, 4, 6, 9, 12, 13, 15, 16, 17):                                             # (6: no label ids, 9: no device-side count)
        a = list(good); a[i] = 0
        assert lib.bliss_bce_logits_masked(*a) == E, i
    for i, v in ((10, 0.0), (10, -1.0), (10, float("nan")), (8, 0), (11, 0), (5, 0)):      # denom, n_rows, n_cls, n_table
        a = list(good); a[i] = v
        assert lib.bliss_bce_logits_masked(*a) == E, (i, v)


def test_module_on_cpu_is_torchs_functional_form():
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(37, 11, generator=gen) * 3).requires_grad_(True)
    y = (torch.rand(37, 11, generator=gen) < 0.1).float()
    xr = x.detach().clone().requires_grad_(True)
    lf = BCEWithLogitsLoss()
    loss = lf(x, y)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(xr, y)
    assert loss.dtype == ref.dtype and torch.equal(loss, ref)
    loss.backward(); ref.backward()
    assert torch.equal(x.grad, xr.grad)
    with torch.no_grad():
        assert torch.equal(lf(x, y), ref.detach())
    # the routes the train loops call take the same fallback
    x2 = x.detach().clone().requires_grad_(True)
    assert torch.equal(lf.backward_from(x2, y), ref.detach()) and torch.equal(x2.grad, xr.grad)
    a = x.detach().clone().requires_grad_(True)
    b = torch.zeros_like(a).requires_grad_(True)
    table = (torch.rand(90, 11, generator=gen) < 0.1).float()
    ids = torch.randperm(90, generator=gen)[:37].to(torch.int32)
    xs = x.detach().clone().requires_grad_(True)
    want = torch.nn.functional.binary_cross_entropy_with_logits(xs, table[ids.long()])
    want.backward()
    got = lf.backward_from_parts(a, b, table, ids)
    assert torch.equal(got, want.detach()) and torch.equal(a.grad, xs.grad) and torch.equal(b.grad, xs.grad)
    # bf16 logits with bf16 targets on the CPU: torch's route and torch's dtype
    xb, yb = x.detach().bfloat16(), y.bfloat16()
    assert torch.equal(lf(xb, yb), torch.nn.functional.binary_cross_entropy_with_logits(xb, yb))


def test_switch_restores_torchs_module(monkeypatch):
    from bliss_gnn_amd import train
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    monkeypatch.delenv("BLISS_FUSED_BCE", raising=False)
    assert type(train._bce_loss()) is BCEWithLogitsLoss
    monkeypatch.setenv("BLISS_FUSED_BCE", "0")
    assert type(train._bce_loss()) is torch.nn.BCEWithLogitsLoss
    monkeypatch.setenv("BLISS_FUSED_BCE", "1")
    assert type(train._bce_loss()) is BCEWithLogitsLoss
