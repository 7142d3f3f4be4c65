"""CPU suite: the step ledger's entry points (csrc/ledger.hip) are exported and bound, refuse bad arguments on the host (a
refused call launches nothing, so this runs without a GPU), and the ctypes mirror of the record has the library's size."""
import ctypes as C

import pytest

import ledger_ref as ref

NAMES = ("bliss_step_ledger", "bliss_step_ledger_bytes")


def test_symbols_are_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from bliss_gnn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in _lib.SIGNATURES and getattr(_lib.lib, n).argtypes is not None
    assert len(_lib.SIGNATURES["bliss_step_ledger"]) == 10
    hdr = open(__graft_entry__.ROOT + "/include/bliss_gnn.h").read()
    assert "#define BLISS_LEDGER_MAX_LAYERS %d" % _lib.LEDGER_MAX_LAYERS in hdr
    for name, v in (("STEP", _lib.LEDGER_STEP), ("RESET_EPOCH", _lib.LEDGER_RESET_EPOCH), ("REARM", _lib.LEDGER_REARM),
                    ("LOSS_BF16", _lib.LEDGER_LOSS_BF16), ("LOSS_F32", _lib.LEDGER_LOSS_F32)):
        assert "#define BLISS_LEDGER_%s %d" % (name, v) in hdr
    assert (ref.STEP, ref.RESET_EPOCH, ref.REARM, ref.BF16, ref.F32) == (_lib.LEDGER_STEP, _lib.LEDGER_RESET_EPOCH, _lib.LEDGER_REARM,
                                                                         _lib.LEDGER_LOSS_BF16, _lib.LEDGER_LOSS_F32)


@pytest.mark.parametrize("L", range(1, 9))
def test_the_ctypes_record_has_the_librarys_size_and_the_restatements_layout(L):
    from bliss_gnn_amd import _lib
    S = _lib.ledger_struct(L)
    assert C.sizeof(S) == _lib.lib.bliss_step_ledger_bytes(L) == ref.ledger_bytes(L) and C.sizeof(S) % 8 == 0
    assert (S.loss_last.offset, S.cum_out.offset, S.first_bad_step.offset, S.err.offset, S.cum_nodes.offset) == (16, 40, 48, 64, 80)
    assert (S.cum_edges.offset, S.hw_K.offset, S.hw_E.offset) == (80 + 8 * L, 80 + 16 * L, 80 + 24 * L)
    fresh = _lib.ledger_new(L)
    assert bytes(fresh) == ref.Ledger(L).to_bytes()
    d = _lib.ledger_dict(fresh)
    assert d == ref.Ledger(L).as_dict()


def test_bad_arguments_are_refused_before_any_launch():
    from bliss_gnn_amd import _lib
    fn, E = _lib.lib.bliss_step_ledger, _lib.EINVAL
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    caps = (C.c_int32 * 24)()
    # (mode, loss, loss_dtype, counts, n_layers, caps, w, regrow_at, ledger, stream)
    good = [_lib.LEDGER_STEP, p, _lib.LEDGER_LOSS_F32, p, 3, caps, 0.99, 0.85, p, 0]
    for i in (1, 3, 5, 8):                                                       # null loss, counts, caps, ledger
        a = list(good); a[i] = None
        assert fn(*a) == E, i
    for L in (0, -1, 9, 100):
        a = list(good); a[4] = L
        assert fn(*a) == E, L
        assert _lib.lib.bliss_step_ledger_bytes(L) == E
    for code in (-1, 2, 7):
        a = list(good); a[2] = code
        assert fn(*a) == E, code
    for mode in (-1, 3):
        a = list(good); a[0] = mode
        assert fn(*a) == E, mode
    for mode in (_lib.LEDGER_RESET_EPOCH, _lib.LEDGER_REARM):                    # the modes that read only the ledger still need one
        assert fn(mode, None, 0, None, 3, None, 0.0, 0.0, None, 0) == E
        assert fn(mode, None, 0, None, 0, None, 0.0, 0.0, p, 0) == E
    with pytest.raises(ValueError):
        _lib.ledger_struct(9)
