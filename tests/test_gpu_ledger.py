"""GPU suite (-m gpu): the step-ledger kernel (csrc/ledger.hip) against its restatement (tests/ledger_ref.py), launched kernel by
kernel and replayed from captured graphs: the record equals the restatement word for word after every step."""
import ctypes as C

import numpy as np
import pytest
import torch

import ledger_ref as ref

pytestmark = pytest.mark.gpu


def _fresh(L, cuda):
    from bliss_gnn_amd import _lib
    return torch.frombuffer(bytearray(bytes(_lib.ledger_new(L))), dtype=torch.int64).to(cuda)


@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("L", [1, 3, 8])
def test_the_record_is_the_restatement_word_for_word(cuda, L, graphed):
    """40 planted steps: sizes exactly at, one below and one above regrow_at * cap, an err bit on step 17, a NaN and an inf loss,
    bf16 and fp32 losses in turn; then the epoch reset, the re-arm and one more step."""
    from bliss_gnn_amd import _lib
    caps, steps = ref.planted_steps(L)
    want = ref.Ledger(L)
    led, counts = _fresh(L, cuda), torch.zeros(L * 10, dtype=torch.int32, device=cuda)
    loss = {ref.BF16: torch.zeros(1, dtype=torch.int16, device=cuda), ref.F32: torch.zeros(1, dtype=torch.int32, device=cuda)}
    caps_c = (C.c_int32 * (3 * L))(*[int(v) for v in caps.reshape(-1)])

    def launch(dtype, target, mode=_lib.LEDGER_STEP):
        _lib.check(_lib.lib.bliss_step_ledger(mode, loss[dtype].data_ptr(), dtype, counts.data_ptr(), L, caps_c, 0.99, 0.85,
                                              target.data_ptr(), torch.cuda.current_stream().cuda_stream), "bliss_step_ledger")

    graphs = {}
    if graphed:
        scratch = _fresh(L, cuda)
        for dtype in (ref.BF16, ref.F32):                                         # (the first launch loads the kernel: not in a capture)
            launch(dtype, scratch)
        torch.cuda.synchronize()
        for dtype in (ref.BF16, ref.F32):
            graphs[dtype] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[dtype]):
                launch(dtype, led)
        assert np.array_equal(led.cpu().numpy().view(np.uint64), want.words())    # the captures executed nothing

    def one(bits, dtype, c):
        counts.copy_(torch.from_numpy(c.reshape(-1)))
        loss[dtype].fill_(bits - (1 << 16 if dtype == ref.BF16 and bits >= 1 << 15 else 0) - (1 << 32 if dtype == ref.F32 and bits >= 1 << 31 else 0))
        if graphed:
            graphs[dtype].replay()
        else:
            launch(dtype, led)
        want.step(bits, dtype, c, caps, 0.99, 0.85)

    for t, (bits, dtype, c) in enumerate(steps):
        one(bits, dtype, c)
        got = led.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want.words()), (t, _lib.ledger_dict(_lib.ledger_struct(L).from_buffer_copy(got.tobytes())), want.as_dict())
    assert want.first_bad_step == 17 and want.first_near_step == 29 and want.nonfinite == 2
    launch(ref.F32, led, _lib.LEDGER_RESET_EPOCH)
    want.reset_epoch()
    assert np.array_equal(led.cpu().numpy().view(np.uint64), want.words())
    launch(ref.F32, led, _lib.LEDGER_REARM)
    want.rearm()
    assert np.array_equal(led.cpu().numpy().view(np.uint64), want.words())
    one(*steps[3])
    assert np.array_equal(led.cpu().numpy().view(np.uint64), want.words())
    assert want.steps_epoch == 1 and want.steps_total == 41
