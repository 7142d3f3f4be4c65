"""GPU suite (-m gpu): bliss_batch_stats (csrc/ledger.hip) replayed from a graph against the plain-Python
restatement (tests/batch_stats_ref.py), bit for bit; the clear mode; the BLISS_EINVAL cases."""
import numpy as np
import pytest
import torch

import batch_stats_ref as ref

pytestmark = pytest.mark.gpu


def _st():
    return torch.cuda.current_stream().cuda_stream


def _values():
    rng = np.random.default_rng(5)
    xs = np.concatenate([[0, 0, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 1, 117000, 21000],
                         rng.integers(0, 400000, 150), rng.integers(2 ** 24, 2 ** 31 - 1, 42)])
    rng.shuffle(xs)
    assert xs.size == 200 and (xs == 0).any() and (xs > 2 ** 24).any()
    return [int(x) for x in xs]


def test_200_replayed_folds_are_the_restatements_bits(cuda):
    from bliss_gnn_amd import _lib
    L, layer = 3, 2
    counts = torch.zeros(10 * L, dtype=torch.int32, device=cuda)                # three counts records; K is word 3 of each
    rec = torch.zeros(4, dtype=torch.int64, device=cuda)
    push = lambda: _lib.lib.bliss_batch_stats(_lib.BATCH_STATS_PUSH, counts.data_ptr(), layer, rec.data_ptr(), _st())
    xs = _values()
    staged = torch.tensor(xs, dtype=torch.int32, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert push() == 0
    torch.cuda.current_stream().wait_stream(side)
    assert _lib.lib.bliss_batch_stats(_lib.BATCH_STATS_CLEAR, None, 0, rec.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert rec.tolist() == [0, 0, 0, 0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert push() == 0
    want = ref.BatchStats()
    counts[3], counts[13] = 123456, 654321                                      # other layers' K: never read
    for i, x in enumerate(xs):
        counts[10 * layer + 3:10 * layer + 4].copy_(staged[i:i + 1])
        graph.replay()
        want.push(x)
        if i in (0, 1, 2, 57, 199):
            assert bytes(rec.cpu().numpy().tobytes()) == want.to_bytes(), i
    got = _lib.BatchStats.from_buffer_copy(rec.cpu().numpy().tobytes())
    assert (got.n, got.m, got.s, got.reserved) == (200, want.m, want.s, 0)
    assert _lib.lib.bliss_batch_stats(_lib.BATCH_STATS_CLEAR, None, 0, rec.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert rec.tolist() == [0, 0, 0, 0]
    graph.replay()                                                              # and the record starts again
    torch.cuda.synchronize()
    one = ref.BatchStats()
    one.push(xs[-1])
    assert bytes(rec.cpu().numpy().tobytes()) == one.to_bytes()
    del graph


def test_invalid_arguments_are_refused_before_any_launch(cuda):
    from bliss_gnn_amd import _lib
    counts = torch.zeros(10, dtype=torch.int32, device=cuda)
    rec = torch.zeros(4, dtype=torch.int64, device=cuda)
    f = _lib.lib.bliss_batch_stats
    assert f(_lib.BATCH_STATS_PUSH, counts.data_ptr(), 0, None, _st()) == _lib.EINVAL
    assert f(_lib.BATCH_STATS_PUSH, None, 0, rec.data_ptr(), _st()) == _lib.EINVAL
    assert f(_lib.BATCH_STATS_PUSH, counts.data_ptr(), -1, rec.data_ptr(), _st()) == _lib.EINVAL
    assert f(_lib.BATCH_STATS_PUSH, counts.data_ptr(), _lib.LEDGER_MAX_LAYERS, rec.data_ptr(), _st()) == _lib.EINVAL
    assert f(7, counts.data_ptr(), 0, rec.data_ptr(), _st()) == _lib.EINVAL
    assert f(_lib.BATCH_STATS_CLEAR, None, 0, None, _st()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert rec.tolist() == [0, 0, 0, 0]
