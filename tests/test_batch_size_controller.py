"""CPU suite: fit.BatchSizeController (the reference's BatchSizeCallback rule, train_lightning.py:425-486, with clamps) on scripted
sequences, and BatchLoader.set_batch_size."""
import math

import pytest
import torch

import batch_stats_ref as ref
from bliss_gnn_amd.fit import BatchSizeController
from bliss_gnn_amd.train import BatchLoader


def _rule(limit, factor, n, m, s):
    return limit > 0 and n >= 2 and abs(limit - m) * n >= math.sqrt(s / (n - 1)) * factor


def test_push_is_the_restated_fold_bit_for_bit():
    c, st = BatchSizeController(1000), ref.BatchStats()
    for x in (117000, 21000, 5, 2 ** 24 + 3, 99999, 0, 12):
        c.push(x)
        st.push(x)
        assert (c.n, c.m, c.s) == (st.n, st.m, st.s)


def test_no_change_below_two_samples_and_without_a_limit():
    c = BatchSizeController(100)
    assert c.propose(64) is None
    c.push(1000)
    assert c.propose(64) is None and c.n == 1            # one sample: no variance yet
    c.push(1000)
    assert c.propose(64) == int(64 * 100 / 1000.0)
    off = BatchSizeController(-1)
    for x in (1000, 1000, 1000):
        off.push(x)
    assert off.propose(64) is None and off.n == 3
    zero = BatchSizeController(0)
    zero.push(5); zero.push(5)
    assert zero.propose(64) is None


def test_scripted_sequence_follows_the_reference_rule():
    xs = [900, 1100, 1000, 950, 1050, 1020, 980]
    c, n, m, s = BatchSizeController(1005, factor=3), 0, 0.0, 0.0
    for x in xs:
        c.push(x)
        n += 1
        m0 = m
        m += (x - m0) / n
        s += (x - m0) * (x - m)
        want = _rule(1005, 3, n, m, s)
        got = BatchSizeController(1005, 3)
        got.load(n, m, s)
        assert (got.propose(256) is not None) == want
    assert (c.n, c.m, c.s) == (n, m, s)


def test_no_change_inside_factor_standard_errors():
    # mean 1000, s = 20000 over n = 5: std = sqrt(5000) ~ 70.7; the rule |limit - m| * n >= std * factor
    c = BatchSizeController(1040, factor=3)
    c.load(5, 1000.0, 20000.0)
    assert abs(1040 - 1000.0) * 5 < math.sqrt(5000.0) * 3
    assert c.propose(128) is None
    assert (c.n, c.m, c.s) == (5, 1000.0, 20000.0)       # kept: the next epoch goes on accumulating
    c.push(1000)
    assert c.n == 6
    far = BatchSizeController(1043, factor=3)
    far.load(5, 1000.0, 20000.0)
    assert abs(1043 - 1000.0) * 5 >= math.sqrt(5000.0) * 3
    assert far.propose(128) == int(128 * 1043 / 1000.0)
    wide = BatchSizeController(1043, factor=4)           # the same record, a wider band
    wide.load(5, 1000.0, 20000.0)
    assert wide.propose(128) is None


def test_new_size_is_truncated_by_int():
    c = BatchSizeController(1000)
    c.load(10, 1500.0, 0.0)
    assert c.propose(100) == 66 == int(100 * 1000 / 1500.0)          # 66.67 -> 66, not 67
    c.load(10, 300.0, 0.0)
    assert c.propose(100, max_size=10 ** 6) == 333


def test_statistics_cleared_only_when_a_change_is_made():
    c = BatchSizeController(500)
    c.load(4, 1000.0, 8.0)
    assert c.propose(64) == 32
    assert (c.n, c.m, c.s) == (0, 0.0, 0.0) and not c.clamped
    assert c.propose(32) is None                          # nothing accumulated since
    c.push(510); c.push(490); c.push(500)
    assert c.propose(32) is None and c.n == 3             # mean on the limit: kept


def test_clamps_at_one_at_the_split_and_at_the_capacity():
    c = BatchSizeController(10)
    c.load(3, 100000.0, 0.0)
    assert c.propose(64, max_size=512) == 1 and c.clamped             # int(0.0064) = 0 -> 1
    c.load(3, 1.0, 0.0)
    split, capacity = 300, 128
    assert c.propose(64, max_size=min(split, capacity)) == 128 and c.clamped
    c.load(3, 1.0, 0.0)
    assert c.propose(64, max_size=min(split, 4096)) == 300 and c.clamped
    c.load(3, 5.0, 0.0)
    assert c.propose(64, max_size=300) == 128 and not c.clamped


def test_loader_batch_size_changes_from_the_next_iteration_only():
    ids = torch.arange(100)
    ld = BatchLoader(ids, 30, shuffle=False, drop_last=True)
    assert len(ld) == 3
    it = iter(ld)
    first = next(it)
    ld.set_batch_size(8)
    assert len(ld) == 3                                    # the pass in progress
    rest = list(it)
    assert [b.numel() for b in [first] + rest] == [30, 30, 30]
    assert torch.equal(rest[-1], ids[60:90])
    got = list(ld)
    assert len(ld) == 12 and len(got) == 12 and all(b.numel() == 8 for b in got)
    assert torch.equal(got[1], ids[8:16])
    ragged = BatchLoader(ids, 30, shuffle=False, drop_last=False)
    ragged.set_batch_size(45)
    assert [b.numel() for b in ragged] == [45, 45, 10] and len(ragged) == 3
    with pytest.raises(ValueError):
        ld.set_batch_size(0)


def test_loader_shuffle_stream_does_not_depend_on_the_batch_size():
    ids = torch.arange(64)
    a, b = BatchLoader(ids, 16, seed=5), BatchLoader(ids, 16, seed=5)
    b.set_batch_size(8)
    assert torch.equal(torch.cat(list(a)), torch.cat(list(b)))
