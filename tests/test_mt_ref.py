"""CPU suite: tests/mt_ref.py (the numpy MT19937 the device generators of csrc/rng.hip are checked against) is torch's CPU
generator, number for number and field for field, from natural states around the 624-word block edge."""
import numpy as np
import pytest
import torch

import mt_ref as R

STARTS = (0, 1, 623, 624, 625, 5000)
N_MAX = 3 * 624 + 17
SEED = 20240


def _entry(start):
    torch.manual_seed(SEED)
    torch.rand(start)
    return R.fields(torch.get_rng_state().numpy())


def _draw_counts(avail):
    ns = {0, 1, 2, 623, 624, 625, 1247, 1248, 1249, 3 * 624, N_MAX}
    for a in (avail, avail + 624, avail + 2 * 624):
        ns.update((a - 1, a, a + 1))
    return sorted(n for n in ns if 0 <= n <= N_MAX)


def test_fields_after_seeding_and_after_one_block():
    torch.manual_seed(SEED)
    _, left, nxt = R.fields(torch.get_rng_state().numpy())
    assert (left, nxt) == (1, 0)                                  # freshly seeded: the first draw regenerates the block
    torch.rand(624)
    _, left, nxt = R.fields(torch.get_rng_state().numpy())
    assert (left, nxt) == (1, 624)                                # a whole block consumed, the next one not made yet


def test_fields_decodes_independently_of_the_engine():
    from bliss_gnn_amd._engine import LayerEngine as Engine
    torch.manual_seed(SEED)
    torch.rand(700)
    st = torch.get_rng_state()
    words, left, nxt = R.fields(st.numpy())
    e_left, e_next, e_words = Engine._rng_fields(st)
    assert left == int(e_left[0]) and nxt == int(e_next[0])
    assert np.array_equal(words, e_words.astype(np.uint32))
    packed = R.pack626(words, left, nxt)
    assert packed.dtype == np.int32 and packed.shape == (626,)
    assert np.array_equal(packed[:624].view(np.uint32), words) and (int(packed[624]), int(packed[625])) == (left, nxt)


@pytest.mark.parametrize("start", STARTS)
def test_numbers_are_torchs(start):
    words, left, nxt = _entry(start)
    avail = R.avail_of(left)
    assert avail == (0 if start == 0 else (-start) % 624)
    blocks = R.raw_blocks(words, R.blocks_for(avail, N_MAX))
    # the unread words of the entry block sit at `next` and run to its end -- except right after seeding (left 1, next 0),
    # when block 0 is the seeded state itself and none of it is handed out
    assert nxt + avail == 624 or (left, nxt) == (1, 0)
    stream = np.concatenate([blocks[0][nxt:nxt + avail], blocks[1:].reshape(-1)])
    assert stream.size >= N_MAX
    got = R.uniform(stream)
    for n in _draw_counts(avail):
        _entry(start)
        want = torch.rand(n).numpy()
        assert np.array_equal(got[:n].view(np.int32), want.view(np.int32)), (start, n)
        assert np.array_equal(R.draws(blocks, left, nxt, n).view(np.int32), want.view(np.int32)), (start, n)


@pytest.mark.parametrize("start", STARTS)
def test_state_after_n_draws_is_torchs(start):
    words, left, nxt = _entry(start)
    avail = R.avail_of(left)
    blocks = R.raw_blocks(words, R.blocks_for(avail, N_MAX))
    for n in _draw_counts(avail):
        _entry(start)
        torch.rand(n)
        t_words, t_left, t_next = R.fields(torch.get_rng_state().numpy())
        if n <= avail:
            want = (blocks[0], left - n, nxt + n)
        else:
            b, t = 1 + (n - avail - 1) // 624, (n - avail - 1) % 624 + 1
            want = (blocks[b], 625 - t, t)
        assert (t_left, t_next) == want[1:], (start, n)
        assert np.array_equal(t_words, want[0]), (start, n)
        got = R.state_after(blocks, left, nxt, n)
        assert got[1:] == want[1:] and np.array_equal(got[0], want[0])


def test_vectorised_recurrence_equals_the_word_by_word_one():
    torch.manual_seed(3)
    od = R.fields(torch.get_rng_state().numpy())[0]
    nw = np.zeros(624, dtype=np.uint32)
    for k in range(624):
        u, v = int(od[k]), int(od[k + 1]) if k < 623 else int(nw[0])
        m = int(od[k + 397]) if k < 227 else int(nw[k - 227])
        y = (u & 0x80000000) | (v & 0x7FFFFFFF)
        nw[k] = m ^ (y >> 1) ^ (0x9908B0DF if v & 1 else 0)
    assert np.array_equal(R._next_block(od), nw)
