"""The device MT19937 generators (csrc/rng.hip) word for word against torch's CPU generator, through the C ABI alone and in the
order the engine uses it (upload, prepare, begin, one wait per layer, end).  Every comparison is an equality of bits or of
ints.  The authority: torch.manual_seed(SEED); torch.rand(start) fixes a natural state, torch.rand(n) from there are the
expected numbers, torch.get_rng_state() after it the expected state; tests/mt_ref.py (pinned by test_mt_ref.py) supplies the
raw blocks.

  a  whole stream, every word, every raw block     test_whole_stream_*
  b  where the consumption ends                     test_stop_*
  c  serial kernel == head + jumps + stretches      test_serial_generator_*
  d  a stream that runs short (bit 128)             test_stream_that_runs_short
  e  generator handed over on the device            test_chain_*
  f  the one-shot kernel                            test_one_shot_*

bliss_rng_prepare keeps its plans for the life of the process, keyed by capacity: 29953, 175000 and 400000 are only ever
prepared without BLISS_RNG_SERIAL (here and nowhere else in the suite), 175003 only with it, and 175005, 4000, 4001, 1000
and 1001 are never prepared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mt_ref as R

pytestmark = pytest.mark.gpu

SEED = 4357
SENT = 0x5A5AA5A5                      # what the words behind the documented sizes hold; as a float 1.5388e16, never a uniform
TAIL = 1248
I32 = torch.int32
STARTS = (0, 1, 623, 624, 625)
N_STREAM = 400000 + 2 * 624            # the longest stream any case reads
PARALLEL = {29953: (33, 6, 3, 51), 175000: (33, 8, 32, 289), 400000: (33, 20, 32, 673)}


def _L():
    from bliss_gnn_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# the authority (computed once per start, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _entry(start):
    """(words, left, next, avail, numbers int32[N_STREAM], raw blocks) of the state `start` draws after seeding."""
    torch.manual_seed(SEED)
    torch.rand(start)
    words, left, nxt = R.fields(torch.get_rng_state().numpy())
    numbers = torch.rand(N_STREAM).numpy().view(np.int32)
    avail = R.avail_of(left)
    blocks = R.raw_blocks(words, R.blocks_for(avail, N_STREAM))
    for a in (words, numbers, blocks):
        a.setflags(write=False)
    return words, left, nxt, avail, numbers, blocks


def _torch_state_after(start, n):
    torch.manual_seed(SEED)
    torch.rand(start)
    torch.rand(n)
    return R.fields(torch.get_rng_state().numpy())


def _same_state(got626, want):
    words, left, nxt = want
    g = got626.cpu().numpy()
    assert (int(g[624]), int(g[625])) == (left, nxt)
    assert np.array_equal(g[:624].view(np.uint32), words)


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
class _Gen:
    """One generator's buffers at the documented sizes plus TAIL sentinel words, and the ABI calls on them."""

    def __init__(self, dev, cap, prepare, n_layers):
        lib = _L()
        self.cap, self.plan = cap, None
        if prepare:
            plan = (C.c_int32 * 4)()
            lib.check(lib.lib.bliss_rng_prepare(cap, plan), "bliss_rng_prepare")
            self.plan = tuple(plan)
            self.n_out = self.n_raw = 624 * (max(self.plan[3], cap // 624 + 1) + 2)
        else:
            self.n_out, self.n_raw = cap + 1248, 624 * (cap // 624 + 3)
        self.out = torch.full((self.n_out + TAIL,), SENT, dtype=I32, device=dev)
        self.raw = torch.full((self.n_raw + TAIL,), SENT, dtype=I32, device=dev)
        assert self.out.data_ptr() % 16 == 0 and self.raw.data_ptr() % 16 == 0
        self.ctl = torch.zeros(8 + n_layers, dtype=I32, device=dev)
        self.state = torch.zeros(626, dtype=I32, device=dev)
        self.err = torch.zeros(1, dtype=I32, device=dev)
        self.dev, self.keep, self.waits = dev, [], 0

    def upload(self, start):
        words, left, nxt = _entry(start)[:3]
        self.state.copy_(torch.from_numpy(R.pack626(words, left, nxt)))

    def begin(self):
        lib = _L()
        lib.check(lib.lib.bliss_rng_stream_begin(self.state.data_ptr(), self.ctl.data_ptr(), self.out.data_ptr(), self.raw.data_ptr(),
                                                 self.cap, _st()), "bliss_rng_stream_begin")

    def wait(self, count, is_last, counts=None):
        lib = _L()
        if counts is None:
            h = torch.zeros(10, dtype=I32)
            h[2] = count
            counts = h.to(self.dev)
        self.keep.append(counts)
        lib.check(lib.lib.bliss_rng_stream_wait(self.ctl.data_ptr(), counts.data_ptr(), self.ctl.data_ptr() + 4 * (8 + self.waits),
                                                int(is_last), self.cap, _st()), "bliss_rng_stream_wait")
        self.waits += 1

    def consume(self, layers):
        for l, c in enumerate(layers):
            self.wait(c, l == len(layers) - 1)

    def chain(self, counts_dev, counts_host):
        lib = _L()
        lib.check(lib.lib.bliss_rng_stream_chain(self.state.data_ptr(), self.ctl.data_ptr(), self.out.data_ptr(), self.raw.data_ptr(),
                                                 self.cap, counts_dev.data_ptr(), counts_dev.numel(), counts_host.data_ptr(), _st()),
                  "bliss_rng_stream_chain")

    def end(self):
        lib = _L()
        lib.check(lib.lib.bliss_rng_stream_end(self.state.data_ptr(), self.ctl.data_ptr(), self.raw.data_ptr(), self.cap,
                                               self.err.data_ptr(), _st()), "bliss_rng_stream_end")
        torch.cuda.synchronize()

    def run(self, start, layers):
        self.upload(start)
        self.begin()
        self.consume(layers)
        self.end()
        return self

    def tails_intact(self):
        return bool((self.out[self.n_out:] == SENT).all()) and bool((self.raw[self.n_raw:] == SENT).all())

    def numbers(self, first, n):
        return self.out[first:first + n].cpu().numpy()


def _check_consumed(g, start, layers, first_pos=0, first_slot=0):
    """Offsets, numbers and sentinels of a call that consumed `layers` from stream position first_pos of the start state."""
    avail_now = R.avail_of(_torch_state_after(start, first_pos)[1]) if first_pos else _entry(start)[3]
    ctl = g.ctl.cpu().tolist()
    base = ctl[4]
    assert base == 624 - avail_now
    offs = ctl[8 + first_slot:8 + first_slot + len(layers)]
    assert offs == [base + int(p) for p in np.concatenate([[0], np.cumsum(layers)[:-1]])]
    n = sum(layers)
    assert np.array_equal(g.numbers(base, n), _entry(start)[4][first_pos:first_pos + n])
    assert g.tails_intact()
    return base


def _layers(cap):
    """Three uneven layers that sum to cap, a zero-length one in between."""
    a, b = cap // 3, cap // 5
    return [a, 0, b, cap - a - b]


# ---------------------------------------------------------------------------------------------------------------------
# a
# ---------------------------------------------------------------------------------------------------------------------
def _whole_stream(cuda, cap, start, prepare):
    words, left, nxt, avail, numbers, blocks = _entry(start)
    g = _Gen(cuda, cap, prepare, 4).run(start, _layers(cap))
    _check_consumed(g, start, _layers(cap))
    k = R.blocks_for(avail, cap)
    raw = g.raw[:624 * (k + 1)].cpu().numpy().view(np.uint32).reshape(k + 1, 624)
    assert np.array_equal(raw, blocks[:k + 1])
    _same_state(g.state, _torch_state_after(start, cap))
    assert int(g.err[0]) == 0 and int(g.ctl[3]) == 0
    return g


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("cap,prepare", [(1, False), (623, True), (624, False), (625, True), (29952, True)])
def test_whole_stream_serial(cuda, cap, prepare, start):
    """Serial kernel: capacities of less than, exactly and just over one block, sized by the header's rule (no plan) or by the
    plan's; 29952 = 48 * 624 is the largest capacity bliss_rng_prepare keeps serial (need = 49 = 33 + 16 blocks)."""
    g = _whole_stream(cuda, cap, start, prepare)
    if prepare:
        assert g.plan == (33, 0, 0, -(-cap // 624) + 1)


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("cap", sorted(PARALLEL))
def test_whole_stream_parallel(cuda, cap, start):
    """Head + jumps + stretches.  29953: the first parallel plan, 3 stretches of 6 that overshoot need = 50 by a block; 175000: 32
    stretches of 8, the shortest length at the stretch cap; 400000: the stretch count capped at 32, stretches of 20.
    A stretch holds 6 .. 8 blocks below the cap of 32 stretches (n = ceil(rest / 8) with rest >= 17, J = ceil(rest / n)) and at
    least 8 from there on."""
    g = _whole_stream(cuda, cap, start, True)
    assert g.plan == PARALLEL[cap]
    b0, J, n, total = g.plan
    assert b0 + n * J == total and 1 <= n <= 32 and total >= -(-cap // 624) + 1
    assert 8 <= J if n == 32 else 6 <= J <= 8


# ---------------------------------------------------------------------------------------------------------------------
# b
# ---------------------------------------------------------------------------------------------------------------------
def _stops(cap, avail, plan):
    ns = {0, 1, avail - 1, avail, avail + 1, avail + 623, avail + 624, avail + 625}
    if plan and plan[2]:
        b0, J, n, _ = plan
        head = avail + b0 * 624                                   # the last number of the head
        ns.update((head, head + 1, cap))
        for seam in {b0 + J, b0 + (n - 1) * J}:                   # the last block of stretch 0 / of the last stretch but one
            ns.update((avail + seam * 624, avail + seam * 624 + 1))
    return sorted(n for n in ns if 0 <= n <= cap)


@pytest.mark.parametrize("start", (0, 1, 624))
@pytest.mark.parametrize("cap", [4000, 29953, 175000])
def test_stop_anywhere_leaves_the_exact_state(cuda, cap, start):
    """One layer of n numbers with is_last, n at the edges of the entry block, of the first regenerated block, of the head (33
    blocks) and of the stretches: the head or a stretch may learn of stop_at early, and commit reads the one raw block n ends
    in.  4000: serial, never prepared; 29953 and 175000: the parallel plans of case a."""
    avail = _entry(start)[3]
    plan = None
    for n in _stops(cap, avail, PARALLEL.get(cap)):
        g = _Gen(cuda, cap, cap in PARALLEL, 1).run(start, [n])
        assert g.plan == PARALLEL.get(cap)
        plan = g.plan
        _check_consumed(g, start, [n])
        _same_state(g.state, _torch_state_after(start, n))
        assert int(g.err[0]) == 0 and int(g.ctl[3]) == 0, n
    if plan:                                                      # the seams were really among the stops
        assert {avail + 33 * 624, avail + 33 * 624 + 1, avail + (33 + plan[1]) * 624 + 1, cap} <= set(_stops(cap, avail, plan))


# ---------------------------------------------------------------------------------------------------------------------
# c
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", (0, 1, 624))
def test_serial_generator_at_a_parallel_capacity(cuda, start, monkeypatch):
    """The serial kernel over 281 blocks, reached in both ways: 175003 is prepared under BLISS_RNG_SERIAL=1 (and only so), 175005
    is never prepared and so has no plan.  Same bits as the parallel generator of case a, i.e. torch's."""
    monkeypatch.setenv("BLISS_RNG_SERIAL", "1")
    g = _whole_stream(cuda, 175003, start, True)
    assert g.plan == (33, 0, 0, 282)
    monkeypatch.delenv("BLISS_RNG_SERIAL")
    g = _whole_stream(cuda, 175005, start, False)
    assert g.plan is None


# ---------------------------------------------------------------------------------------------------------------------
# d
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", (0, 1, 625))
def test_stream_that_runs_short(cuda, start):
    """Capacity 1000 (serial, never prepared), layers 600 + 600: the second layer gets its offset and what is left, the error bit
    arrives, and the generator state is torch's after exactly 1000 draws."""
    g = _Gen(cuda, 1000, False, 2).run(start, [600, 600])
    ctl = g.ctl.cpu().tolist()
    assert int(g.err[0]) & 128 and ctl[3] & 1
    assert ctl[4] == 624 - _entry(start)[3] and ctl[8:10] == [ctl[4], ctl[4] + 600] and ctl[2] == 1000
    assert np.array_equal(g.numbers(ctl[4], 1000), _entry(start)[4][:1000])
    assert g.tails_intact()
    _same_state(g.state, _torch_state_after(start, 1000))


# ---------------------------------------------------------------------------------------------------------------------
# e
# ---------------------------------------------------------------------------------------------------------------------
def _chain(cuda, cap, prepare, start, first, second, ready):
    """begin, `first` layers, chain, `second` layers, end.  Returns the generator, the counts record and its host copy."""
    lib = _L()
    g = _Gen(cuda, cap, prepare, len(first) + len(second))
    rec = torch.arange(1000, 1010, dtype=I32)
    rec[2], rec[5] = first[-1], 0                                  # LayerCounts: word 2 = C, word 5 = err
    counts_dev = rec.to(cuda)
    counts_host = torch.full((10,), -1, dtype=I32).pin_memory()
    g.upload(start)
    g.begin()
    for c in first[:-1]:
        g.wait(c, False)
    g.wait(first[-1], True, counts_dev)
    g.chain(counts_dev, counts_host)
    if ready:
        lib.check(lib.lib.bliss_rng_stream_ready(_st()), "bliss_rng_stream_ready")
    for l, c in enumerate(second):
        g.wait(c, l == len(second) - 1)
    g.end()
    return g, counts_dev.cpu(), counts_host


@pytest.mark.parametrize("ready", (False, True))
@pytest.mark.parametrize("cap", [4001, 29953])
def test_chain_hands_the_generator_over(cuda, cap, ready):
    """The second generator starts where the first call's consumption ended -- at the end of a block, one past it, one short of
    it, or nowhere (n1 = 0) -- without a host round trip.  4001: serial, never prepared; 29953: the parallel plan of case a,
    n1 beyond the head."""
    k, second = (1, [700, 0, 600]) if cap == 4001 else (34, [9000, 0, 16000])
    for start in (0, 1, 624):
        for n1 in [0] + [(r - start) % 624 + k * 624 for r in (0, 1, 623)]:
            first = [n1 // 2, n1 - n1 // 2]
            g, rec, host = _chain(cuda, cap, cap in PARALLEL, start, first, second, ready)
            assert n1 == 0 or (start + n1) % 624 in (0, 1, 623)
            _check_consumed(g, start, second, first_pos=n1, first_slot=2)
            _same_state(g.state, _torch_state_after(start, n1 + sum(second)))
            assert rec.tolist() == list(range(1000, 1002)) + [first[-1]] + [1003, 1004, 0] + list(range(1006, 1010))
            assert torch.equal(host, rec)
            assert int(g.err[0]) == 0 and int(g.ctl[3]) == 0


@pytest.mark.parametrize("start", (0, 625))
def test_chain_reports_a_first_call_that_ran_short(cuda, start):
    """Capacity 1001 (serial, never prepared): 600 + 600 in the first call.  Bit 128 lands in the err word of the counts record
    and in its host copy; the second generator continues after exactly 1001 draws."""
    g, rec, host = _chain(cuda, 1001, False, start, [600, 600], [700], False)
    assert rec[5].item() == 128 and host[5].item() == 128
    assert torch.equal(host, rec)
    _check_consumed(g, start, [700], first_pos=1001, first_slot=2)
    _same_state(g.state, _torch_state_after(start, 1701))
    assert int(g.err[0]) == 0 and int(g.ctl[3]) == 0               # the second call itself had enough


# ---------------------------------------------------------------------------------------------------------------------
# f
# ---------------------------------------------------------------------------------------------------------------------
def _one_shot(state, n, cap, out):
    lib = _L()
    n_dev = torch.tensor([-7, 1 << 30, -1, n, 1 << 30], dtype=I32).to(state.device)
    lib.check(lib.lib.bliss_mt19937_uniform(state.data_ptr(), n_dev.data_ptr(), 3, out.data_ptr(), cap, _st()), "bliss_mt19937_uniform")
    torch.cuda.synchronize()


@pytest.mark.parametrize("start", STARTS)
def test_one_shot_numbers_and_state(cuda, start):
    words, left, nxt, avail, numbers, _ = _entry(start)
    for n in sorted({0, 1, avail, avail + 1, avail + 624, avail + 625, 3 * 624 + 17}):
        state = torch.from_numpy(R.pack626(words, left, nxt)).to(cuda)
        out = torch.full((n + 5 + TAIL,), SENT, dtype=I32, device=cuda)
        _one_shot(state, n, n + 5, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], numbers[:n]), n
        assert (got[n:] == SENT).all(), n
        _same_state(state, _torch_state_after(start, n))


@pytest.mark.parametrize("start", (0, 1, 624))
def test_one_shot_clamps_to_its_capacity(cuda, start):
    words, left, nxt, _, numbers, _ = _entry(start)
    state = torch.from_numpy(R.pack626(words, left, nxt)).to(cuda)
    out = torch.full((2000 + TAIL,), SENT, dtype=I32, device=cuda)
    _one_shot(state, 2000, 700, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[:700], numbers[:700]) and (got[700:] == SENT).all()
    _same_state(state, _torch_state_after(start, 700))


@pytest.mark.parametrize("start", (0, 1, 623))
def test_one_shot_calls_continue_each_other(cuda, start):
    words, left, nxt, avail, numbers, _ = _entry(start)
    state = torch.from_numpy(R.pack626(words, left, nxt)).to(cuda)
    pos = 0
    for n in (avail + 1, 623, 0, 625, 1300):
        out = torch.full((n + TAIL,), SENT, dtype=I32, device=cuda)
        _one_shot(state, n, n, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], numbers[pos:pos + n]) and (got[n:] == SENT).all()
        pos += n
        _same_state(state, _torch_state_after(start, pos))
