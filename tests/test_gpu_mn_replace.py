"""GPU suite (-m gpu): the layer-wise draw WITH replacement (bliss_multinomial_draw_replace, csrc/replace_draw.hip, DESIGN.md section
24) against the CPU restatement (tests/replace_ref.py): picks and marks equal -- the rule is integers only.

C = 1, 7 (fewer candidates than draws), 1024 and 1025 (one chunk of 1024 candidates, and the first with two) and 20000 (20 chunks: the
last workgroup's scan of the chunk totals and both levels of the search)."""
import ctypes as C

import numpy as np
import pytest
import torch

import replace_ref as ref
import wneighbor_ref as wref
from test_replace_ref import CASES, case_counts, check_counts

pytestmark = pytest.mark.gpu

SEED = 1234
GUARD = 8
SIZES = [1, 7, 1024, 1025, 20000]
M64 = ref.M64


def importances(Cn, kind="random"):
    """bf16 bit patterns of ``Cn`` importances: positive over nine octaves with a ninth zeros; "bad": NaN, +-inf and negative
    entries among them; "zero": nothing positive and finite."""
    rng = np.random.default_rng(41 + Cn)
    p = wref.rbf(np.exp2(rng.uniform(-6, 3, Cn)).astype(np.float32))
    p[rng.permutation(Cn)[:Cn // 9]] = 0.0
    if kind == "bad":
        for i, v in enumerate((np.nan, np.inf, -np.inf, -2.0, -0.0)):
            p[(i * 977 + 3) % Cn] = v
    if kind == "zero":
        p[:] = 0.0
        p[::3], p[1::5] = np.nan, np.inf
    return wref.bf16_bits(p)


class Draw:
    """Hand-allocated buffers of direct bliss_multinomial_draw_replace calls, guard words after every output."""

    def __init__(self, dev, cap_c, cap_f):
        from bliss_gnn_amd import _lib
        self.lib, self.dev, self.cap_c, self.cap_f = _lib, dev, cap_c, cap_f
        self.counts = torch.zeros(10, dtype=torch.int32, device=dev)
        self.p = torch.zeros(cap_c, dtype=torch.bfloat16, device=dev)
        self.drawn = torch.full((cap_c + GUARD,), -7, dtype=torch.int32, device=dev)
        self.picks = torch.full((cap_f + GUARD,), -7, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(int(_lib.lib.bliss_multinomial_draw_replace_scratch_bytes(cap_c)) // 8, dtype=torch.int64, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)

    def load(self, p_bits):
        Cn = len(p_bits)
        self.p[:Cn] = torch.from_numpy(np.ascontiguousarray(p_bits).view(np.int16)).to(self.dev).view(torch.bfloat16)
        self.p[Cn:] = 1.0                                                       # (past C: never read for a result)
        self.counts[2] = Cn

    def __call__(self, fanout, step=0, layer=0, bump=0, r_ov=None, set_step=True, picks=True, sync=True):
        if set_step:
            self.step.fill_(step)
        self.drawn.fill_(-7)
        self.picks.fill_(-7)
        rc = self.lib.lib.bliss_multinomial_draw_replace(self.p.data_ptr(), self.counts.data_ptr(), self.cap_c, fanout,
                                                         0 if r_ov is None else r_ov.data_ptr(), SEED, self.step.data_ptr(), layer,
                                                         bump, self.scratch.data_ptr(), self.drawn.data_ptr(),
                                                         self.picks.data_ptr() if picks else 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        if sync:
            torch.cuda.synchronize()

    def assert_equals(self, want_picks, want_drawn):
        Cn, n = len(want_drawn), len(want_picks)
        assert np.array_equal(self.picks[:n].cpu().numpy(), want_picks), "picks"
        assert np.array_equal(self.drawn[:Cn].cpu().numpy(), want_drawn), "marks"
        assert bool((self.picks[n:] == -7).all()) and bool((self.drawn[Cn:] == -7).all()), "written past n / C"
        assert int(self.scratch[0].item()) == 0, "the ticket is not zero"


@pytest.mark.parametrize("Cn", SIZES)
@pytest.mark.parametrize("kind", ["random", "bad", "zero"])
def test_picks_and_marks_equal_the_restatement(cuda, Cn, kind):
    p = importances(Cn, kind)
    for cap_c in (Cn, Cn + 1500):                                                # grids sized from the capacity stride over the true C
        d = Draw(cuda, cap_c, 3000)
        d.load(p)
        for fanout, step, layer in ((16, 0, 0), (512, 3, 1), (3000, 7, 2), (0, 1, 0)):
            d(fanout, step=step, layer=layer)
            pk, drawn = ref.mn_draw(p, fanout, SEED, step, layer)
            assert len(pk) == min(fanout, Cn)
            d.assert_equals(pk, drawn)
            ok = np.isfinite(wref.from_bits(p)) & (wref.from_bits(p) > 0)
            if bool(ok.any()) and len(pk):
                assert bool(ok[pk].all())                                        # only positive finite importances are drawn
    if kind == "zero" and Cn == 20000:
        pk, _ = ref.mn_draw(p, 3000, SEED, 7, 2)
        assert len(set(pk.tolist())) > 2000 and pk.min() < 500 and pk.max() > 19500   # the uniform fallback spans the whole list


@pytest.mark.parametrize("Cn", [7, 1025, 20000])
def test_planted_variates(cuda, Cn):
    """r = 0, r = 2^64 - 1, and pairs (r, r - 1) around prefix boundaries, among them the boundary between two chunks."""
    p = importances(Cn)
    w = ref.fixed_weights(p)
    cum = np.cumsum(np.array(w, dtype=np.int64))
    W = int(cum[-1])
    r = [0, M64]
    marks = sorted(set([0, Cn // 2, Cn - 2] + [c * 1024 - 1 for c in range(1, (Cn + 1023) // 1024)]))
    for i in marks:
        if 0 < int(cum[i]) < W:
            rb = -((-int(cum[i]) << 64) // W)
            assert (rb * W) >> 64 == int(cum[i])
            r += [rb, rb - 1]
    n = min(len(r), Cn)
    r = r[:n]
    d = Draw(cuda, Cn + 100, n)
    d.load(p)
    d(n, r_ov=torch.from_numpy(np.array(r, dtype=np.uint64).view(np.int64)).to(cuda))
    pk, drawn = ref.mn_draw(p, n, SEED, 0, 0, r_override=r)
    d.assert_equals(pk, drawn)
    pos = [i for i in range(Cn) if w[i]]
    assert pk[0] == pos[0] and pk[1] == pos[-1]
    if Cn == 20000:
        assert any(a // 1024 != b // 1024 for a, b in zip(pk[2::2].tolist(), pk[3::2].tolist()))   # a pair straddles two chunks


def test_replay_on_one_scratch_and_the_step_bump(cuda):
    p = importances(20000)
    d = Draw(cuda, 20000, 512)
    d.load(p)
    snaps = []
    for _ in range(2):                                                           # the step rewound: the same draw, the same scratch
        d(512, step=9, layer=1)
        assert int(d.step.item()) == 9
        snaps.append((d.picks.clone(), d.drawn.clone()))
    assert torch.equal(snaps[0][0], snaps[1][0]) and torch.equal(snaps[0][1], snaps[1][1])
    d(512, step=9, layer=1, bump=1)
    assert int(d.step.item()) == 10 and torch.equal(d.picks, snaps[0][0])        # (the call itself drew with step 9)
    d(512, layer=1, bump=1, set_step=False)
    assert int(d.step.item()) == 11
    d.assert_equals(*ref.mn_draw(p, 512, SEED, 10, 1))
    p2 = importances(1025, "bad")                                                # a shorter list on the same scratch: nothing is left over
    d.load(p2)
    d(512, step=4, layer=0)
    d.assert_equals(*ref.mn_draw(p2, 512, SEED, 4, 0))


def test_pick_counts_on_the_device(cuda):
    """p = 1..8, three draws per step, steps 0 .. 2047 counted by the device's own step counter: the restatement's counts, so within
    5 sigma of the multinomial expectation."""
    name = "layer-1..8"
    _, q, m, f = CASES[name]
    d = Draw(cuda, m, f)
    d.load(wref.bf16_bits(np.asarray(q, dtype=np.float32)))
    hits = torch.zeros(m, dtype=torch.int64, device=cuda)
    one = torch.ones(f, dtype=torch.int64, device=cuda)
    for t in range(2048):
        d(f, layer=1, bump=1, set_step=t == 0, sync=False)
        hits.index_add_(0, d.picks[:f].long(), one)
    torch.cuda.synchronize()
    assert int(d.step.item()) == 2048
    assert np.array_equal(hits.cpu().numpy(), case_counts(name, 2048))
    check_counts(hits.cpu().numpy(), name, 2048)
