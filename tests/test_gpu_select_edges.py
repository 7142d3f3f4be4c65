"""GPU suite (-m gpu): the candidate -> kept stage of csrc/sampler.hip called DIRECTLY on hand-made candidate lists --
bliss_poisson_select, bliss_poisson_select_keyed, bliss_multinomial_select, bliss_multinomial_select_marked (k_poisson_scale,
k_select_fused / k_select_keyed with their look-back over 1024-candidate chunks, k_mn_*) -- against the host restatement
tests/select_ref.py, buffer for buffer with torch.equal on integer views: there is no tolerance anywhere.

Every output buffer is TAIL entries longer than its capacity and pre-filled with a sentinel, and the expected buffers hold the
sentinels; the counts record is pre-filled with garbage and only the documented fields may change; hist goes in as the bincount of
p's patterns and must come back zero; the status words have cap_c / 1024 + 2 entries (include/bliss_gnn.h) and sentinels behind.
The lists and case tables live in select_ref.py: tests/test_select_ref.py (CPU) checks the exact-sum condition on the same inputs
and shows that a structural model with one fault planted fails this module's comparison on them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import select_ref as R

pytestmark = pytest.mark.gpu

TAIL, SENT = R.TAIL, R.SENT
GARBAGE = dict(E=0x1111, K=0x2222, B=0x3333, iters=0x4444, all_one=0x5555, c=-123.25)
U_OFF = 11                                                     # *uniforms_offset_dev of the buffer path


@functools.lru_cache(maxsize=None)
def _list(n, kind, seed):
    return R.make_list(n, kind, seed)


def _window(n):
    return _list(n, "window", n)


class Ws:
    """A hand-built bliss_layer_ws_t with the fields the candidate -> kept stage reads, every output followed by guard entries."""

    def __init__(self, dev, cap_c, cap_k, V, n_in=None):
        from bliss_gnn_amd import _lib
        self.lib, self.dev, self.cap_c, self.cap_k, self.V = _lib, dev, cap_c, cap_k, V
        n_in = max(cap_c, n_in or 0)
        i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
        i16 = lambda n: torch.zeros(n, dtype=torch.int16, device=dev)
        self.counts = i32(12)
        self.p, self.cand_nid = i16(n_in + TAIL), i32(n_in + TAIL)
        self.P, self.node_prob = i16(cap_c + TAIL), i16(cap_k + TAIL)
        self.new_id, self.kept_nid, self.kept_map = i32(cap_c + TAIL), i32(cap_k + TAIL), i32(V + TAIL)
        self.hist = i32(R.HIST_BINS)
        self.n_state = cap_c // R.CHUNK + 2
        self.chunk_cnt = i32(self.n_state + TAIL, SENT["chunk_cnt"])
        self.uniforms = torch.zeros(U_OFF + n_in + 8, dtype=torch.float32, device=dev)      # (u = 0 in front: kept if the offset is lost)
        self.u_off = i32(1, U_OFF)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.fs_ticket = i32(1)
        self.chosen = i32(n_in + 8)

    def load(self, p_bits, cand, S, n, counts_extra=None):
        """The inputs of one call: the list, the counts record (garbage apart from S, C and err = 0), hist, fresh sentinels."""
        self.p[:n] = p_bits[:n].to(torch.int16).to(self.dev)
        self.cand_nid[:n] = cand[:n].to(self.dev)
        rec = self.lib.LayerCounts(S=S, C=n, err=0, **{**GARBAGE, **(counts_extra or {})})
        self.rec_in = rec
        self.counts[:10] = torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.int32).copy()).to(self.dev)
        for name in ("P", "new_id", "kept_nid", "node_prob", "kept_map"):
            getattr(self, name).fill_(SENT[name])
        self.chunk_cnt[self.n_state:] = SENT["chunk_cnt"]

    def struct(self, kept_map=True, fs_ticket=False):
        ws = self.lib.LayerWs()
        for name in ("counts", "chunk_cnt", "cand_nid", "p", "P", "new_id", "kept_nid", "node_prob", "hist"):
            setattr(ws, name, getattr(self, name).data_ptr())
        ws.cap_c, ws.cap_k = self.cap_c, self.cap_k
        ws.kept_map = self.kept_map.data_ptr() if kept_map else 0
        ws.fs_ticket = self.fs_ticket.data_ptr() if fs_ticket else 0
        return ws

    def result(self, kept_map=True):
        torch.cuda.synchronize()
        rec = self.lib.LayerCounts.from_buffer_copy(self.counts[:10].cpu().numpy().tobytes())
        # only the documented fields may change
        assert (rec.S, rec.E, rec.C, rec.B) == (self.rec_in.S, self.rec_in.E, self.rec_in.C, self.rec_in.B), "S / E / C / B changed"
        assert bool((self.chunk_cnt[self.n_state:] == SENT["chunk_cnt"]).all()), "the sentinels behind the status words were overwritten"
        got = dict(K=rec.K, err=rec.err, c=float(rec.c), iters=rec.iters, all_one=rec.all_one)
        for name in ("P", "node_prob"):
            got[name] = getattr(self, name).cpu().to(torch.int32) & 0xFFFF
        for name in ("new_id", "kept_nid"):
            got[name] = getattr(self, name).cpu()
        if kept_map:
            got["kept_map"] = self.kept_map.cpu()
        else:
            assert bool((self.kept_map == SENT["kept_map"]).all()), "kept_map written although the pointer was NULL"
        return got


def _st():
    return torch.cuda.current_stream().cuda_stream


def poisson(ws, p, cand, S, n, fanout, eps, draw, kept_map=True, alone=None, bump=0, cand_bound=None):
    """One bliss_poisson_select (draw: an fp32 vector, planted behind U_OFF) or bliss_poisson_select_keyed (draw: (seed, step,
    layer)) call on a freshly loaded workspace -> (got, want).  alone = (c, all_one): select alone -- fs_ticket is set, so the call
    skips its scale launch; the test plays bliss_frontier_prob's part: it writes counts.c / all_one / iters and zeroes the ticket
    and the status words the select will use."""
    lib = ws.lib
    hist = R.histogram(p, n)
    if alone is None:
        ws.load(p, cand, S, n)
        ws.hist.copy_(hist.to(ws.dev))
        c, iters, all_one = R.scale(p, n, fanout, eps)
    else:
        c, all_one = alone
        iters = 7
        ws.load(p, cand, S, n, dict(c=c, all_one=all_one, iters=iters))
        ws.hist.zero_()
        ws.chunk_cnt[:min(n, ws.cap_c) // R.CHUNK + 2] = 0        # bliss_frontier_prob's part: the ticket + one word per chunk
        ws.fs_ticket.zero_()
    s = ws.struct(kept_map, fs_ticket=alone is not None)
    bound = ws.cap_c if cand_bound is None else cand_bound
    if isinstance(draw, tuple):
        seed, step, layer = draw
        ws.step.fill_(step)
        lib.check(lib.lib.bliss_poisson_select_keyed(C.byref(s), fanout, eps, seed, ws.step.data_ptr(), layer, bump, bound, _st()),
                  "bliss_poisson_select_keyed")
    else:
        ws.uniforms[U_OFF:U_OFF + n] = draw[:n].to(ws.dev)
        lib.check(lib.lib.bliss_poisson_select(C.byref(s), fanout, eps, ws.uniforms.data_ptr(), ws.u_off.data_ptr(), 0, 0, 0, bound,
                                               _st()), "bliss_poisson_select")
    got = ws.result(kept_map)
    assert int(ws.hist.abs().sum()) == 0, "hist is not zero after the call"
    assert int(ws.fs_ticket) == 0 and int(ws.u_off) == U_OFF
    if isinstance(draw, tuple):
        got["step"] = int(ws.step)
    r = R.select(p, cand, S, n, c, all_one, draw, ws.cap_c, ws.cap_k, num_nodes=ws.V if kept_map else None)
    want = R.want_buffers(r, ws.cap_c, ws.cap_k)
    want.update(c=float(c), iters=iters, all_one=all_one)
    if isinstance(draw, tuple):
        want["step"] = draw[1] + (1 if bump else 0)
    return got, want


def _check(got, want, what):
    diff = R.compare(got, want)
    assert diff == [], (what, diff)


KEY = (1234, 2 ** 40 + 3, 2)


@pytest.mark.parametrize("n", R.SIZES)
def test_scale_and_select_on_the_ladder(cuda, n):
    """k_poisson_scale + the select, both entry points, cap_c = C + 3000 (whole trailing workgroups draw tickets past the last
    chunk) and cap_c = C, every fanout class, the S ladder, kept_map given and NULL."""
    p, cand, V = _window(n)
    u = R.make_uniforms(p, n)
    for cap_c in (n + 3000, n):
        ws = Ws(cuda, cap_c, cap_c, V)
        for i, fan in enumerate(R.fanouts(n)):
            S = R.seeds_for(n, i + (cap_c == n))
            for draw in (u, KEY):
                km = (i + isinstance(draw, tuple)) % 2 == 0
                got, want = poisson(ws, p, cand, S, n, fan, 0.9999, draw, kept_map=km, bump=i % 2)
                assert want["err"] == 0
                _check(got, want, (n, cap_c, fan, S, "keyed" if isinstance(draw, tuple) else "buffer"))


@pytest.mark.parametrize("n,kind", R.KIND_CASES)
def test_scale_and_select_on_lists_outside_the_window(cuda, n, kind):
    """p = 0 (the bin-0 counter), p >= 2 (bins >= 0x4000), p < 2^-31 (below the window), 0x7fc0 (c becomes NaN; every P of a
    non-seed is the pattern 0x7fc0 and is never drawn), the list whose fixed point does not settle (iters = 50); eps 0.9999 / 0.99."""
    p, cand, V = _list(n, kind, n + 7)
    u = R.make_uniforms(p, n + 7)
    ws = Ws(cuda, n + 3000, n + 3000, V)
    seen = set()
    for i, (fan, eps) in enumerate([(f, 0.9999) for f in R.fanouts(n)] + [(max(n // 3, 1), 0.99)]):
        for draw in (u, KEY):
            got, want = poisson(ws, p, cand, R.seeds_for(n, i), n, fan, eps, draw)
            _check(got, want, (n, kind, fan, eps))
            seen.add(want["iters"])
    assert 50 in seen or kind not in ("nan", "unsettled")      # (other lists may run out of iterations too: fanout C - 1)


def _alone_cases():
    n = 150000
    p, cand, V = _window(n)
    gen = torch.Generator().manual_seed(4)
    u = torch.rand(n, generator=gen)
    far = u.clone()
    far[[5, 100000, 100001, n - 1]] = 0.0
    per_chunk = torch.ones(n)
    per_chunk[torch.arange(R.chunks(n)) * R.CHUNK + torch.randint(0, n - (R.chunks(n) - 1) * R.CHUNK, (R.chunks(n),), generator=gen)] = 0.0
    first = torch.ones(n)
    first[:R.CHUNK] = 0.0
    pp, pc, pV = _list(n, "payload", n + 7)
    sp, sc, sV = _list(3000, "payload", 3007)
    return [("c = 2^-16: runs of far more than 64 empty chunks", p, cand, V, 0, 2.0 ** -16, 0, far),
            ("c = 1e9: every P = 1, K = C", p, cand, V, 64, 1e9, 0, u),
            ("all_one", p, cand, V, 1, 0.001, 1, u),
            ("exactly one kept per chunk", p, cand, V, 0, 1.0, 0, per_chunk),
            ("all of chunk 0 and nothing after it", p, cand, V, 0, 1.0, 0, first),
            ("0xffc0, 0x7fc0, 0, a denormal and values above 1", pp, pc, pV, 4000, 0.37, 0, R.make_uniforms(pp, 1)),
            ("the same palette, three chunks, c above 1", sp, sc, sV, 1025, 3.0, 0, R.make_uniforms(sp, 2))]


def test_select_alone_with_an_arbitrary_scale(cuda):
    """fs_ticket set: no scale launch; c and all_one as the test wrote them."""
    for what, p, cand, V, S, c, all_one, u in _alone_cases():
        n = int(p.numel())
        ws = Ws(cuda, n + 3000, n + 3000, V)
        for draw in (KEY, u):
            got, want = poisson(ws, p, cand, S, n, 3, 0.9999, draw, alone=(c, all_one))
            _check(got, want, what)
        if what.startswith("c = 1e9") or what == "all_one":
            assert want["K"] == n
        if what.startswith("exactly one"):
            assert want["K"] == R.chunks(n)
        if what.startswith("all of chunk 0"):
            assert want["K"] == R.CHUNK and int(want["new_id"][:n].max()) == R.CHUNK - 1


def test_capacity_clamps(cuda):
    """cap_k in {K, K - 1, S}: bit 4, K = cap_k, the entries below cap_k correct, the sentinels intact.  cap_c = C - 1: the kernels
    work on min(counts.C, cap_c) candidates."""
    for n, fan, S in ((3000, 1000, 64), (66561, 22187, 1025)):
        p, cand, V = _window(n)
        u = R.make_uniforms(p, n)
        c, _, all_one = R.scale(p, n, fan)
        K = R.select(p, cand, S, n, c, all_one, u, n, n)["K"]
        assert S < K - 1 < n
        for cap_k in (K, K - 1, S):
            ws = Ws(cuda, n, cap_k, V)
            for draw in (u, KEY):
                got, want = poisson(ws, p, cand, S, n, fan, 0.9999, draw)
                if not isinstance(draw, tuple):
                    assert (want["err"], want["K"]) == ((0 if cap_k == K else R.ERR_CAP_KEPT), cap_k)
                _check(got, want, (n, cap_k))
    for n in (1000, 3000):
        p, cand, V = _window(n)
        ws = Ws(cuda, n - 1, n, V, n_in=n)
        for draw in (R.make_uniforms(p, n), KEY):
            got, want = poisson(ws, p, cand, 64, n, n // 3, 0.9999, draw)
            assert want["P"].numel() == n - 1 + TAIL
            _check(got, want, (n, "cap_c = C - 1"))


@pytest.mark.parametrize("n,cap_c", [(3000, 6000), (1025, 1025)])
def test_keyed_draw(cuda, n, cap_c):
    """64-bit step and the layer byte in the key; bump_step: the step word advances by exactly one or not at all, also when the
    grid is larger than the chunk count (cap_c = 6000: six workgroups, three chunks); the buffer path with keyed_uniform's values
    planted gives the same outputs."""
    from oracle import bliss_oracle as bo
    p, cand, V = _window(n)
    ws = Ws(cuda, cap_c, cap_c, V)
    seen = set()
    for step in (0, 1, 2 ** 40 + 3):
        for layer in (0, 2, 255):
            for bump in (0, 1):
                got, want = poisson(ws, p, cand, 64, n, n // 3, 0.9999, (1234, step, layer), bump=bump)
                _check(got, want, (step, layer, bump))
                assert got["step"] == step + bump
                seen.add(tuple(got["new_id"][:n].tolist()))
            u = bo.keyed_uniform(1234, step, layer, cand.long())
            got_u, want_u = poisson(ws, p, cand, 64, n, n // 3, 0.9999, u)
            _check(got_u, want_u, (step, layer, "buffer"))
            for k in ("P", "new_id", "kept_nid", "node_prob", "kept_map", "K", "c", "iters"):
                _check({k: got_u[k]}, {k: got[k]}, (step, layer, "buffer == keyed", k))
    assert len(seen) == 9                                       # every (step, layer) draws its own set


def multinomial(ws, p, cand, S, n, marks=None, chosen=None, kept_map=True):
    """bliss_multinomial_select_marked (marks) or bliss_multinomial_select (chosen) -> (got, want)."""
    lib = ws.lib
    ws.load(p, cand, S, n)
    ws.hist.zero_()
    s = ws.struct(kept_map)
    if chosen is None:
        ws.new_id[:n] = marks.to(ws.dev)
        lib.check(lib.lib.bliss_multinomial_select_marked(C.byref(s), _st()), "bliss_multinomial_select_marked")
    else:
        k = int(chosen.numel())
        ws.chosen[:k] = chosen.to(ws.dev)
        lib.check(lib.lib.bliss_multinomial_select(C.byref(s), ws.chosen.data_ptr() if k else 0, k, _st()), "bliss_multinomial_select")
    got = ws.result(kept_map)
    assert int(ws.hist.abs().sum()) == 0
    r = R.mn_select(p, cand, S, n, marks, ws.cap_c, ws.cap_k, num_nodes=ws.V if kept_map else None, chosen=chosen)
    want = R.want_buffers(r, ws.cap_c, ws.cap_k)
    want.update(c=GARBAGE["c"], iters=GARBAGE["iters"], all_one=GARBAGE["all_one"])      # not this stage's fields
    return got, want


def _chosen(marks, seed):
    idx = torch.nonzero(marks).flatten().to(torch.int32)
    return idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize("n", R.SIZES)
def test_multinomial_selects_on_the_ladder(cuda, n):
    """Both entry points against mn_select and against each other: marks none (n_chosen = 0) / all / only seeds / only non-seeds /
    one per chunk / random 0.3, the S ladder, cap_c = C + 3000 and C; chosen holding -1 and C: bit 2, the rest still marked."""
    p, cand, V = _list(n, "payload", n + 7)
    wss = [Ws(cuda, n + 3000, n + 3000, V), Ws(cuda, n, n, V)]
    for i, pattern in enumerate(R.MARKS):
        S = R.seeds_for(n, i)
        marks = R.mark_list(n, S, pattern, n + i)
        ws = wss[i % 2]
        got_m, want = multinomial(ws, p, cand, S, n, marks=marks, kept_map=i % 3 != 0)
        _check(got_m, want, (n, pattern, "marked"))
        got_c, want_c = multinomial(ws, p, cand, S, n, chosen=_chosen(marks, i), kept_map=i % 3 != 0)
        _check(got_c, want_c, (n, pattern, "chosen"))
        _check(got_c, got_m, (n, pattern, "chosen == marked"))
        assert want["err"] == 0 and want["K"] == int(((marks == 1) | (torch.arange(n) < S)).sum())
    clean, _ = multinomial(wss[1], p, cand, S, n, chosen=_chosen(marks, 9))
    bad = torch.cat([torch.tensor([n], dtype=torch.int32), _chosen(marks, 9), torch.tensor([-1], dtype=torch.int32)])
    got, want_b = multinomial(wss[1], p, cand, S, n, chosen=bad)
    assert want_b["err"] == R.ERR_CAP_CAND and clean["err"] == 0
    _check(got, want_b, (n, "chosen out of range"))
    _check({k: v for k, v in got.items() if k != "err"}, {k: v for k, v in clean.items() if k != "err"}, (n, "the rest still marked"))


def test_multinomial_capacity_clamps(cuda):
    n, S = 3000, 64
    p, cand, V = _list(n, "payload", n + 7)
    marks = R.mark_list(n, S, "random", 5)
    K = int(((marks == 1) | (torch.arange(n) < S)).sum())
    for cap_k in (K, K - 1, S):
        ws = Ws(cuda, n, cap_k, V)
        got_m, want = multinomial(ws, p, cand, S, n, marks=marks)
        assert (want["err"], want["K"]) == ((0 if cap_k == K else R.ERR_CAP_KEPT), cap_k)
        _check(got_m, want, (cap_k, "marked"))
        got_c, want_c = multinomial(ws, p, cand, S, n, chosen=_chosen(marks, 1))
        _check(got_c, want_c, (cap_k, "chosen"))


def test_twelve_calls_on_one_workspace(cuda):
    """Alternating list sizes with C = 1 rounds in between, buffer and keyed draws in turn, nothing re-zeroed by the test but the
    outputs' sentinels: the scale re-zeroes the ticket and the status words, hist comes back clean -- every call equals a
    fresh-state call (the restatement knows no state)."""
    cap = 150000 + 3000
    ws = Ws(cuda, cap, cap, 2 * 150000 + 11)
    for i, (n, fan) in enumerate(R.REUSE_ROUNDS):
        p, cand, V = _window(n)
        draw = R.make_uniforms(p, n) if i % 2 == 0 else (99, i, i)
        got, want = poisson(ws, p, cand, R.seeds_for(n, i), n, fan, 0.9999, draw, bump=1, cand_bound=cap if i % 3 else n)
        _check(got, want, (i, n, fan))
