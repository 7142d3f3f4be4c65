"""GPU suite: the kernels of the static-shape sharded sampler (csrc/shard_dense.hip) and their routed twins (csrc/shard.hip), called
directly through the C ABI on one GPU with no process group, against the host restatement tests/shard_dense_ref.py at the shapes
where an ordered compaction by decoupled look-back, a last-workgroup ticket and a grid-stride loop go wrong.

Rules of this module: every output buffer is longer than its capacity and pre-filled with a sentinel, and nothing behind the
documented extent may change; what a kernel must define is pre-filled with garbage; after every call the error word holds exactly
the expected bits (BLISS_ERR_FLAG_TIMEOUT never); comparisons are torch.equal on integer views (shard_dense_ref.compare) -- the
results are integers and bf16 bit patterns, there is no tolerance anywhere.  tests/test_shard_dense_ref.py shows on the CPU that
this comparison fails for each of a list of planted faults on this module's own inputs."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

import shard_dense_ref as R                                   # noqa: E402

TAIL = R.TAIL
GARBAGE = 0x0BADBAD
SEED = 7


def _lib():
    from bliss_gnn_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _d(t):
    return t.to("cuda:0")


def _bf(n, sentinel):
    """A bf16 buffer of n entries, as its int16 bit view, filled with ``sentinel``."""
    return torch.full((n,), sentinel, dtype=torch.int16, device="cuda:0")


def _bits16(t):
    return t.cpu().to(torch.int32) & 0xFFFF


def _counts(words=None):
    c = torch.full((10 + 4,), GARBAGE, dtype=torch.int32)
    if words is not None:
        c[:10] = words
    return _d(c)


def _read_counts(c):
    lib = _lib()
    raw = c.cpu()
    return lib.LayerCounts.from_buffer_copy(raw[:10].numpy().tobytes()), raw


def _rec_words(C, c, all_one):
    """A LayerCounts as bliss_poisson_scale leaves it, for hand-made lists."""
    lc = _lib().LayerCounts(S=GARBAGE, E=GARBAGE, C=C, K=GARBAGE, B=GARBAGE, err=0, iters=3, all_one=all_one, c=c)
    return torch.frombuffer(bytearray(bytes(lc)), dtype=torch.int32).clone()


class Scratch:
    """The shared status-word array of one (num_nodes, cap_c): candidate pass's words, kept pass's words, the ticket, a sentinel tail.
    Starts zeroed, as the product allocates it; no test writes a tag into it."""

    def __init__(self, V, cap_c):
        self.nb_c, self.nb_k = R.blocks(V), R.blocks(cap_c)
        w = torch.zeros(R.scratch_words(V, cap_c) + 8, dtype=torch.int64)
        w[-8:] = -5
        self.w = _d(w)

    def check(self, after):
        w = self.w.cpu()
        assert torch.equal(w[-8:], torch.full((8,), -5, dtype=torch.int64)), "wrote behind the scratch array"
        assert int(w[self.nb_c + self.nb_k]) == 0, "ticket word not returned to zero"
        other = w[self.nb_c: self.nb_c + self.nb_k] if after == "candidates" else w[: self.nb_c]
        assert not other.any(), f"the other pass's status words are not zero after {after}"
        own = w[: self.nb_c] if after == "candidates" else w[self.nb_c: self.nb_c + self.nb_k]
        assert bool(((own >> 62) & 3 == 2).all()), f"a status word of {after} holds no inclusive prefix"


def _err_buf():
    e = torch.zeros(4, dtype=torch.int32)
    e[1:] = 99
    return _d(e)


def _read_err(e):
    e = e.cpu()
    assert e[1:].tolist() == [99, 99, 99]
    return int(e[0])


def run_candidates(dense, uniform, cap_c, scr=None, dense_d=None):
    """bliss_shard_candidates on ``dense`` ([V, 2] on the host, or already on the device with its tail) -> (got, device state)."""
    lib = _lib()
    V = dense.shape[0]
    scr = scr or Scratch(V, cap_c)
    if dense_d is None:
        dense_d = _d(torch.cat([dense.flatten(), torch.full((2 * TAIL,), 0x1111, dtype=torch.int64)]))
    s = dict(cand=torch.full((cap_c + TAIL,), R.SENT["cand_nid"], dtype=torch.int32, device="cuda:0"), p=_bf(cap_c + TAIL, R.SENT["p"]),
             is_seed=torch.full((cap_c + TAIL,), R.SENT["is_seed"], dtype=torch.uint8, device="cuda:0"),
             hist=_d(torch.cat([torch.zeros(R.HIST_BINS, dtype=torch.int32), torch.full((TAIL,), 77, dtype=torch.int32)])),
             counts=_counts(), err=_err_buf(), scr=scr, dense=dense_d, V=V, cap_c=cap_c)
    lib.check(lib.lib.bliss_shard_candidates(dense_d.data_ptr(), V, uniform, s["cand"].data_ptr(), s["p"].data_ptr(), s["is_seed"].data_ptr(),
                                             s["hist"].data_ptr(), s["counts"].data_ptr(), cap_c, scr.w.data_ptr(), s["err"].data_ptr(), _st()),
              "bliss_shard_candidates")
    torch.cuda.synchronize()
    lc, raw = _read_counts(s["counts"])
    assert raw[10:].tolist() == [GARBAGE] * 4 and (lc.S, lc.E, lc.K, lc.B) == (GARBAGE,) * 4, "counts: a field outside C / err / iters / all_one changed"
    hist = s["hist"].cpu()
    dn = dense_d.cpu()
    assert hist[R.HIST_BINS:].tolist() == [77] * TAIL and dn[2 * V:].tolist() == [0x1111] * (2 * TAIL)
    scr.check("candidates")
    got = dict(cand_nid=s["cand"].cpu(), p=_bits16(s["p"]), is_seed=s["is_seed"].cpu().to(torch.int32), hist=hist[:R.HIST_BINS], C=lc.C,
               counts_err=lc.err, iters=lc.iters, all_one=lc.all_one, err=_read_err(s["err"]), dense=dn[: 2 * V].view(V, 2))
    return got, s


def run_scale(s, fanout):
    """bliss_poisson_scale on the histogram and counts that run_candidates left."""
    lib = _lib()
    C = _read_counts(s["counts"])[0].C
    n = R.blocks(C) + 2
    sel = _d(torch.cat([torch.full((n,), GARBAGE, dtype=torch.int32), torch.full((TAIL,), 55, dtype=torch.int32)]))
    lib.check(lib.lib.bliss_poisson_scale(s["hist"].data_ptr(), s["counts"].data_ptr(), fanout, 0.9999, sel.data_ptr(), _st()), "bliss_poisson_scale")
    torch.cuda.synchronize()
    lc, _ = _read_counts(s["counts"])
    sel = sel.cpu()
    assert sel[n:].tolist() == [55] * TAIL and not sel[:n].any()
    hist = s["hist"].cpu()
    assert hist[R.HIST_BINS:].tolist() == [77] * TAIL
    return dict(c=float(lc.c), all_one=lc.all_one, iters=lc.iters, hist=hist[:R.HIST_BINS]), lc


def run_select(cand_d, p_d, is_seed_d, counts_d, V, cap_c, cap_k, seeds_g, S, step, layer, n_local=5, bump=1, seeds_on_device=False, flag=True,
               scr=None, kept_map_d=None):
    """bliss_shard_select_kept -> got (every buffer with its tail)."""
    lib = _lib()
    scr = scr or Scratch(V, cap_c)
    seeds_d = _d(torch.cat([seeds_g[:S].to(torch.int32), torch.full((3,), -1, dtype=torch.int32)]))
    n_dev = _d(torch.tensor([S, -1], dtype=torch.int32))
    step_d = _d(torch.tensor([step, -3], dtype=torch.int64))
    P = _bf(cap_c + TAIL, R.SENT["P"])
    kept = torch.full((cap_k + TAIL,), R.SENT["kept_nid"], dtype=torch.int32, device="cuda:0")
    prob = _bf(cap_k + TAIL, R.SENT["node_prob"])
    kmap = kept_map_d if kept_map_d is not None else torch.full((V + TAIL,), -1, dtype=torch.int32, device="cuda:0")
    layer_counts = _counts()
    nloc = _d(torch.tensor([n_local, -1], dtype=torch.int32))
    done = _d(torch.tensor([0, -1], dtype=torch.int32))
    err = _err_buf()
    lib.check(lib.lib.bliss_shard_select_kept(cand_d.data_ptr(), p_d.data_ptr(), is_seed_d.data_ptr(), counts_d.data_ptr(), SEED, step_d.data_ptr(),
                                              layer, seeds_d.data_ptr(), -1 if seeds_on_device else S, n_dev.data_ptr() if seeds_on_device else 0,
                                              P.data_ptr(), kept.data_ptr(), prob.data_ptr(), kmap.data_ptr(), cap_k, cap_c, V,
                                              layer_counts.data_ptr(), nloc.data_ptr(), scr.w.data_ptr(), bump, done.data_ptr() if flag else 0,
                                              err.data_ptr(), _st()), "bliss_shard_select_kept")
    torch.cuda.synchronize()
    lc, raw = _read_counts(layer_counts)
    assert raw[10:].tolist() == [GARBAGE] * 4 and (lc.S, lc.E, lc.B, lc.err, lc.iters, lc.all_one) == (GARBAGE,) * 6, "layer_counts: a field besides K / C changed"
    assert done.cpu().tolist() == [1 if flag else 0, -1], "done flag"
    assert int(step_d[1]) == -3 and n_dev.cpu().tolist() == [S, -1] and int(nloc[1]) == -1
    scr.check("select")
    return dict(P=_bits16(P), kept_nid=kept.cpu(), node_prob=_bits16(prob), kept_map=kmap.cpu(), K=lc.K, layer_C=lc.C, err=_read_err(err),
                step=int(step_d[0]))


def _same(got, want):
    diff = R.compare(got, want)
    assert diff == [], diff


def _scale_ok(hist, C, fanout):
    """The oracle's loop divides by the sum of min(c p, 1): a list whose importances are all zero has no scale."""
    return C <= fanout or int(hist[1:].sum()) > 0


# ------------------------------------------------------------------------------------------------------ bliss_shard_candidates
def _candidates_case(dense, uniform, cap_c, fanout_of, then_select=False, step=0, layer=0):
    V = dense.shape[0]
    got, s = run_candidates(dense, uniform, cap_c)
    want = R.want_candidates(dense, uniform, cap_c)
    _same(got, want)
    C = want["C"]
    fanout = max(1, fanout_of(C))
    if not _scale_ok(want["hist"], C, fanout):
        return
    sc, lc = run_scale(s, fanout)
    _same(sc, R.scale(want["hist"], C, fanout))
    assert (lc.C, lc.err) == (C, 0)
    if then_select:
        cand, p, sd = want["cand_nid"][:C], want["p"][:C], want["is_seed"][:C].to(torch.uint8)
        seeds = cand[sd.bool()].flip(0)                              # (descending: not the candidates' order)
        S = int(seeds.numel())
        w = R.want_select(cand, p, sd, C, sc["c"], sc["all_one"], SEED, step, layer, seeds, S, V, cap_c, V, 5, 1)
        g = run_select(s["cand"], s["p"], s["is_seed"], s["counts"], V, cap_c, V, seeds, S, step, layer, scr=s["scr"])
        _same(g, w)


FANOUTS = [lambda C: C + 3, lambda C: C, lambda C: C - 1, lambda C: C // 50, lambda C: C // 3]


@pytest.mark.parametrize("V", R.CAND_SIZES)
def test_candidates_at_edge_sizes(cuda, V):
    """Every mark pattern that fits the size, marks of 1, 2 and 8 ranks, uniform_nodes 0 and 1, cap_c in {C, C - 1, 1, V}; the
    Poisson scale on the histogram each call leaves (fanouts above, at, just below and far below C in turn); on the random and gap
    patterns the kept pass on top, on the same scratch array."""
    n = 0
    for pi, pattern in enumerate(R.PATTERNS):
        for uniform in (0, 1):
            ranks = (1, 2, 8)[(pi + uniform) % 3]
            dense = R.make_dense(V, pattern, ranks, seed=1000 + 17 * pi + uniform)
            if dense is None:
                continue
            C = int((dense[:, 1] != 0).sum())
            caps = R.cap_choices(C, V) if pattern in ("all", "random", "one_per_block", "first") and not uniform else [max(C, 1)]
            for cap_c in caps:
                _candidates_case(dense, uniform, cap_c, FANOUTS[n % len(FANOUTS)], then_select=pattern.startswith("gap") or pattern == "random",
                                 step=(0, 1, (1 << 40) + 3)[n % 3], layer=(0, 2, 255)[n % 3])
                n += 1
    assert n >= 12


def test_candidates_with_more_workgroups_than_are_resident(cuda):
    """|V| = 2 449 029: 2392 look-back blocks, far more than the device holds at once -- sd_lookback relies on workgroups being
    dispatched in index order.  Random density 0.3 with a run of 130 empty blocks cut into it; then the scale and the kept pass."""
    V = R.CAND_BIG
    dense = R.make_dense(V, "random", 8, seed=77)
    dense[1000 * R.BLOCK: 1130 * R.BLOCK] = 0
    dense[999 * R.BLOCK: 1000 * R.BLOCK, 1] = 1
    dense[1130 * R.BLOCK: 1131 * R.BLOCK, 1] = R.SEED_MARK + 2
    _candidates_case(dense, 0, V, lambda C: C // 50, then_select=True, step=(1 << 40) + 3, layer=2)


# ----------------------------------------------------------------------------------------------------- bliss_shard_select_kept
def _hand_case(C, S, c, all_one, k, cap_k_kind="K"):
    V = max(2 * C + 7, 16)
    cap_c = C + 3000                                                  # whole trailing workgroups find nothing
    cand, p, sd, seeds = R.hand_list(C, V, S, seed=300 + C % 1000 + S)
    step, layer = (0, 1, (1 << 40) + 3)[k % 3], (0, 2, 255)[(k // 3) % 3]
    bump, on_dev, flag = k % 2, (k // 2) % 2 == 1, (k // 4) % 2 == 0
    n_local = 11 + k
    K_true = R.select_kept(cand, p, sd, C, c, all_one, SEED, step, layer, seeds, S, 1 << 30, torch.full((V,), -1, dtype=torch.int32), n_local, bump)["K"]
    cap_k = dict(K=max(K_true, 1), Km1=K_true - 1, S=S)[cap_k_kind]
    if cap_k < 1:
        return False
    want = R.want_select(cand, p, sd, C, c, all_one, SEED, step, layer, seeds, S, cap_k, cap_c, V, n_local, bump)
    assert want["err"] == (R.ERR_CAP_KEPT if cap_k < K_true else 0)
    cand_d = _d(R.padded(cand, cap_c + TAIL, R.SENT["cand_nid"]))
    p_d = _d(R.padded(p, cap_c + TAIL, R.SENT["p"]).to(torch.int16))
    sd_d = _d(R.padded(sd, cap_c + TAIL, R.SENT["is_seed"]))
    got = run_select(cand_d, p_d, sd_d, _d(_rec_words(C, c, all_one)), V, cap_c, cap_k, seeds, S, step, layer, n_local=n_local, bump=bump,
                     seeds_on_device=on_dev, flag=flag)
    _same(got, want)
    assert torch.equal(cand_d.cpu(), R.padded(cand, cap_c + TAIL, R.SENT["cand_nid"]))          # inputs untouched
    return True


@pytest.mark.parametrize("C", [0, 1, 1024, 1025, 65 * 1024 + 1, 150000])
def test_select_kept_on_hand_made_lists(cuda, C):
    """p with 0 and two NaN patterns; all_one, c so large that every P = 1, c so small that almost nothing is drawn (runs of more
    than 64 kept-pass blocks with a count of 0), an ordinary c; S in {0, 1, 64, 4000} in an order that is not ascending, passed on
    the host and through *n_seeds_dev; step in {0, 1, 2^40 + 3}, layer in {0, 2, 255}; bump_step and done_flag on and off;
    cap_k in {K, K - 1, S}."""
    k = ran = 0
    for S in (0, 1, 64, 4000):
        if S > C:
            continue
        for c, all_one in ((1.0, 1), (1.0e9, 0), (2.0 ** -16, 0), (0.37, 0)):
            ran += _hand_case(C, S, c, all_one, k)
            k += 1
        for kind in ("Km1", "S"):
            ran += _hand_case(C, S, 0.37, 0, k, kind)
            k += 1
    assert ran >= 4


def test_select_kept_draws_nothing_over_many_blocks(cuda):
    """c = 2^-16 over 150 000 candidates, no seeds: the kept pass's 150 blocks hold almost only zero counts (tag 1, value 0)."""
    C, V = 150000, 300007
    cand, p, sd, seeds = R.hand_list(C, V, 0, seed=9)
    want = R.want_select(cand, p, sd, C, 2.0 ** -16, 0, SEED, 1, 2, seeds, 0, 4096, C + 3000, V, 3, 1)
    assert 0 < want["K"] < 300 and want["err"] == 0
    got = run_select(_d(R.padded(cand, C + 3000 + TAIL, -7)), _d(R.padded(p, C + 3000 + TAIL, 0).to(torch.int16)),
                     _d(R.padded(sd, C + 3000 + TAIL, 0)), _d(_rec_words(C, 2.0 ** -16, 0)), V, C + 3000, 4096, seeds, 0, 1, 2, n_local=3)
    _same(got, want)


# ------------------------------------------------------------------------------------------------------ the alternation contract
def test_twelve_rounds_on_one_scratch_array_equal_fresh_state(cuda):
    """scatter -> candidates -> scale -> select, 12 rounds with a different mark pattern each (the empty one included) on ONE dense
    buffer and ONE scratch array: each pass returns the other's status words, the ticket, the dense buffer and the
    histogram to zero, so every round's outputs equal those of a fresh, zeroed state (the restatement's)."""
    lib = _lib()
    V, cap_c, cap_k = 70 * 1024 + 3, 70 * 1024 + 3, 30000
    scr = Scratch(V, cap_c)
    dense_d = _d(torch.cat([torch.zeros(2 * V, dtype=torch.int64), torch.full((2 * TAIL,), 0x1111, dtype=torch.int64)]))
    gen = torch.Generator().manual_seed(21)
    for rnd in range(12):
        n_seed, n_t = ((0, 0) if rnd == 4 else (int(torch.randint(1, 400, (1,), generator=gen)), int(torch.randint(1, 40000, (1,), generator=gen))))
        if rnd == 7:
            n_seed, n_t = 0, 900
        if rnd == 9:
            n_seed, n_t = 300, 0
        ids = torch.randperm(V, generator=gen)[: n_seed + n_t].to(torch.int32)
        sums = torch.randint(0, 1 << 44, (n_seed + n_t,), generator=gen)
        seeds_l, tkey = ids[:n_seed], ids[n_seed:].long() | (int(rnd) << 40)          # (the key's high word is not the node id)
        ref = R.scatter(seeds_l, sums[:n_seed], n_seed, tkey, sums[n_seed:], n_t, V)
        err = _err_buf()
        n_loc, n_td = _d(torch.tensor([n_seed], dtype=torch.int32)), _d(torch.tensor([n_t], dtype=torch.int32))
        bufs = [_d(torch.cat([seeds_l, torch.tensor([V + 5], dtype=torch.int32)])), _d(torch.cat([sums[:n_seed], torch.tensor([-1])])),
                _d(torch.cat([tkey, torch.tensor([V + 9])])), _d(torch.cat([sums[n_seed:], torch.tensor([-1])]))]     # (entries behind the counts: never read)
        lib.check(lib.lib.bliss_shard_scatter_partials(bufs[0].data_ptr(), bufs[1].data_ptr(), n_loc.data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                                       n_td.data_ptr(), dense_d.data_ptr(), V, err.data_ptr(), _st()), "bliss_shard_scatter_partials")
        torch.cuda.synchronize()
        assert _read_err(err) == 0
        assert torch.equal(dense_d.cpu()[: 2 * V].view(V, 2), ref["dense"])
        got, s = run_candidates(ref["dense"], 0, cap_c, scr=scr, dense_d=dense_d)
        want = R.want_candidates(ref["dense"], 0, cap_c)
        _same(got, want)
        C = want["C"]
        fanout = max(1, C // 4)
        assert _scale_ok(want["hist"], C, fanout)
        sc, _ = run_scale(s, fanout)
        _same(sc, R.scale(want["hist"], C, fanout))
        seeds = seeds_l.clone()
        w = R.want_select(want["cand_nid"][:C], want["p"][:C], want["is_seed"][:C].to(torch.uint8), C, sc["c"], sc["all_one"], SEED, rnd, rnd % 3,
                          seeds, n_seed, cap_k, cap_c, V, 5, rnd % 2)
        assert w["err"] == 0
        _same(run_select(s["cand"], s["p"], s["is_seed"], s["counts"], V, cap_c, cap_k, seeds, n_seed, rnd, rnd % 3, bump=rnd % 2, scr=scr,
                         seeds_on_device=bool(rnd & 2), flag=bool(rnd & 4)), w)


# ----------------------------------------------------------------------------------------------------- dense and routed twins
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 262144, 262145])
def test_dense_and_routed_twins_agree(cuda, n):
    """bliss_cand_importance / bliss_keyed_select (256-thread grid-stride kernels, at most 1024 workgroups: 262 145 is the second
    trip) give the p, P and keep bits of k_sd_cand / k_sd_keep on the same candidate list, and both equal the restatement."""
    lib = _lib()
    V = n + 11
    dense = R.make_dense(V, "all", 2, seed=500 + n % 1000)
    dense[n:] = 0                                                     # exactly n candidates
    for uniform in (0, 1):
        got, s = run_candidates(dense, uniform, V)
        want = R.want_candidates(dense, uniform, V)
        _same(got, want)
        sums_d = _d(torch.cat([dense[:n, 0], torch.tensor([1 << 44])]))
        p2, err = _bf(n + TAIL, 0x5A5A), _err_buf()
        lib.check(lib.lib.bliss_cand_importance(sums_d.data_ptr(), n, uniform, p2.data_ptr(), err.data_ptr(), _st()), "bliss_cand_importance")
        torch.cuda.synchronize()
        assert _read_err(err) == 0
        _same(dict(p=_bits16(p2)), dict(p=R.padded(want["p"][:n], n + TAIL, 0x5A5A)))
        assert torch.equal(_bits16(p2)[:n], got["p"][:n])
        for c, all_one in ((0.37, 0), (1.0, 1)):
            cand, sd = want["cand_nid"][:n], want["is_seed"][:n].to(torch.uint8)
            seeds = cand[sd.bool()]
            S = int(seeds.numel())
            rec = _d(_rec_words(n, c, all_one))
            step, layer = (1 << 40) + 3, 2
            g = run_select(s["cand"], s["p"], s["is_seed"], rec, V, V, V, seeds, S, step, layer, scr=Scratch(V, V))
            w = R.want_select(cand, want["p"][:n], sd, n, c, all_one, SEED, step, layer, seeds, S, V, V, V, 5, 1)
            _same(g, w)
            P2 = _bf(n + TAIL, 0x6B6B)
            keep = torch.full((n + TAIL,), 0xEE, dtype=torch.uint8, device="cuda:0")
            lib.check(lib.lib.bliss_keyed_select(s["cand"].data_ptr(), s["p"].data_ptr(), s["is_seed"].data_ptr(), n, rec.data_ptr(), SEED, step, layer,
                                                 P2.data_ptr(), keep.data_ptr(), _st()), "bliss_keyed_select")
            torch.cuda.synchronize()
            P_ref, keep_ref = R.inclusion(cand, want["p"][:n], sd, c, all_one, SEED, step, layer)
            _same(dict(P=_bits16(P2), keep=keep.cpu().to(torch.int32)),
                  dict(P=R.padded(P_ref, n + TAIL, 0x6B6B), keep=R.padded(keep_ref.to(torch.int32), n + TAIL, 0xEE)))
            assert torch.equal(_bits16(P2)[:n], g["P"][:n])
            new = (keep.cpu()[:n] != 0) & ~sd.bool()                 # the routed draw's new nodes = the dense kept list behind its seeds
            assert torch.equal(cand[new], g["kept_nid"][S: g["K"]])


# ------------------------------------------------------------------------------------------------------ bliss_shard_local_seeds
@pytest.mark.parametrize("S", [0, 1, 1023, 1024, 1025, 3000])
def test_local_seeds(cuda, S):
    """[lo, hi) owning none, all and a middle range with seeds on lo, hi - 1 and hi; the count on the host and on the device; a device
    count above cap_s (error bit, clamp); the copy pointer null or given; padding ids and positions."""
    lib = _lib()
    gen = torch.Generator().manual_seed(60 + S)
    seeds = torch.randperm(50000, generator=gen)[: S + 40].to(torch.int32)
    lo, hi = 20000, 30000
    if S >= 3:
        seeds[S // 2], seeds[S // 3], seeds[S - 1] = lo, hi - 1, hi
    k = 0
    for a, b in ((60000, 70000), (0, 50000), (lo, hi)):
        for cap_s, n_seen, on_dev in ((S + 7, S, False), (S + 7, S, True), (max(S, 1), S, True), (max(S - 5, 1), S, True), (S + 7, S + 7 + 33, True)):
            if n_seen > seeds.numel():
                continue
            want = R.local_seeds(seeds, n_seen, a, b, cap_s)
            assert want["err"] == (R.ERR_CAP_SEEDS if n_seen > cap_s else 0)
            seeds_d = _d(seeds)
            out = {n: torch.full((cap_s + TAIL,), -4, dtype=torch.int32, device="cuda:0") for n in ("seeds_l", "copy", "seed_pos")}
            n_local, n_dev, err = _d(torch.tensor([GARBAGE, -1], dtype=torch.int32)), _d(torch.tensor([n_seen], dtype=torch.int32)), _err_buf()
            with_copy = k % 2 == 0
            k += 1
            lib.check(lib.lib.bliss_shard_local_seeds(seeds_d.data_ptr(), -1 if on_dev else n_seen, n_dev.data_ptr() if on_dev else 0, a, b, cap_s,
                                                      out["seeds_l"].data_ptr(), out["copy"].data_ptr() if with_copy else 0, out["seed_pos"].data_ptr(),
                                                      n_local.data_ptr(), err.data_ptr(), _st()), "bliss_shard_local_seeds")
            torch.cuda.synchronize()
            nl = want["n_local"]
            _same(dict(seeds_l=out["seeds_l"].cpu(), seed_pos=out["seed_pos"].cpu(), copy=out["copy"].cpu(), n_local=int(n_local[0]), err=_read_err(err)),
                  dict(seeds_l=R.padded(want["seeds_l"], cap_s + TAIL, -4), seed_pos=R.padded(want["seed_pos"], cap_s + TAIL, -4),
                       copy=R.padded(want["seeds_l_copy"] if with_copy else want["seeds_l"][:0], cap_s + TAIL, -4), n_local=nl, err=want["err"]))
            assert int(n_local[1]) == -1 and torch.equal(seeds_d.cpu(), seeds)


# ------------------------------------------------------------------------------------------------- bliss_shard_scatter_partials
def _run_scatter(seeds_l, seed_p2, n_local, tkey, tsum, n_t, V, dense0):
    lib = _lib()
    dense_d = _d(torch.cat([dense0.flatten(), torch.full((2 * TAIL,), 0x1111, dtype=torch.int64)]))
    err = _err_buf()
    bufs = [_d(torch.cat([seeds_l.to(torch.int32), torch.tensor([3], dtype=torch.int32)])), _d(torch.cat([seed_p2, torch.tensor([-1])])),
            _d(torch.cat([tkey, torch.tensor([4])])), _d(torch.cat([tsum, torch.tensor([-1])]))]
    n_loc, n_td = _d(torch.tensor([n_local], dtype=torch.int32)), _d(torch.tensor([n_t], dtype=torch.int32))
    lib.check(lib.lib.bliss_shard_scatter_partials(bufs[0].data_ptr(), bufs[1].data_ptr(), n_loc.data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                                   n_td.data_ptr(), dense_d.data_ptr(), V, err.data_ptr(), _st()), "bliss_shard_scatter_partials")
    torch.cuda.synchronize()
    d = dense_d.cpu()
    assert d[2 * V:].tolist() == [0x1111] * (2 * TAIL)
    return dict(dense=d[: 2 * V].view(V, 2), err=_read_err(err))


def test_scatter_partials(cuda):
    """Counts of 0 on either list; ids -1 and V among valid ones (error bit 2, the others scattered, nothing else written); 300 000
    touched records on |V| = 400 000 (the grid-stride loop's second trip: 1024 x 256 threads); the 16-byte store leaves the neighbours
    alone -- the buffer starts as a pattern, not as zeros, and every node that is not named keeps it."""
    gen = torch.Generator().manual_seed(31)
    for V, n_local, n_t, bad in ((1, 0, 0, False), (1, 1, 0, False), (1, 0, 1, False), (1025, 0, 300, False), (1025, 200, 0, False),
                                 (4099, 100, 2000, True), (400000, 1000, 300000, False), (400000, 0, 262145, True)):
        ids = torch.randperm(V, generator=gen)[: n_local + n_t]
        sums = torch.randint(0, 1 << 50, (n_local + n_t,), generator=gen)
        seeds_l, touched = ids[:n_local].clone(), ids[n_local:].clone()
        if bad:
            touched[n_t // 2], touched[n_t - 1] = -1, V
            if n_local:
                seeds_l[n_local // 2] = V + 70
        tkey = (touched & 0xFFFFFFFF) | (torch.randint(0, 1 << 20, (n_t,), generator=gen) << 32)       # (high word: not the id)
        dense0 = torch.arange(2 * V, dtype=torch.int64).view(V, 2) * 3 + 1
        want = R.scatter(seeds_l, sums[:n_local], n_local, tkey, sums[n_local:], n_t, V, dense=dense0)
        assert want["err"] == (R.ERR_CAP_CAND if bad else 0)
        _same(_run_scatter(seeds_l, sums[:n_local], n_local, tkey, sums[n_local:], n_t, V, dense0), want)


# ------------------------------------------------------------------------------------------ pack_rows, place_rows, take_rows
def _rows_buf(rows, stride, sentinel=0x7A7A):
    """rows [n, D] of bits -> a device int16 buffer [n, stride] with the sentinel between the rows (and one row of it behind)."""
    n, D = rows.shape
    b = torch.full((n + 1, stride), sentinel, dtype=torch.int32)
    b[:n, :D] = rows
    return _d(b.to(torch.int16))


@pytest.mark.parametrize("D", [2, 130, 256, 602, 1030])
def test_pack_rows(cuda, D):
    """ids on lo, hi - 1, hi, lo - 1; padding rows whose id IS owned; NaN in the table's rows that are not owned by the list; -0.0 in
    owned rows keeps its bits, every unowned row is +0 bits; strides larger than the row on both sides; *n in {0, 1, cap, cap + 5}."""
    lib = _lib()
    rc = R.row_case(D, seed=D)
    cap, lo, hi = rc["cap"], rc["lo"], rc["hi"]
    table = rc["table"].clone()
    used = torch.zeros(hi - lo, dtype=torch.bool)
    mine = (rc["nid"] >= lo) & (rc["nid"] < hi)
    used[(rc["nid"][mine] - lo).long()] = True
    table[~used] = float("nan")
    ts, os_ = D + 6, D + 10
    for n_rows in (0, 1, cap - 6, cap, cap + 5):
        tab_d = _rows_buf(R.bits(table), ts)
        out_d = _rows_buf(torch.full((cap, D), 0x1234, dtype=torch.int32), os_)
        nid_d, n_d = _d(rc["nid"]), _d(torch.tensor([n_rows], dtype=torch.int32))
        lib.check(lib.lib.bliss_shard_pack_rows(nid_d.data_ptr(), n_d.data_ptr(), cap, lo, hi, tab_d.data_ptr(), ts, D, out_d.data_ptr(), os_, _st()),
                  "bliss_shard_pack_rows")
        torch.cuda.synchronize()
        want = torch.full((cap + 1, os_), 0x7A7A, dtype=torch.int32)
        want[:cap, :D] = R.pack_rows(rc["nid"], n_rows, lo, hi, table, D)
        _same(dict(out=_bits16(out_d)), dict(out=want))
        if n_rows >= 1:
            assert int(want[0, 0]) == 0x8000                        # -0.0 of an owned row


@pytest.mark.parametrize("D", [2, 130, 256, 602, 1030])
def test_place_and_take_rows(cuda, D):
    """*n in {0, 1, cap, cap + 5}; rows with -0.0; strides longer than the row on both sides; take: positions at and far past the
    source's rows give a +0 row, n_dev null takes all cap rows, an fp32 source holds the rounding edges of take_rows_f32_values."""
    lib = _lib()
    gen = torch.Generator().manual_seed(70 + D)
    cap_s, n_rows = 24, 61
    ss, os_ = D + 4, D + 8
    src = torch.randn(cap_s, D, generator=gen).bfloat16()
    src[:, 1] = -0.0
    table = torch.randn(n_rows, D, generator=gen).bfloat16()
    table32 = (torch.randn(n_rows, D, generator=gen) * 3)
    vals = R.take_rows_f32_values()
    table32[:, : min(D, vals.numel())] = vals[: min(D, vals.numel())]
    table32[5] = vals.repeat(D // vals.numel() + 1)[:D]
    table32[0] = table32[5]                                           # (padding positions point at row 0)
    for n in (0, 1, cap_s, cap_s + 5):
        m = min(n, cap_s)
        pos = torch.zeros(cap_s, dtype=torch.int32)
        pos[:m] = torch.sort(torch.randperm(n_rows, generator=gen)[:m]).values.to(torch.int32)
        if m:
            pos[0] = 5 if m == 1 else min(int(pos[0]), 5)
        pos_d, n_d = _d(pos), _d(torch.tensor([n], dtype=torch.int32))
        out_d = _rows_buf(torch.full((n_rows, D), 0x1234, dtype=torch.int32), os_)
        src_d = _rows_buf(R.bits(src), ss)
        lib.check(lib.lib.bliss_shard_place_rows(src_d.data_ptr(), ss, pos_d.data_ptr(), n_d.data_ptr(), cap_s, out_d.data_ptr(), os_, n_rows, D, _st()),
                  "bliss_shard_place_rows")
        torch.cuda.synchronize()
        want = torch.full((n_rows + 1, os_), 0x7A7A, dtype=torch.int32)
        want[:n_rows, :D] = R.place_rows(src, pos, n, cap_s, n_rows, D)
        _same(dict(out=_bits16(out_d)), dict(out=want))
        # take: pos beyond the source's rows gives a zero row; n_dev null takes all cap_s rows
        tpos = pos.clone()
        if m > 2:
            tpos[1], tpos[2] = n_rows, n_rows + 1000
        tpos_d = _d(tpos)
        for f32 in (0, 1):
            for null_n in (False, True):
                if f32:
                    buf = torch.full((n_rows + 1, ss), 7.0, dtype=torch.float32)
                    buf[:n_rows, :D] = table32
                    tab_d, tab = _d(buf), table32
                else:
                    tab_d, tab = _rows_buf(R.bits(table), ss), table
                out_d = _rows_buf(torch.full((cap_s, D), 0x1234, dtype=torch.int32), os_)
                lib.check(lib.lib.bliss_shard_take_rows(tab_d.data_ptr(), f32, ss, n_rows, tpos_d.data_ptr(), 0 if null_n else n_d.data_ptr(), cap_s,
                                                        out_d.data_ptr(), os_, D, _st()), "bliss_shard_take_rows")
                torch.cuda.synchronize()
                want = torch.full((cap_s + 1, os_), 0x7A7A, dtype=torch.int32)
                want[:cap_s, :D] = R.take_rows(tab, tpos, None if null_n else n, cap_s, D)
                _same(dict(out=_bits16(out_d)), dict(out=want))
