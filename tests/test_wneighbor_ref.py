"""CPU suite: the restatement of the weighted device-side neighbor draw (tests/wneighbor_ref.py) against
brute force, its inclusion statistics against the exact probabilities of successive sampling, its EXP3-mode q against the oracle
bit for bit, its Hajek weights, and planted faults that the comparison helper must catch."""
import copy
import math

import numpy as np
import pytest
import torch

import mn_draw_ref
import wneighbor_ref as ref
from oracle import bliss_oracle as bo
from test_neighbor_ref import small_graph

SEED = 1234
COLUMNS = {"a": (0, [1, 2, 3, 4, 5, 6, 7, 8], 3), "b": (100, [1, 1, 2, 4, 0.5, 0.25, 8, 1], 2)}     # first position, q, fanout


def random_q(n, seed=2):
    """bf16 probabilities (fp32 values) with a few zeros, a NaN and a negative entry."""
    rng = np.random.default_rng(seed)
    q = ref.rbf(np.exp2(rng.uniform(-6, 3, n)).astype(np.float32))
    q[rng.permutation(n)[:n // 9]] = 0.0
    q[5], q[11] = np.nan, -2.0
    return q


def inclusion_counts(which, n_steps, seed=SEED, layer=1):
    """How often every edge of the issue's column ``which`` is kept over draw steps 0 .. n_steps - 1."""
    a, q, f = COLUMNS[which]
    q_pos = np.zeros(a + 8, dtype=np.float32)
    q_pos[a:a + 8] = q
    pos = np.arange(a, a + 8, dtype=np.int64)
    hits = np.zeros(8, dtype=np.int64)
    for t in range(n_steps):
        bits = ref.race_keys(q_pos[a:a + 8], seed, t, layer, pos)
        hits[np.lexsort((pos, bits))[:f]] += 1
    return hits


def check_inclusion(hits, which, n_steps):
    """5 sigma of the binomial around n * pi, pi the exact inclusion probabilities of successive sampling (section 12's bound)."""
    _, q, f = COLUMNS[which]
    pi = mn_draw_ref.inclusion_probabilities(np.array(q, dtype=np.float64), f)
    assert int(hits.sum()) == n_steps * f
    for j in range(8):
        sigma = math.sqrt(n_steps * pi[j] * (1.0 - pi[j]))
        print("column %s edge %d: kept %d times, mean %.1f, deviation %.2f sigma" % (which, j, hits[j], n_steps * pi[j],
                                                                                     (hits[j] - n_steps * pi[j]) / sigma))
        assert abs(hits[j] - n_steps * pi[j]) <= 5.0 * sigma, (which, j, hits[j], n_steps * pi[j], sigma)


def test_uniforms_lie_in_the_half_open_unit_interval_and_keys_are_ordered_bits():
    pos = np.arange(20000, dtype=np.int64)
    u = ref.uniforms(SEED, 3, 1, pos)
    assert u.dtype == np.float32 and float(u.min()) > 0.0 and float(u.max()) <= 1.0
    q = ref.rbf(np.full(20000, 0.37, dtype=np.float32))
    bits = ref.race_keys(q, SEED, 3, 1, pos)
    assert bits.dtype == np.uint32 and int(bits.max()) < ref.INF_BITS
    assert np.array_equal(np.argsort(bits, kind="stable"), np.argsort(bits.view(np.float32), kind="stable"))
    for bad in (0.0, -1.0, np.nan, -np.inf):
        assert int(ref.race_keys(np.array([bad], dtype=np.float32), SEED, 0, 0, np.array([7]))[0]) == ref.INF_BITS
    assert int(ref.race_keys(np.array([np.inf], dtype=np.float32), SEED, 0, 0, np.array([7]))[0]) == 0     # the sign of zero dropped


def test_kept_edges_are_the_brute_force_selection():
    indptr, indices = small_graph()
    E = int(indptr[-1])
    q_pos = random_q(E)
    seeds = np.random.default_rng(1).permutation(60)[:25]
    for fanout in (1, 4, 15, 16, 40, -1):
        lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 3, 1, q_pos)
        for s, nid in enumerate(seeds):
            a, b = int(indptr[nid]), int(indptr[nid + 1])
            got = lay["pos"][lay["indptr"][s]:lay["indptr"][s + 1]].tolist()
            if fanout < 0 or b - a <= fanout:
                assert got == list(range(a, b)) and bool(lay["whole"][s])
                continue
            allp = np.arange(a, b)
            bits = ref.race_keys(q_pos[a:b], SEED, 3, 1, allp)
            brute = sorted(zip(bits.tolist(), allp.tolist()))[:fanout]        # ties go to the lower position
            assert sorted(p for _, p in brute) == got
            n_pos = int((q_pos[a:b] > 0).sum())
            fillers = [p for k, p in brute if k == ref.INF_BITS]
            assert len(fillers) == max(0, fanout - n_pos)                       # +inf keys fill only when positive ones run out
            assert fillers == [p for p in allp.tolist() if not q_pos[p] > 0][:len(fillers)]
        assert np.array_equal(lay["q_ij"], ref.bf16_bits(q_pos[lay["pos"]]))


def test_whole_columns_compute_no_key(monkeypatch):
    indptr, indices = small_graph()
    q_pos = random_q(int(indptr[-1]))
    seeds = np.array([0, 10, 20, 3])
    monkeypatch.setattr(ref, "race_keys", lambda *a, **k: pytest.fail("a key was computed for a whole column"))
    for fanout in (-1, 1000):
        lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 0, 0, q_pos)
        assert lay["B"] == lay["E"] and bool((lay["weights"] == 1).all()) and bool(lay["whole"].all())
        assert np.array_equal(lay["q_ij"], ref.bf16_bits(q_pos[lay["pos"]]))      # q_ij also in whole columns


@pytest.mark.parametrize("which,n_steps", [("a", 4096), ("b", 4096)])         # (largest deviations: 3.27 and 2.20 sigma)
def test_inclusion_frequencies_follow_successive_sampling(which, n_steps):
    hits = inclusion_counts(which, n_steps)
    check_inclusion(hits, which, n_steps)


@pytest.mark.parametrize("eta", [0.1, 0.4])
def test_exp3_q_is_the_oracles_bit_for_bit(eta):
    indptr, indices = small_graph(seed=8, n=80, e=3000)
    E = int(indptr[-1])
    rng = np.random.default_rng(3)
    w = ref.rbf(np.exp2(rng.uniform(-8, 4, E)).astype(np.float32))               # positive bf16 weights in [2^-8, 2^4]
    seeds = np.random.default_rng(4).permutation(80)[:30]
    q = ref.exp3_q_pos(indptr, seeds, w, eta)
    g = bo.CSC(torch.from_numpy(indptr), torch.from_numpy(indices.astype(np.int32)))
    fr = bo.expand_frontier(g, torch.from_numpy(seeds))
    want, _ = bo.exp3_edge_prob(g, fr, torch.from_numpy(w).bfloat16(), eta)
    got = torch.from_numpy(q[fr.pos.numpy()]).bfloat16()
    assert torch.equal(got.float(), torch.from_numpy(q[fr.pos.numpy()]))        # (already bf16 values)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    untouched = np.ones(E, dtype=bool)
    untouched[fr.pos.numpy()] = False
    assert bool(np.isnan(q[untouched]).all())


def test_hajek_weights():
    indptr, indices = small_graph()
    E = int(indptr[-1])
    q_pos = ref.rbf(np.exp2(np.random.default_rng(6).uniform(-6, 3, E)).astype(np.float32))
    seeds = np.arange(60)
    a7, b7 = int(indptr[7]), int(indptr[8])
    assert b7 - a7 > 4
    q_pos[a7:b7] = 0.0                                                          # a degenerate column: fillers only
    lay = ref.sample_layer(indptr, indices, None, seeds, 4, SEED, 2, 0, q_pos)
    n_checked = 0
    for s in range(60):
        o, e = int(lay["indptr"][s]), int(lay["indptr"][s + 1])
        w = lay["weights"][o:e]
        if lay["whole"][s] or s == 7:
            assert bool((w == 1).all())
            continue
        assert e - o == 4 and abs(float(w.astype(np.float64).sum()) - 4) <= 4 * 2.0 ** -8
        q = q_pos[lay["pos"][o:e]].astype(np.float64)
        assert np.allclose(w, (1 / q) * 4 / (1 / q).sum(), rtol=2.0 ** -8)
        n_checked += 1
    assert n_checked > 30
    ref.compare(lay, lay)
    # one rounding from fp64, subnormals as IEEE
    assert ref.fraction_to_bf16(1) == 1.0 and ref.fraction_to_bf16(1 + 2.0 ** -8) == 1.0 and ref.fraction_to_bf16(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6
    assert ref.fraction_to_bf16(2.0 ** -133) == 2.0 ** -133 and ref.fraction_to_bf16(2.0 ** -135) == 0.0


def _case():
    rng = np.random.default_rng(5)
    deg = rng.multinomial(900, np.ones(60) / 60)
    deg[[0, 10, 20, 30]] = [2, 4, 1, 3]                                          # whole columns at fanout 4
    indptr = np.zeros(61, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = rng.integers(0, 60, int(indptr[-1]))
    E = int(indptr[-1])
    q_pos = ref.rbf(np.exp2(np.random.default_rng(6).uniform(-6, 3, E)).astype(np.float32))
    seeds = np.concatenate([[0, 10, 20, 30], np.random.default_rng(1).permutation(np.arange(31, 60))[:21]])
    keys, _ = ref.frontier_keys(indptr, seeds, 4, SEED, 3, 1, q_pos)
    return indptr, indices, seeds, q_pos, keys


def _rebuild(indptr, indices, seeds, q_pos, keys, edit):
    """The restatement's layer with the kept positions of one column edited by ``edit(s, a, b, kept) -> kept`` (sorted)."""
    cols = []
    for s, nid in enumerate(seeds):
        a, b = int(indptr[nid]), int(indptr[nid + 1])
        pos = np.arange(a, b)
        kept = pos if b - a <= 4 else np.sort(pos[np.lexsort((pos, keys[a:b]))[:4]])
        cols.append(np.asarray(edit(s, a, b, kept)))
    # a key array under which exactly these positions win: 0 for the kept ones, 1 for the rest
    ov = np.ones(int(indptr[-1]), dtype=np.uint32)
    ov[np.concatenate(cols)] = 0
    return ref.sample_layer(indptr, indices, None, seeds, 4, SEED, 3, 1, q_pos, keys_override=ov)


def test_planted_faults_fail_the_comparison():
    indptr, indices, seeds, q_pos, keys = _case()
    want = ref.sample_layer(indptr, indices, None, seeds, 4, SEED, 3, 1, q_pos, keys_override=keys)
    ref.compare(_rebuild(indptr, indices, seeds, q_pos, keys, lambda s, a, b, kept: kept), want)     # the unedited rebuild passes
    s0 = next(s for s in range(25) if not want["whole"][s] and indptr[seeds[s] + 1] - indptr[seeds[s]] > 5)

    def swap_for_next_larger(s, a, b, kept):
        if s != s0:
            return kept
        order = np.arange(a, b)[np.lexsort((np.arange(a, b), keys[a:b]))]
        return np.sort(np.concatenate([order[:3], order[4:5]]))                 # the 4th smallest swapped for the 5th
    with pytest.raises(AssertionError):
        ref.compare(_rebuild(indptr, indices, seeds, q_pos, keys, swap_for_next_larger), want)

    # a tie resolved to the higher position
    a0 = int(indptr[seeds[s0]])
    tied = keys.copy()
    order = np.arange(a0, int(indptr[seeds[s0] + 1]))[np.lexsort((np.arange(a0, int(indptr[seeds[s0] + 1])), keys[a0:int(indptr[seeds[s0] + 1])]))]
    tied[order[4]] = tied[order[3]]                                             # the 4th and 5th smallest now tie
    want_t = ref.sample_layer(indptr, indices, None, seeds, 4, SEED, 3, 1, q_pos, keys_override=tied)
    lo, hi = min(order[3], order[4]), max(order[3], order[4])
    assert lo in want_t["pos"] and hi not in want_t["pos"]
    wrong = _rebuild(indptr, indices, seeds, q_pos, tied,
                     lambda s, a, b, kept: kept if s != s0 else np.sort(np.concatenate([order[:3], [hi]])))
    with pytest.raises(AssertionError):
        ref.compare(wrong, want_t)

    # q_ij of a whole column left at 1
    sw = next(s for s in range(25) if want["whole"][s] and want["indptr"][s + 1] > want["indptr"][s])
    bad = copy.deepcopy(want)
    bad["q_ij"][want["indptr"][sw]:want["indptr"][sw + 1]] = 0x3F80
    with pytest.raises(AssertionError):
        ref.compare(bad, want)

    # weights normalised to d instead of k
    bad = copy.deepcopy(want)
    o, e = int(want["indptr"][s0]), int(want["indptr"][s0 + 1])
    d = int(indptr[seeds[s0] + 1] - indptr[seeds[s0]])
    bad["weights"][o:e] = ref.rbf((bad["weights"][o:e] * np.float32(d / 4.0)).astype(np.float32))
    with pytest.raises(AssertionError):
        ref.compare(bad, want)
