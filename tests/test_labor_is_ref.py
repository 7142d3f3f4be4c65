"""CPU suite: the restatement of the device-side LABOR-i sampler's rule (tests/labor_is_ref.py) -- 0 iterations against the LABOR-0
restatement, the scale against a brute-force downward search, the two sum bounds, the iteration against a brute-force maximum,
the strict comparison, multi-edges, the shrinking importance mass, six planted faults, and the inclusion statistics of one layer."""
import functools
import math

import numpy as np
import pytest

import labor_is_ref as ref
import labor_ref
from test_labor_ref import brute_layer as brute_layer0, column_graph, hash32, same, toy_graph

SEED = 1234
ONE = ref.ONE


# ------------------------------------------------------------------------------------------------- brute force, Python ints only
def total(c, pis, ceil=False):
    return sum(-((-c * p) >> 32) if ceil else (c * p) >> 32 for p in pis)


def brute_scale(pis, f, fault=None):
    """32 bisection steps in Python integers.  ``fault``: 'strict' accepts a step only below the bound, 'ceil' rounds p up."""
    lim, c = f << 32, 0
    for bit in range(31, -1, -1):
        t = c | (1 << bit)
        s = total(t, pis, ceil=fault == "ceil")
        if s < lim or (s == lim and fault != "strict"):
            c = t
    return c


def downward_scale(pis, f):
    """The largest c in [0, ONE - 1] with the sum <= f * ONE, searched DOWNWARD one by one from a proven upper bound:
    sum_pos (c * pi) >> 32 > c * sum(pi) / ONE - d, so every c > (f * ONE + d) * ONE / sum(pi) is over the bound."""
    lim, d = f << 32, len(pis)
    c = min(ONE - 1, ((lim + d) << 32) // sum(pis) + 1)
    assert c == ONE - 1 or total(c + 1, pis) > lim
    steps = 0
    while total(c, pis) > lim:
        c -= 1
        steps += 1
        assert steps < 1 << 16
    return c


def brute_importances(indptr, indices, seeds, f, iterations, fault=None, pi0=None):
    """Rule 1 to 3 as loops over edges; pi as a dict over the frontier.  ``pi0``: the starting importances (the 'carried' fault)."""
    cols = [[int(u) for u in indices[int(indptr[s]):int(indptr[s + 1])]] for s in seeds]
    whole = [f < 0 or len(c) <= f for c in cols]
    pi = {u: ONE for c in cols for u in c}
    if pi0:
        pi.update({u: v for u, v in pi0.items() if u in pi})
    sfault = fault if fault in ("strict", "ceil") else None
    scales = lambda: [None if w else brute_scale([pi[u] for u in c], f, sfault) for c, w in zip(cols, whole)]
    cs = scales()
    for _ in range(iterations):
        new = {}
        for c, w, sc in zip(cols, whole, cs):
            for u in c:
                if w and fault == "whole_not_one":
                    continue
                P = ONE if w else ((-((-sc * pi[u]) >> 32)) if fault == "ceil" else (sc * pi[u]) >> 32)
                new[u] = max(new.get(u, 0), P)
        pi = {u: max(1, new.get(u, 0), pi[u] if fault == "max_with_old" else 0) for u in pi}
        cs = scales()
    return pi, cs, cols, whole


def brute_layer(indptr, indices, seeds, f, seed, step, layer, iterations, ov=None, fault=None, pi0=None):
    seeds = [int(s) for s in seeds]
    pi, cs, cols, whole = brute_importances(indptr, indices, seeds, f, iterations, fault, pi0)
    b_indptr, pos, dst, ps, w = [0], [], [], [], []
    for s, (nid, c, wh, sc) in enumerate(zip(seeds, cols, whole, cs)):
        a, kept = int(indptr[nid]), []
        for i, u in enumerate(c):
            p = ONE if wh else ((-((-sc * pi[u]) >> 32)) if fault == "ceil" else (sc * pi[u]) >> 32)
            ps.append(p)
            if wh or (hash32(seed, step, layer, u) if ov is None else int(ov[u])) < p:
                kept.append((a + i, p))
        tot = 0.0
        for _, p in kept:
            tot += float(ONE) / float(p)
        for q, p in kept:
            pos.append(q)
            dst.append(s)
            w.append(1.0 if wh else float(ONE) / float(p) * (1.0 if fault == "no_ks" else float(len(kept))) / tot)
        b_indptr.append(len(pos))
    srcs = [int(indices[q]) for q in pos]
    new = sorted(set(srcs) - set(seeds))
    kept_nid = seeds + new
    local = {v: i for i, v in enumerate(kept_nid)}
    return dict(indptr=b_indptr, pos=pos, dst=dst, src=[local[u] for u in srcs], kept_nid=kept_nid, p=ps, edge_weights=w, pi=pi,
                c=[0 if x is None else x for x in cs])


def brute_blocks(indptr, indices, seeds, fanouts, seed, step, iterations, fault=None):
    out, pi0 = [], None
    for n, f in enumerate(fanouts):
        lay = brute_layer(indptr, indices, seeds, f, seed, step, n, iterations, fault=fault, pi0=pi0)
        out.append(lay)
        seeds = lay["kept_nid"]
        pi0 = lay["pi"] if fault == "carried" else None
    return out


def same_is(lay, brute):
    return (same(lay, brute) and np.array_equal(lay["p"], np.array(brute["p"], dtype=np.uint64))
            and np.array_equal(lay["c"], np.array(brute["c"], dtype=np.uint64))
            and np.array_equal(lay["edge_weights"], np.array(brute["edge_weights"], dtype=np.float64)))


def lognormal_graph(n=400, seed=7):
    rng = np.random.default_rng(seed)
    deg = np.minimum(np.round(rng.lognormal(2.5, 1.0, n)).astype(np.int64), n - 1)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    indices = np.concatenate([rng.choice(n, int(d), replace=False) for d in deg]).astype(np.int64)
    return indptr, indices, rng.permutation(n)[:64]


# ------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("fanout", [-1, 1, 3, 10])
def test_zero_iterations_is_labor_0(fanout):
    indptr, indices = toy_graph()
    seeds = np.random.default_rng(1).permutation(60)[:25]
    eid = np.random.default_rng(2).permutation(int(indptr[-1]))
    for step, layer in ((3, 1), (0, 0)):
        got = ref.sample_layer(indptr, indices, eid, seeds, fanout, SEED, step, layer, 0)
        want = labor_ref.sample_layer(indptr, indices, eid, seeds, fanout, SEED, step, layer)
        for k, v in want.items():
            assert np.array_equal(got[k], v), k
        assert same(got, brute_layer0(indptr, indices, seeds, fanout, SEED, step, layer))
        # equal probabilities inside a column: the weights are 1 up to the fp64 sum's rounding, exactly 1 as bf16
        assert bool((np.abs(got["edge_weights"] - 1.0) < 2.0 ** -44).all()) and bool((got["q_ij"] <= 0x3F80).all())
        assert bool((ref.bf16_of_f64(got["edge_weights"]) == 0x3F80).all())
    for dep in (False, True):
        got = ref.sample_blocks(indptr, indices, eid, seeds[:5], [fanout, 3, fanout], SEED, 9, 0, layer_dependency=dep)
        want = labor_ref.sample_blocks(indptr, indices, eid, seeds[:5], [fanout, 3, fanout], SEED, 9, layer_dependency=dep)
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            for k, v in b.items():
                assert np.array_equal(a[k], v), k
    ov = np.random.default_rng(3).integers(0, 2 ** 32, 60, dtype=np.uint64).astype(np.uint32)
    got = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 0, 0, 0, keys_override=ov)
    want = labor_ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 0, 0, keys_override=ov)
    assert all(np.array_equal(got[k], v) for k, v in want.items())


def test_zero_iterations_on_the_column_graphs():
    wide, narrow = list(range(40, 52)), list(range(40, 46))
    for cols, f in (([[10, 11, 12, 13, 14, 15, 16]], 3), ([list(range(20, 25)), list(range(30, 36))], 5), ([wide, narrow], 3),
                    ([[7, 9, 7, 11, 12, 7, 13, 14]], 3)):
        indptr, indices = column_graph(*cols)
        seeds = list(range(len(cols)))
        for t in range(8):
            got = ref.sample_layer(indptr, indices, None, seeds, f, SEED, t, 1, 0)
            want = labor_ref.sample_layer(indptr, indices, None, seeds, f, SEED, t, 1)
            assert all(np.array_equal(got[k], v) for k, v in want.items())
            for c, (a, b) in zip(got["c"], zip(indptr[:-1], indptr[1:])):
                assert c == (0 if b - a <= f else labor_ref.threshold(f, b - a))


def test_scale_is_the_brute_force_downward_search():
    rng = np.random.default_rng(4)
    cases = [([ONE] * d, f) for d, f in ((2, 1), (7, 3), (8, 3), (12, 10), (12, 1))]
    cases += [([1] * 5, 3), ([1] * 12, 1)]                                       # all tiny: the scale saturates
    cases += [([ONE] + [1] * 6, 3), ([3, ONE, 2, 1], 1), ([ONE] + [5] * 11, 1)]  # one at ONE among tiny ones
    for _ in range(24):
        d = int(rng.integers(2, 13))
        f = int(rng.integers(1, d))
        cases.append(([int(x) for x in rng.integers(1 << 20, ONE + 1, d)], f))
    sat = 0
    for pis, f in cases:
        c = ref.scale(pis, f)
        assert c == downward_scale(pis, f) == brute_scale(pis, f), (pis, f)
        assert 0 <= c <= ONE - 1 and total(c, pis) <= f << 32
        assert all((c * p) >> 32 < ONE for p in pis)                             # no clamp is needed
        if c < ONE - 1:
            assert total(c + 1, pis) > f << 32 and total(c, pis) > (f << 32) - len(pis)
        sat += c == ONE - 1
    assert ref.scale([1] * 5, 3) == ONE - 1 and sat >= 2
    for d, f in ((7, 3), (5000, 3), (12, 10)):
        assert ref.scale([ONE] * d, f) == labor_ref.threshold(f, d)               # pi^(0): LABOR-0's thr


@pytest.mark.parametrize("fanout", [1, 3, 10])
def test_sum_bounds_hold_for_every_column(fanout):
    indptr, indices, seeds = lognormal_graph()
    seen = 0
    for I in range(4):
        lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 0, 0, I)
        o = 0
        for s, c in zip(seeds, lay["c"]):
            d = int(indptr[s + 1] - indptr[s])
            p = [int(x) for x in lay["p"][o:o + d]]
            o += d
            if d <= fanout:
                assert c == 0 and all(x == ONE for x in p)
                continue
            assert all(x < ONE for x in p) and sum(p) <= fanout << 32
            if c < ONE - 1:
                assert sum(p) > (fanout << 32) - d
            seen += 1
        assert o == lay["E"]
    assert seen > 100


def test_iteration_is_the_brute_force_maximum():
    indptr, indices = toy_graph()
    seeds = np.random.default_rng(1).permutation(60)[:25]
    for f in (1, 4, 15, 16):
        for I in (1, 2, 3):
            pi, cs = ref.importances(indptr, indices, seeds, f, I)
            bpi, bcs, _, _ = brute_importances(indptr, indices, seeds, f, I)
            assert all(int(pi[u]) == v for u, v in bpi.items())
            assert [None if c is None else int(c) for c in cs] == bcs
            lay = ref.sample_layer(indptr, indices, None, seeds, f, SEED, 3, 1, I)
            assert same_is(lay, brute_layer(indptr, indices, seeds, f, SEED, 3, 1, I))
    # a source shared by a whole and a non-whole column gets ONE; a source seen by one column only gets that column's P
    whole, wide = [20, 21], [20, 30, 31, 32, 33, 34, 35, 36]
    indptr, indices = column_graph(whole, wide)
    pi, cs = ref.importances(indptr, indices, [0, 1], 3, 1)
    thr = labor_ref.threshold(3, 8)
    assert cs[0] is None and int(pi[20]) == ONE and int(pi[21]) == ONE and all(int(pi[u]) == thr for u in range(30, 37))
    pi2, cs2 = ref.importances(indptr, indices, [0, 1], 3, 2)
    assert int(pi2[20]) == ONE and all(int(pi2[u]) == (cs[1] * thr) >> 32 for u in range(30, 37))
    assert int(pi2[30]) < thr and cs2[1] > cs[1]                                  # (the maximum is over the NEW values only)
    assert int(pi[0]) == ONE                                                     # outside the frontier: never touched


def test_the_comparison_is_strict():
    srcs = [10, 11, 12, 13, 14, 15, 16]
    indptr, indices = column_graph(srcs, [10, 11, 12, 13, 14, 15, 16, 17, 18], n=19)
    lay = ref.sample_layer(indptr, indices, None, [0, 1], 3, SEED, 0, 0, 2)
    p = [int(x) for x in lay["p"]]
    assert len(set(p[:7])) > 1 or p[0] != labor_ref.threshold(3, 7)               # (the iterations did move the probabilities)
    ov = np.full(19, 0xFFFFFFFF, dtype=np.uint32)
    ov[11], ov[14], ov[16] = p[1] - 1, p[4], 0
    lay = ref.sample_layer(indptr, indices, None, [0, 1], 3, SEED, 0, 0, 2, keys_override=ov)
    kept0 = lay["pos"][lay["dst"] == 0].tolist()
    assert kept0 == [1, 6]                                                        # p - 1 kept, p dropped, 0 kept
    assert same_is(lay, brute_layer(indptr, indices, [0, 1], 3, SEED, 0, 0, 2, ov=ov))
    # key 0 against p = 1: planted importances (pi_override), the scale saturates at ONE - 1 and (2 * (ONE - 1)) >> 32 = 1
    indptr, indices = column_graph([5, 6, 7, 8], n=9)
    pi = np.full(9, ONE, dtype=np.uint64)
    pi[5], pi[6], pi[7], pi[8] = 2, 1 << 30, 1 << 30, 1 << 30
    ov = np.full(9, 0xFFFFFFFF, dtype=np.uint32)
    ov[5], ov[6] = 0, 1 << 30
    lay = ref.sample_layer(indptr, indices, None, [0], 1, SEED, 0, 0, 0, keys_override=ov, pi_override=pi)
    assert int(lay["c"][0]) == ONE - 1 and [int(x) for x in lay["p"]] == [1, (1 << 30) - 1] + [(1 << 30) - 1] * 2
    assert lay["pos"].tolist() == [0]                                             # 0 < 1 kept; 2^30 < 2^30 - 1 is not
    ov[5] = 1
    assert ref.sample_layer(indptr, indices, None, [0], 1, SEED, 0, 0, 0, keys_override=ov, pi_override=pi)["B"] == 0


def test_a_multi_edge_is_kept_or_dropped_as_one_and_counts_m_terms():
    srcs = [7, 9, 7, 11, 12, 7, 13, 14]                                           # source 7 three times
    indptr, indices = column_graph(srcs, [7, 20, 21, 22, 23], n=24)
    seen = set()
    for t in range(64):
        lay = ref.sample_layer(indptr, indices, None, [0, 1], 3, SEED, t, 0, 2)
        kept = lay["pos"][lay["dst"] == 0].tolist()
        hit = [q in kept for q in (0, 2, 5)]
        assert all(hit) or not any(hit)
        seen.add(all(hit))
    assert seen == {True, False}
    pi, cs = ref.importances(indptr, indices, [0, 1], 3, 2)
    mult = [int(pi[u]) for u in srcs]
    assert cs[0] == brute_scale(mult, 3) != brute_scale([int(pi[u]) for u in dict.fromkeys(srcs)], 3)
    p = [int(x) for x in lay["p"][:8]]
    assert p[0] == p[2] == p[5] and sum(p) <= 3 << 32 and sum(p) > (3 << 32) - 8


@pytest.mark.parametrize("fanout", [3, 10])
def test_importance_mass_shrinks_with_every_iteration(fanout):
    """sum_u pi^(I)_u / ONE over the frontier = the expected number of distinct sources when every pi_u is reached by some
    column: strictly smaller with every iteration."""
    indptr, indices, seeds = lognormal_graph()
    front = np.unique(np.concatenate([indices[indptr[s]:indptr[s + 1]] for s in seeds]))
    mass = []
    for I in range(4):
        pi, _ = ref.importances(indptr, indices, seeds, fanout, I)
        mass.append(sum(int(x) for x in pi[front]) / ONE)
    print("fanout %d: importance mass over %d frontier vertices %s" % (fanout, len(front), ["%.1f" % m for m in mass]))
    assert mass[0] == len(front) and all(mass[I] < mass[I - 1] for I in (1, 2, 3)), mass


# ------------------------------------------------------------------------------------------------- planted faults
def _fault_case(fault):
    """(graph, seeds or first seeds, fanouts, iterations, ov) on which ``fault`` must show."""
    if fault == "strict":
        indptr, indices = column_graph([10, 11, 12, 13, 14, 15, 16, 17])          # d = 8, fanout 3: 8 c = 3 * ONE is met exactly
        ov = np.full(18, 0xFFFFFFFF, dtype=np.uint32)
        ov[12] = labor_ref.threshold(3, 8) - 1
        return indptr, indices, [0], [3], 0, ov
    if fault == "whole_not_one":
        indptr, indices = column_graph([20, 21], [20, 30, 31, 32, 33, 34, 35, 36])
        return indptr, indices, [0, 1], [3], 1, None
    indptr, indices = toy_graph()
    seeds = np.random.default_rng(1).permutation(60)[:25]
    if fault == "carried":
        return indptr, indices, seeds[:6], [4, 4], 1, None
    return indptr, indices, seeds, [4], 2, None


@pytest.mark.parametrize("fault", ["max_with_old", "strict", "ceil", "whole_not_one", "carried", "no_ks"])
def test_planted_fault_changes_the_output(fault):
    indptr, indices, seeds, fanouts, I, ov = _fault_case(fault)
    if fault == "carried":
        lays = ref.sample_blocks(indptr, indices, None, seeds, fanouts, SEED, 3, I)
        good, bad = brute_blocks(indptr, indices, seeds, fanouts, SEED, 3, I), brute_blocks(indptr, indices, seeds, fanouts, SEED, 3, I, fault)
        assert all(same_is(a, b) for a, b in zip(lays, good))
        assert not all(same_is(a, b) for a, b in zip(lays, bad))
        return
    lay = ref.sample_layer(indptr, indices, None, seeds, fanouts[0], SEED, 3, 0, I, keys_override=ov)
    assert same_is(lay, brute_layer(indptr, indices, seeds, fanouts[0], SEED, 3, 0, I, ov=ov))
    assert not same_is(lay, brute_layer(indptr, indices, seeds, fanouts[0], SEED, 3, 0, I, ov=ov, fault=fault)), fault


# ------------------------------------------------------------------------------------------------- weights
def test_weights_and_inclusion_probabilities():
    indptr, indices, seeds = lognormal_graph()
    lay = ref.sample_layer(indptr, indices, None, seeds, 3, SEED, 5, 0, 2)
    w, q, p = lay["edge_weights"], lay["q_ij"], lay["p_e"]
    assert w.dtype == np.float64 and q.dtype == np.uint16 and len(w) == len(q) == len(p) == lay["B"]
    nonunit = 0
    for s in range(lay["S"]):
        o, e = lay["indptr"][s], lay["indptr"][s + 1]
        k = e - o
        if k == 0:
            continue
        assert abs(w[o:e].sum() - k) <= k * 2.0 ** -40                            # Hajek: the weights of a column sum to its kept count
        if int(p[o]) == ONE:
            assert (w[o:e] == 1.0).all() and (q[o:e] == 0x3F80).all()
        else:
            nonunit += bool((w[o:e] != 1.0).any())
            inv = ONE / p[o:e].astype(np.float64)
            assert np.allclose(w[o:e], inv * k / inv.sum(), rtol=1e-12, atol=0)
    assert nonunit > 10
    # q_ij: two defined roundings.  2^31 + 2^7 is a tie at fp32 (24 bits): to even, down; the bf16 step then rounds 0.5 exactly
    assert ref.bf16_of_p([1 << 31, (1 << 31) + (1 << 7), 1, (1 << 32) - 1, 3 << 29]).tolist() == [0x3F00, 0x3F00, 0x2F80, 0x3F80, 0x3EC0]
    # fp64 -> bf16 in one rounding: 1 + 2^-8 is a tie (to even: 1.0), a hair above it goes up, 1.9999 carries into the exponent
    assert ref.bf16_of_f64([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8, 1.99999, 0.3]).tolist() == \
        [0x3F80, 0x3F80, 0x3F81, 0x3F82, 0x4000, 0x3E9A]


# ------------------------------------------------------------------------------------------------- statistics
STAT_COLS = ([10, 11, 12, 13, 14, 15, 16, 17], [14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25], [10, 11, 12, 20, 21, 22, 23, 24, 25, 26])
STAT_LAYER, STAT_ITERS, STAT_STEPS = 1, 2, 2048


def stat_graph():
    """Three seed columns (nodes 0, 1, 2) that share sources; 64 nodes."""
    return column_graph(*STAT_COLS, n=64)


@functools.lru_cache(maxsize=None)
def inclusion_counts():
    """How often every edge of the layer is kept over draw steps 0 .. 2047 (fanout 3, 2 iterations), and its probability."""
    indptr, indices = stat_graph()
    first = ref.sample_layer(indptr, indices, None, [0, 1, 2], 3, SEED, 0, STAT_LAYER, STAT_ITERS)
    p = first["p"]
    hits = np.zeros(len(indices), dtype=np.int64)
    for t in range(STAT_STEPS):
        key = ref.keys(SEED, t, STAT_LAYER, indices).astype(np.uint64)
        hits += key < p
        if t % 128 == 0:                                                          # (the short cut is the restatement's own draw)
            lay = ref.sample_layer(indptr, indices, None, [0, 1, 2], 3, SEED, t, STAT_LAYER, STAT_ITERS)
            assert np.array_equal(lay["pos"], np.nonzero(key < p)[0]) and np.array_equal(lay["p"], p)
    return hits, p


def check_inclusion(hits, p):
    """5 sigma of the binomial around n * p / ONE, per edge."""
    for j, (h, pj) in enumerate(zip(hits.tolist(), p.tolist())):
        pr = pj / ONE
        mean, sigma = STAT_STEPS * pr, math.sqrt(STAT_STEPS * pr * (1.0 - pr))
        print("edge %2d: p = %.4f, kept %4d times, mean %6.1f, deviation %+.2f sigma" % (j, pr, h, mean, (h - mean) / sigma))
        assert abs(h - mean) <= 5.0 * sigma, (j, h, mean, sigma)


def test_inclusion_frequencies():
    hits, p = inclusion_counts()
    indptr, _ = stat_graph()
    assert len(set(p.tolist())) > 3                                               # (not LABOR-0: the probabilities differ inside a column)
    c = ref.sample_layer(indptr, stat_graph()[1], None, [0, 1, 2], 3, SEED, 0, STAT_LAYER, STAT_ITERS)["c"]
    for a, b, cs in zip(indptr[:3], indptr[1:4], c):
        assert int(p[a:b].sum()) <= 3 << 32 and (int(cs) == ONE - 1 or int(p[a:b].sum()) > (3 << 32) - (b - a))
    check_inclusion(hits, p)
