"""CPU suite: the restatement of the draws with replacement (tests/replace_ref.py; csrc/replace_draw.hip) --
the draw is a categorical draw with the fixed-point probabilities (pick counts within 5 sigma of the multinomial expectation, the
bound of sections 12, 13 and 17), zero weights are never picked, the fixed-point weights, planted variates, the block's shape."""
import functools

import numpy as np
import pytest

import replace_ref as ref
import wneighbor_ref as wref

SEED = 1234
bits = lambda x: wref.bf16_bits(np.asarray(x, dtype=np.float32))

# name -> (ident, probabilities or None, group size, draws per step)
CASES = {
    "uniform-8": (7, None, 8, 3),
    "uniform-2-of-5": (9, None, 2, 5),                                # d < f
    "weighted-1..8": (7, np.arange(1, 9), 8, 3),
    "weighted-mixed": (107, np.array([1, 1, 2, 4, 0.5, 0.25, 8, 1]), 8, 2),
    "layer-1..8": (ref.LAYER_IDENT, np.arange(1, 9), 8, 3),
}
GPU_WINDOW = ("uniform-8", "weighted-1..8", "layer-1..8")             # the 8-wide cases the GPU tests count over steps 0 .. 2047


def case_probs(name):
    _, q, m, _ = CASES[name]
    if q is None:
        return np.full(m, 1.0 / m)
    w = np.array(ref.fixed_weights(bits(q)), dtype=np.float64)
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def case_counts(name, steps):
    ident, q, m, f = CASES[name]
    w = None if q is None else ref.fixed_weights(bits(q))
    counts = np.zeros(m, dtype=np.int64)
    for step in range(steps):
        for i in ref.picks(ref.variates(SEED, step, 1, ident, f), w, m):
            counts[i] += 1
    return counts


def check_counts(counts, name, steps):
    dev = ref.sigma_deviation(counts, case_probs(name), steps * CASES[name][3])
    print("%s over %d steps: largest deviation %.2f sigma" % (name, steps, dev))
    assert dev <= 5.0, (name, dev)
    return dev


@pytest.mark.parametrize("name", sorted(CASES))
def test_pick_counts_within_five_sigma(name):
    check_counts(case_counts(name, 4096), name, 4096)


@pytest.mark.parametrize("name", GPU_WINDOW)
def test_pick_counts_over_the_gpu_tests_window(name):
    check_counts(case_counts(name, 2048), name, 2048)


def test_two_draws_of_one_column_are_independent():
    """The joint table of draws j = 0, 1 over d = 4 and 8192 steps: every cell within 5 sigma of 1/16."""
    table = np.zeros((4, 4), dtype=np.int64)
    for step in range(8192):
        a, b = ref.picks(ref.variates(SEED, step, 1, 7, 2), None, 4)
        table[a, b] += 1
    dev = ref.sigma_deviation(table.ravel(), np.full(16, 1 / 16), 8192)
    print("joint table: largest cell %.2f sigma" % dev)
    assert dev <= 5.0


def test_variates_do_not_depend_on_the_batch():
    """(seed, step, layer, node id, j) and nothing else: the same column draws the same whatever the other seeds are."""
    ip = np.array([0, 3, 3, 9, 12], dtype=np.int64)
    ix = np.arange(12) % 4
    a = ref.sample_layer(ip, ix, None, [2, 0], 4, SEED, 3, 1)
    b = ref.sample_layer(ip, ix, None, [3, 1, 0, 2], 4, SEED, 3, 1)
    assert a["pos"][0:4].tolist() == b["pos"][8:12].tolist() and a["pos"][4:8].tolist() == b["pos"][4:8].tolist()
    assert ref.variate(ref.group_key(SEED, 3, 1, 2), 0) != ref.variate(ref.group_key(SEED, 3, 1, 2), 1)
    assert ref.group_key(SEED, 3, 1, 2) != ref.group_key(SEED, 4, 1, 2) != ref.group_key(SEED, 4, 2, 2)
    assert ref.fin(0) == 0 and ref.fin(1) == 0x5692161D100B05E5        # SplitMix64's finaliser
    h = ref.group_key(SEED, 3, 1, 2)
    assert ref.variates(SEED, 3, 1, 2, 100) == [ref.variate(h, j) for j in range(100)]   # (the array form of long lists)


def test_bad_values_are_never_picked():
    col = bits([0, 3, np.nan, 1, -2, np.inf, 2, 0])
    w = ref.fixed_weights(col)
    assert w == [0, 3 << 22, 0, 1 << 22, 0, 0, 2 << 22, 0]
    counts = np.zeros(8, dtype=np.int64)
    for step in range(1024):
        for i in ref.picks(ref.variates(SEED, step, 0, 5, 4), w, 8):
            counts[i] += 1
    assert counts[[0, 2, 4, 5, 7]].sum() == 0 and bool((counts[[1, 3, 6]] > 0).all())
    assert ref.sigma_deviation(counts, np.array(w) / sum(w), 4096) <= 5.0


def test_an_all_zero_column_falls_back_to_the_uniform_pick():
    for col in (np.zeros(6), [np.nan, -1, 0, -np.inf, np.inf, -0.0]):
        w = ref.fixed_weights(bits(col))
        assert w == [0] * 6
        rs = ref.variates(SEED, 2, 1, 11, 64)
        assert ref.picks(rs, w, 6) == ref.picks(rs, None, 6) == [(r * 6) >> 64 for r in rs]
    assert len(set(ref.picks(ref.variates(SEED, 2, 1, 11, 64), None, 6))) == 6


def test_fixed_point_weights():
    assert ref.fixed_weights(bits([1, 1.5 * 2.0 ** -16, 2.0 ** -24, 3e38])) == [0, 0, 0, 14811136]
    assert ref.fixed_weights(bits([1, 1.5 * 2.0 ** -16, 2.0 ** -24])) == [1 << 23, 192, 0]     # within 2^-16 of the maximum: exact
    assert ref.fixed_weights(bits([1.5, 2.0 ** -23, 2.0 ** -24])) == [3 << 22, 1, 0]           # the resolution 2^(E - 23)
    sub = np.array([0x0001, 0x0003, 0x0040], dtype=np.uint16)          # bf16 subnormals: 1, 3 and 64 units of 2^-133
    assert ref.fixed_weights(sub) == [1 << 17, 3 << 17, 1 << 23]
    for col in ([5, 3, 0.01], [2.0 ** -100, 2.0 ** -101], [1e30, 7e29]):
        w = ref.fixed_weights(bits(col))
        assert (1 << 23) <= max(w) < (1 << 24)


def test_planted_variates():
    w = ref.fixed_weights(bits([1, 2, 0, 1]))                          # weights 2^22 * [1, 2, 0, 1]... with E = 1: [2^22, 2^23, 0, 2^22]
    assert w == [1 << 22, 1 << 23, 0, 1 << 22]
    W = sum(w)
    assert ref.pick(0, w, 4) == 0 and ref.pick(ref.M64, w, 4) == 3     # r = 0: the first positive entry; r = 2^64 - 1: the last
    assert ref.pick(0, None, 4) == 0 and ref.pick(ref.M64, None, 4) == 3
    assert ref.pick(0, [0, 0, 5, 0], 4) == 2 and ref.pick(ref.M64, [0, 0, 5, 0], 4) == 2
    # t exactly on a prefix boundary: the smallest r with (r * W) >> 64 == prefix picks the NEXT entry, r - 1 still this one
    for prefix, nxt in ((w[0], 1), (w[0] + w[1], 3)):                  # (entry 2 has weight zero: skipped)
        r = -((-prefix << 64) // W)                                     # ceil(prefix * 2^64 / W)
        assert (r * W) >> 64 == prefix and ((r - 1) * W) >> 64 == prefix - 1
        assert ref.pick(r, w, 4) == nxt and ref.pick(r - 1, w, 4) == nxt - (2 if nxt == 3 else 1)
        assert ref.picks([r, r - 1], w, 4) == [ref.pick(r, w, 4), ref.pick(r - 1, w, 4)]


def test_block_invariants():
    rng = np.random.default_rng(5)
    deg = np.array([0, 1, 2, 5, 9, 30] + rng.integers(0, 7, 44).tolist())
    ip = np.zeros(51, dtype=np.int64)
    ip[1:] = np.cumsum(deg)
    ix = rng.integers(0, 50, int(ip[-1]))
    eid = rng.permutation(int(ip[-1]))
    prob = bits(np.exp2(rng.uniform(-4, 4, int(ip[-1]))))
    seeds = [5, 0, 3, 1, 40, 2, 4]
    for f in (1, 3, 7, -1):
        for pb in (None, prob):
            lay = ref.sample_layer(ip, ix, eid, seeds, f, SEED, 2, 1, prob_bits=pb)
            want_k = [int(deg[v]) if f < 0 else (f if deg[v] else 0) for v in seeds]
            assert np.diff(lay["indptr"]).tolist() == want_k and lay["B"] == sum(want_k)   # B is known before the draw
            assert lay["E"] == int(deg[seeds].sum()) and lay["S"] == 7
            for s, v in enumerate(seeds):
                o, e = lay["indptr"][s], lay["indptr"][s + 1]
                p = lay["pos"][o:e]
                assert bool((np.diff(p) >= 0).all()) and bool((p >= ip[v]).all()) and bool((p < ip[v + 1]).all())
                assert np.array_equal(p - ip[v], lay["picks"][o:e]) and bool((lay["dst"][o:e] == s).all())
            assert np.array_equal(lay["eid"], eid[lay["pos"]])
            assert lay["kept_nid"][:7].tolist() == seeds
            new = lay["kept_nid"][7:]
            assert bool((np.diff(new) > 0).all()) and not set(new.tolist()) & set(seeds)
            assert np.array_equal(lay["kept_nid"][lay["src"]], ix[lay["pos"]])
            assert set(new.tolist()) == set(ix[lay["pos"]].tolist()) - set(seeds)
            if pb is not None and f > 0:
                assert np.array_equal(lay["q_ij"], prob[lay["pos"]])
                for s in range(7):
                    o, e = lay["indptr"][s], lay["indptr"][s + 1]
                    if e > o:
                        assert abs(float(lay["weights"][o:e].astype(np.float64).sum()) - (e - o)) <= (e - o) * 2.0 ** -8
            else:
                assert bool((lay["weights"] == 1).all())
    # d = 2 < f = 7: repeats are adjacent, separate edges
    lay = ref.sample_layer(ip, ix, eid, [2], 7, SEED, 0, 0)
    assert lay["B"] == 7 and set(lay["pos"].tolist()) <= {int(ip[2]), int(ip[2]) + 1}
    with pytest.raises(ValueError):
        ref.sample_layer(ip, ix, eid, [2], 1025, SEED, 0, 0)
    with pytest.raises(ValueError):
        ref.sample_layer(ip, ix, eid, [2], 0, SEED, 0, 0)


def test_layer_wise_marks():
    p = bits(np.arange(1, 9))
    pk, drawn = ref.mn_draw(p, 3, SEED, 5, 1)
    assert len(pk) == 3 and drawn.sum() == len(set(pk.tolist())) and bool((drawn[pk] == 1).all())
    pk, drawn = ref.mn_draw(p, 100, SEED, 5, 1)                        # n = min(fanout, C)
    assert len(pk) == 8
    pk, drawn = ref.mn_draw(p, 4, SEED, 5, 1, r_override=[0, ref.M64, 0, ref.M64])
    assert pk.tolist() == [0, 7, 0, 7] and drawn.tolist() == [1, 0, 0, 0, 0, 0, 0, 1]   # duplicates collapse in the marks
    pk, drawn = ref.mn_draw(bits(np.zeros(5)), 3, SEED, 5, 1, r_override=[0, ref.M64, 1 << 63])
    assert pk.tolist() == [0, 4, 2]
