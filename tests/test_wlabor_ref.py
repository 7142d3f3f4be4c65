"""CPU suite: the restatement of the weighted device-side LABOR sampler's rule (tests/wlabor_ref.py) -- the
integer weights and the scale against Python-integer brute force, the sum bounds and whole columns on a lognormal graph, uniform
probabilities against LABOR-0's threshold, the shared per-source variate, the strict comparison, the inclusion statistics of the
two columns of sections 12 and 17, and EXP3 mode's q against the oracle bit for bit."""
import functools
import math
import struct

import numpy as np
import pytest
import torch

import labor_ref
import wlabor_ref as ref
from oracle import bliss_oracle as bo
from test_labor_is_ref import lognormal_graph
from test_labor_ref import column_graph, hash32

SEED = 1234
ONE = ref.ONE


# ------------------------------------------------------------------------------------------------- brute force, Python ints only
def bf16_bits_of(x):
    """bf16 bits of a Python float that is a bf16 value."""
    return struct.unpack("<I", struct.pack("<f", x))[0] >> 16


def brute_weights(bits):
    valid, me = [], []
    for b in bits:
        E, M = (b >> 7) & 0xFF, b & 0x7F
        ok = not (b & 0x8000) and E != 0xFF and (E or M)
        valid.append(bool(ok))
        me.append((128 + M if E else M, max(E, 1)))
    if not any(valid):
        return [0] * len(bits), 0
    e_max = max(e for (m, e), v in zip(me, valid) if v)
    a = []
    for (m, e), v in zip(me, valid):
        sh = e_max - e
        a.append((m << 24) >> sh if v and sh < 32 else 0)
    return a, e_max


def total(c, a):
    return sum(min(ONE - 1, (c * x) >> 24) for x in a)


def brute_scale(a, f):
    lim, c = f << 32, 0
    for bit in range(31, -1, -1):
        t = c | (1 << bit)
        if total(t, a) <= lim:
            c = t
    return c


def random_q(n, seed=2, bad=True):
    """bf16 probabilities (fp32 values) over nine octaves, with zeros, a NaN, an infinity, a negative and a subnormal entry."""
    rng = np.random.default_rng(seed)
    q = ref.wneighbor_ref.rbf(np.exp2(rng.uniform(-6, 3, n)).astype(np.float32))
    if bad:
        q[rng.permutation(n)[:n // 9]] = 0.0
        q[5], q[11], q[17], q[23] = np.nan, -2.0, np.inf, 2.0 ** -130
    return q


# ------------------------------------------------------------------------------------------------- the rule
def test_integer_weights_and_scale_are_the_brute_force():
    rng = np.random.default_rng(4)
    cases = [([1.0] * 7, 3), ([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], 3), ([1, 1, 2, 4, 0.5, 0.25, 8, 1], 2),
             ([0.0] * 5, 2),                                                     # no valid edge: nothing can be kept
             ([1000.0, 1.0, 1.0, 1.0, 1.0], 2),                                  # one dominant edge: clamped at ONE - 1
             ([1.0, 2.0 ** -40, 2.0 ** -30, 2.0 ** -31, 3.0], 2),                # shifts of 31, 32 and more: a_pos = 1, 0, 0
             ([float("nan"), -1.0, float("inf"), 2.0 ** -130, 2.0 ** -133, 1.0, 0.5, -0.0], 2),
             ([2.0 ** -133, 2.0 ** -132, 2.0 ** -127, 2.0 ** -126], 1)]          # subnormals only: E = 0 counts as e = 1
    for _ in range(24):
        d = int(rng.integers(2, 13))
        cases.append((random_q(d, seed=int(rng.integers(1 << 30)), bad=False).tolist(), int(rng.integers(1, d))))
    sat = 0
    for q, f in cases:
        bits = ref.q_bits(np.array(q, dtype=np.float32))
        assert bits.tolist() == [bf16_bits_of(x) if x == x else 0x7FC0 for x in q]
        a, e_max = ref.column_weights(bits)
        ba, be = brute_weights(bits.tolist())
        assert a.tolist() == ba and e_max == be and all(x < ONE for x in ba), (q, f)
        c = ref.scale(a, f)
        assert c == brute_scale(ba, f), (q, f)
        p = ref.probs(c, a).tolist()
        assert p == [min(ONE - 1, (c * x) >> 24) for x in ba]
        assert all(x < ONE for x in p) and sum(p) <= f << 32
        if c < ONE - 1:
            assert total(c + 1, ba) > f << 32 and sum(p) > (f << 32) - 256 * len(p)
        sat += c == ONE - 1
    assert sat >= 3
    a, _ = ref.column_weights(ref.q_bits(np.array([1000.0, 1.0, 1.0, 1.0, 1.0], dtype=np.float32)))
    p = ref.probs(ref.scale(a, 2), a).tolist()
    assert p[0] == ONE - 1 and len(set(p[1:])) == 1 and (1 << 30) - 256 < p[1] <= 1 << 30       # the other four share the rest
    a, _ = ref.column_weights(ref.q_bits(np.array([0.0] * 5, dtype=np.float32)))
    assert ref.scale(a, 2) == ONE - 1 and ref.probs(ONE - 1, a).tolist() == [0] * 5
    a, e_max = ref.column_weights(ref.q_bits(np.array([1.0, 2.0 ** -40, 2.0 ** -30, 2.0 ** -31, 3.0], dtype=np.float32)))
    assert e_max == 128 and a.tolist() == [128 << 23, 0, 1, 0, 192 << 24]


@pytest.mark.parametrize("fanout", [1, 3, 10])
def test_sum_bounds_hold_for_every_column(fanout):
    indptr, indices, seeds = lognormal_graph()
    E = int(indptr[-1])
    w = ref.wneighbor_ref.rbf(np.exp2(np.random.default_rng(3).uniform(-8, 4, E)).astype(np.float32))
    seen = 0
    for q_pos in (random_q(E), ref.exp3_q_pos(indptr, seeds, w, 0.4)):
        lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 0, 0, q_pos)
        o = 0
        for s, c, wh in zip(seeds, lay["c"], lay["whole"]):
            d = int(indptr[s + 1] - indptr[s])
            p = [int(x) for x in lay["p"][o:o + d]]
            o += d
            if d <= fanout:
                assert wh and c == 0 and all(x == ONE for x in p)
                continue
            assert not wh and all(x < ONE for x in p) and sum(p) <= fanout << 32
            if c < ONE - 1:
                assert sum(p) > (fanout << 32) - 256 * d
            seen += 1
        assert o == lay["E"]
        whole = lay["p_e"] == np.uint64(ONE)
        assert bool((lay["edge_weights"][whole] == 1.0).all()) and bool((lay["p_ij"][whole] == 0x3F80).all())
        assert np.array_equal(lay["q_ij"], ref.q_bits(q_pos)[lay["pos"]])         # q_ij also in whole columns
        assert bool((lay["p_e"] >= 1).all())                                     # an edge with p = 0 is never kept
    assert seen > 60


@pytest.mark.parametrize("value", [1.0, 0.37109375, 255.0, 2.0 ** -130])
def test_uniform_probabilities_are_labor_0_up_to_256(value):
    indptr, indices, seeds = lognormal_graph()
    q_pos = np.full(int(indptr[-1]), value, dtype=np.float32)
    assert np.array_equal(ref.wneighbor_ref.rbf(q_pos), q_pos)
    for fanout in (1, 3, 10):
        lay = ref.sample_layer(indptr, indices, None, seeds, fanout, SEED, 2, 1, q_pos)
        o = 0
        for s in seeds:
            d = int(indptr[s + 1] - indptr[s])
            p = lay["p"][o:o + d]
            o += d
            if d > fanout:
                thr = labor_ref.threshold(fanout, d)
                assert len(set(p.tolist())) == 1 and thr - 256 < int(p[0]) <= thr
        kept = lay["p_e"] != np.uint64(ONE)
        assert bool((ref.bf16_of_f64(lay["edge_weights"][kept]) == 0x3F80).all())  # equal probabilities: unit weights as bf16


def test_equal_weight_columns_keep_a_shared_source_in_all_or_in_none():
    shared = [20, 21, 22, 23, 24, 25]
    cols = [shared + [30, 31], shared + [40, 41], [50, 51] + shared]              # three columns of degree 8 over six shared sources
    wide = shared + list(range(60, 70))                                          # degree 16: the smaller threshold
    indptr, indices = column_graph(*cols, wide, n=70)
    q_pos = np.full(len(indices), 0.75, dtype=np.float32)
    both = set()
    for t in range(64):
        lay = ref.sample_layer(indptr, indices, None, [0, 1, 2, 3], 3, SEED, t, 0, q_pos)
        src = lambda s: set(indices[lay["pos"][lay["dst"] == s]].tolist()) & set(shared)
        assert src(0) == src(1) == src(2)
        assert src(3) <= src(0)                                                  # nested: one variate per source, LABOR's property
        both.add((len(src(0)) > 0, len(src(0)) < 6))
    assert (True, True) in both


def test_the_comparison_is_strict_and_p_zero_is_never_kept():
    indptr, indices = column_graph([10, 11, 12, 13, 14, 15, 16, 17], n=18)
    q_pos = np.array([1, 2, 3, 4, 5, 6, 7, 0], dtype=np.float32)
    p = [int(x) for x in ref.sample_layer(indptr, indices, None, [0], 3, SEED, 0, 0, q_pos)["p"]]
    assert p[7] == 0 and all(0 < x < ONE - 1 for x in p[:7])
    ov = np.full(18, 0xFFFFFFFF, dtype=np.uint32)
    ov[11], ov[14], ov[16], ov[17] = p[1] - 1, p[4], 0, 0
    lay = ref.sample_layer(indptr, indices, None, [0], 3, SEED, 0, 0, q_pos, keys_override=ov)
    assert lay["pos"].tolist() == [1, 6]                                          # p - 1 kept, p dropped, 0 kept, 0 against p = 0 dropped
    assert lay["p_e"].tolist() == [p[1], p[6]]
    inv = [ONE / p[1], ONE / p[6]]
    assert np.allclose(lay["edge_weights"], [x * 2 / sum(inv) for x in inv], rtol=1e-14, atol=0)
    assert lay["p_ij"].tolist() == ref.bf16_of_p([p[1], p[6]]).tolist() and lay["q_ij"].tolist() == [0x4000, 0x40E0]
    # the draw is the hash of the SOURCE: the same loop in Python integers
    lay = ref.sample_layer(indptr, indices, None, [0], 3, SEED, 5, 2, q_pos)
    assert lay["pos"].tolist() == [i for i in range(8) if hash32(SEED, 5, 2, 10 + i) < p[i]]


def test_layers_chain_and_layer_dependency():
    indptr, indices, seeds = lognormal_graph()
    q_pos = random_q(int(indptr[-1]))
    for dep in (False, True):
        lays = ref.sample_blocks(indptr, indices, None, seeds[:9], [3, 2], SEED, 4, [q_pos, q_pos], layer_dependency=dep)
        assert np.array_equal(lays[1]["kept_nid"][:lays[0]["K"]], lays[0]["kept_nid"])
        want = ref.sample_layer(indptr, indices, None, lays[0]["kept_nid"], 2, SEED, 4, 0 if dep else 1, q_pos)
        assert np.array_equal(lays[1]["pos"], want["pos"])


# ------------------------------------------------------------------------------------------------- statistics
STAT_Q = ([1, 2, 3, 4, 5, 6, 7, 8], [1, 1, 2, 4, 0.5, 0.25, 8, 1])
STAT_F = (3, 2)
STAT_LAYER, STAT_STEPS = 1, 2048


def stat_graph():
    """Two seed columns (nodes 0 and 1, fanouts 3 and 2) of eight sources each; 64 nodes."""
    indptr, indices = column_graph(list(range(10, 18)), list(range(20, 28)), n=64)
    return indptr, indices, np.array(STAT_Q[0] + STAT_Q[1], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def inclusion_counts():
    """How often every edge of the two columns is kept over draw steps 0 .. 2047, and its probability."""
    indptr, indices, q_pos = stat_graph()
    hits, ps = [], []
    for s, f in enumerate(STAT_F):
        a, b = int(indptr[s]), int(indptr[s + 1])
        p = ref.sample_layer(indptr, indices, None, [s], f, SEED, 0, STAT_LAYER, q_pos)["p"]
        h = np.zeros(b - a, dtype=np.int64)
        for t in range(STAT_STEPS):
            key = ref.keys(SEED, t, STAT_LAYER, indices[a:b]).astype(np.uint64)
            h += key < p
            if t % 256 == 0:                                                      # (the short cut is the restatement's own draw)
                lay = ref.sample_layer(indptr, indices, None, [s], f, SEED, t, STAT_LAYER, q_pos)
                assert np.array_equal(lay["pos"], a + np.nonzero(key < p)[0]) and np.array_equal(lay["p"], p)
        hits.append(h)
        ps.append(p)
    return hits, ps


def check_inclusion(hits, p):
    """5 sigma of the binomial around n * p / ONE, per edge (the bound of sections 12 and 17).  Returns the largest deviation."""
    worst = 0.0
    for j, (h, pj) in enumerate(zip(hits.tolist(), p.tolist())):
        pr = pj / ONE
        mean, sigma = STAT_STEPS * pr, math.sqrt(STAT_STEPS * pr * (1.0 - pr))
        print("edge %2d: p = %.4f, kept %4d times, mean %6.1f, deviation %+.2f sigma" % (j, pr, h, mean, (h - mean) / sigma))
        assert abs(h - mean) <= 5.0 * sigma, (j, h, mean, sigma)
        worst = max(worst, abs(h - mean) / sigma)
    return worst


def test_inclusion_frequencies():                                                 # (largest deviations: see DESIGN.md section 19)
    hits, ps = inclusion_counts()
    for h, p, q, f in zip(hits, ps, STAT_Q, STAT_F):
        assert int(p.sum()) <= f << 32 and int(p.sum()) > (f << 32) - 256 * 8
        ideal = np.array(q, dtype=np.float64) * f / sum(q)
        assert np.allclose(p.astype(np.float64) / ONE, ideal, rtol=0, atol=2.0 ** -20)   # proportional to q: no clamp is met here
        print("column q = %s, fanout %d: largest deviation %.2f sigma" % (q, f, check_inclusion(h, p)))


# ------------------------------------------------------------------------------------------------- EXP3 mode
@pytest.mark.parametrize("eta", [0.1, 0.4])
def test_exp3_q_is_the_oracles_bit_for_bit(eta):
    indptr, indices, seeds = lognormal_graph()
    E = int(indptr[-1])
    w = ref.wneighbor_ref.rbf(np.exp2(np.random.default_rng(3).uniform(-8, 4, E)).astype(np.float32))
    q_pos = ref.exp3_q_pos(indptr, seeds, w, eta)
    g = bo.CSC(torch.from_numpy(indptr), torch.from_numpy(indices.astype(np.int32)))
    fr = bo.expand_frontier(g, torch.from_numpy(seeds))
    want, _ = bo.exp3_edge_prob(g, fr, torch.from_numpy(w).bfloat16(), eta)
    lay = ref.sample_layer(indptr, indices, None, seeds, -1, SEED, 0, 0, q_pos)      # every frontier edge kept: q_ij of all of them
    assert np.array_equal(lay["pos"], fr.pos.numpy())
    assert np.array_equal(lay["q_ij"], want.view(torch.int16).numpy().view(np.uint16))
    lay = ref.sample_layer(indptr, indices, None, seeds, 3, SEED, 0, 0, q_pos)
    by_pos = dict(zip(fr.pos.numpy().tolist(), want.view(torch.int16).numpy().view(np.uint16).tolist()))
    assert lay["q_ij"].tolist() == [by_pos[int(x)] for x in lay["pos"]] and 0 < lay["B"] < lay["E"]
