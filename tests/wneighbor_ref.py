"""CPU restatement of the weighted device-side neighbor draw (csrc/neighbor_w.hip).  NumPy and exact
Python integers / fractions only.

For sampling layer ``layer`` of draw step ``step``, seed column s with CSC positions [a, b), d = b - a, fanout f:
  q_pos    = prob_pos[pos] (raw mode: bf16, unnormalised), or eta / n_i + (1 - eta) * w_pos / sum_col(w) (EXP3 mode, ``exp3_q_pos``:
             the column sum exact, rounded once to bf16; (1 / n) * eta and the product each rounded to bf16)
  u_pos    = ((key32(pos) >> 8) + 1) * 2^-24, key32 = neighbor_ref.keys (seed, step, layer, CSC position); in (0, 1], exact in fp32
  key_pos  = fp32(-log(fp64(u_pos)) / fp64(q_pos)), the sign of zero dropped; +inf unless q_pos > 0 (a NaN q: +inf)
  k        = d if f < 0 or d <= f (a WHOLE column: no key is computed), else f; kept = the k smallest pairs (key bits, pos)
  block    = neighbor_ref's (columns in seed order, ascending position inside a column, the seeds first among the sources, then the
             others in ascending node id); q_ij = q_pos (bf16) for every kept edge; node_prob = 1
  weights  = (1 / q_e) * k_s / sum over the column's kept e' of (1 / q_e') in fp64 from the bf16 q, rounded once to bf16; exactly 1 in
             a whole column and in a column that keeps an edge whose q is not a positive finite number
"""
import math
from fractions import Fraction

import numpy as np

import neighbor_ref as nref

INF_BITS = 0x7F800000


# ------------------------------------------------------------------------------------------------- bf16 as fp32 values
def bf16_bits(x):
    """fp32 -> bf16 bits (uint16), round to nearest even, NaN -> 0x7FC0 (c10::BFloat16)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    r[(u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)] = 0x7FC0
    return r


def from_bits(b):
    return (np.asarray(b).astype(np.uint32) << np.uint32(16)).view(np.float32)


def rbf(x):
    """Round fp32 values to bf16, returned as fp32."""
    return from_bits(bf16_bits(x))


def fraction_to_bf16(fr):
    """An exact non-negative rational -> the nearest bf16 (ties to even), as a Python float.  Subnormals as IEEE."""
    fr = Fraction(fr)
    if fr == 0:
        return 0.0
    e = fr.numerator.bit_length() - fr.denominator.bit_length()        # 2^(e-1) < fr < 2^(e+1)
    if Fraction(2) ** e > fr:
        e -= 1
    unit = Fraction(2) ** (max(e, -126) - 7)                           # spacing of bf16 at fr (2^-133 below the normal range)
    m = fr / unit
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return float(n * unit)


# ------------------------------------------------------------------------------------------------- probabilities and keys
def exp3_q_pos(indptr, seeds, w_pos, eta):
    """EXP3-mode q by CSC position (fp32 values of bf16), NaN outside the seeds' columns.  ``w_pos``: the EXP3 row by position."""
    indptr = np.asarray(indptr, dtype=np.int64)
    w = np.asarray(w_pos, dtype=np.float32)
    q = np.full(w.shape[0], np.nan, dtype=np.float32)
    eta_f, ome_f = np.float32(eta), np.float32(1.0 - eta)
    for s in np.asarray(seeds, dtype=np.int64):
        a, b = int(indptr[s]), int(indptr[s + 1])
        if b == a:
            continue
        wsum = np.float32(fraction_to_bf16(sum((Fraction(float(x)) for x in w[a:b]), Fraction(0))))
        with np.errstate(divide="ignore", invalid="ignore"):
            wd = rbf(w[a:b] / wsum)
        av = rbf(np.array([(np.float32(1.0) / np.float32(b - a)) * eta_f], dtype=np.float32))[0]
        q[a:b] = rbf(av + rbf(ome_f * wd))
    return q


def uniforms(seed, step, layer, pos):
    return ((nref.keys(seed, step, layer, pos) >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)


def race_keys(q, seed, step, layer, pos):
    """uint32 fp32 bit patterns of the race keys of positions ``pos`` with probabilities ``q`` (fp32 values of bf16)."""
    q = np.asarray(q, dtype=np.float32)
    u = uniforms(seed, step, layer, pos)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        key = (-np.log(u.astype(np.float64)) / q.astype(np.float64)).astype(np.float32)
    bits = key.view(np.uint32) & np.uint32(0x7FFFFFFF)
    bits[~(q > 0)] = INF_BITS
    return bits


def frontier_keys(indptr, seeds, fanout, seed, step, layer, q_pos):
    """uint32 [|E|]: the key bits of every position of a NON-WHOLE seed column (what the device's keys_out holds), 0 elsewhere."""
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.zeros(int(indptr[-1]), dtype=np.uint32)
    mask = np.zeros(int(indptr[-1]), dtype=bool)
    for s in np.asarray(seeds, dtype=np.int64):
        a, b = int(indptr[s]), int(indptr[s + 1])
        if fanout < 0 or b - a <= fanout:
            continue
        pos = np.arange(a, b, dtype=np.int64)
        out[a:b] = race_keys(np.asarray(q_pos, dtype=np.float32)[a:b], seed, step, layer, pos)
        mask[a:b] = True
    return out, mask


# ------------------------------------------------------------------------------------------------- the layer
def hajek_weights(q, whole):
    """bf16 weights (as fp32) of one column's kept edges with probabilities ``q`` (fp32 values of bf16)."""
    q = np.asarray(q, dtype=np.float32)
    k = q.shape[0]
    if whole or k == 0 or not bool(((q > 0) & np.isfinite(q)).all()):
        return np.ones(k, dtype=np.float32)
    inv = 1.0 / q.astype(np.float64)
    tot = math.fsum(inv.tolist())
    return np.array([fraction_to_bf16(Fraction(float(x * float(k) / tot))) for x in inv], dtype=np.float32)


def sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, q_pos, keys_override=None):
    """One layer.  ``q_pos``: fp32 values of the bf16 probabilities by CSC position.  ``keys_override``: uint32 key bits by
    position.  Returns neighbor_ref.sample_layer's dict + ``q_ij`` (uint16 bf16 bits), ``weights`` (fp32 values of bf16), ``whole``
    (bool per column)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    q_pos = np.asarray(q_pos, dtype=np.float32)
    if keys_override is None:
        keys_override, _ = frontier_keys(indptr, seeds, fanout, seed, step, layer, q_pos)
    lay = nref.sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, keys_override=keys_override)
    pos = lay["pos"].astype(np.int64)
    q = q_pos[pos]
    lay["q_ij"] = bf16_bits(q)
    sd = np.asarray(seeds, dtype=np.int64)
    deg = indptr[sd + 1] - indptr[sd]
    lay["whole"] = (deg <= fanout) if fanout >= 0 else np.ones(len(sd), dtype=bool)
    w = np.ones(len(pos), dtype=np.float32)
    for s in range(len(sd)):
        o, e = int(lay["indptr"][s]), int(lay["indptr"][s + 1])
        w[o:e] = hajek_weights(q[o:e], bool(lay["whole"][s]))
    lay["weights"] = w
    return lay


def compare(got, want):
    """``got`` against the restatement ``want`` (dicts as sample_layer returns them; ``got['weights']`` fp32 values of bf16):
    every integer array and q_ij equal, the weights within one bf16 ulp, exactly 1 in whole columns, and in every other column
    with positive finite q  |sum_e W_e - k_s| <= k_s * 2^-8.  Raises AssertionError."""
    for name in ("S", "E", "K", "B"):
        assert int(got[name]) == int(want[name]), name
    for name in ("indptr", "pos", "dst", "eid", "src", "kept_nid", "t_indptr", "t_edge", "q_ij"):
        assert np.array_equal(np.asarray(got[name]), np.asarray(want[name])), name
    gw, ww = np.asarray(got["weights"], dtype=np.float32), np.asarray(want["weights"], dtype=np.float32)
    assert gw.shape == ww.shape and bool((gw > 0).all())
    gb, wb = bf16_bits(gw).astype(np.int64), bf16_bits(ww).astype(np.int64)
    assert np.array_equal(from_bits(gb.astype(np.uint16)), gw), "weights are not bf16 values"
    assert int(np.abs(gb - wb).max(initial=0)) <= 1, "a weight is more than one bf16 ulp off"
    q = from_bits(want["q_ij"])
    for s in range(int(want["S"])):
        o, e = int(want["indptr"][s]), int(want["indptr"][s + 1])
        if want["whole"][s] or not bool(((q[o:e] > 0) & np.isfinite(q[o:e])).all()):
            assert bool((gw[o:e] == 1).all()), "unit weights expected in column %d" % s
        else:
            k = e - o
            assert abs(float(gw[o:e].astype(np.float64).sum()) - k) <= k * 2.0 ** -8, "column %d: weights do not sum to k" % s
