"""CPU restatement of the draws WITH replacement (csrc/replace_draw.hip).  NumPy and exact Python integers /
fractions only: there is no floating-point arithmetic in the rule, so every comparison against the device is an equality.

  fin(z)   = the SplitMix64 finaliser of neighbor_ref.keys;  mk = neighbor_ref.mix(seed, step, layer)
  h        = fin(mk ^ (uint64)(uint32)ident): ident = the node id of the seed column (node-wise), 0xFFFFFFFF (layer-wise)
  r_j      = fin(h ^ ((uint64)(j + 1) * 0x9E3779B97F4A7C15)), the variate of draw j = 0, 1, ...
  weights  = over one group of bf16 probabilities: E = floor(log2(largest positive finite value)), w_i = floor(x_i * 2^(23 - E)) for
             a positive finite x_i, else 0; W = sum w_i
  one draw = over a group of m entries: W > 0: t = (r_j * W) >> 64, the smallest i whose inclusive prefix sum exceeds t;
             W == 0 or no probabilities: (r_j * m) >> 64
  node-wise: column s, CSC positions [a, a + d), fanout f: k_s = d if f < 0 (whole, no draw), 0 if d == 0, else f (also when d <= f);
             block edges column by column, inside a column in ascending (position, j); sources = the seeds, then the other sources in
             ascending node id; with probabilities q_ij = prob[pos] and the weights (1 / q_e) * k_s / sum (1 / q_e') over the column's
             edges with repeats counted (unit weights in a whole column and in a column that fell back to the uniform pick)
  layer-wise: n = min(fanout, C) draws over the candidate list; drawn[i] = 1 iff some draw picked i
"""
import math
from fractions import Fraction

import numpy as np

import neighbor_ref as nref
import wneighbor_ref as wref

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
LAYER_IDENT = 0xFFFFFFFF
MAX_FANOUT = 1024


def fin(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def group_key(seed, step, layer, ident):
    return fin(nref.mix(seed, step, layer) ^ (int(ident) & 0xFFFFFFFF))


def variate(h, j):
    return fin(h ^ (((j + 1) * GOLD) & M64))


def variates(seed, step, layer, ident, n):
    """The variates r_0 .. r_{n-1} of one group, Python ints."""
    h = group_key(seed, step, layer, ident)
    if n < 32:
        return [variate(h, j) for j in range(n)]
    with np.errstate(over="ignore"):                                  # the same arithmetic mod 2^64 on uint64 arrays
        z = np.uint64(h) ^ (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(GOLD))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return [int(x) for x in z]


def fixed_weights(bits):
    """bf16 bit patterns (uint16) of one group -> its fixed-point weights, a list of Python ints."""
    x = wref.from_bits(np.asarray(bits, dtype=np.uint16)).astype(np.float64)
    ok = np.isfinite(x) & (x > 0)
    if not bool(ok.any()):
        return [0] * len(x)
    E = math.frexp(float(x[ok].max()))[1] - 1                        # floor(log2): frexp's mantissa lies in [0.5, 1)
    scale = Fraction(2) ** (23 - E)
    return [int(Fraction(float(v)) * scale) if o else 0 for v, o in zip(x, ok)]   # (positive: int() floors)


def pick(r, weights, m):
    """One draw with variate ``r`` over a group of ``m`` entries; ``weights`` None (uniform) or the group's fixed-point weights."""
    W = 0 if weights is None else sum(weights)
    if W == 0:
        return (r * m) >> 64
    t = (r * W) >> 64
    acc = 0
    for i, w in enumerate(weights):
        acc += w
        if acc > t:
            return i
    raise AssertionError("t < W")


def picks(rs, weights, m):
    """``pick`` for every variate in ``rs`` (a prefix-sum search instead of the scan; the same results)."""
    W = 0 if weights is None else sum(weights)
    if W == 0:
        return [(r * m) >> 64 for r in rs]
    cum = np.cumsum(np.asarray(weights, dtype=np.int64))             # (w < 2^24, m < 2^31: no overflow)
    ts = np.array([(r * W) >> 64 for r in rs], dtype=np.int64)       # (t < W < 2^55)
    return np.searchsorted(cum, ts, side="right").tolist()


def column_weights(q, whole):
    """wneighbor_ref.hajek_weights over a column's edges with repeats counted (the same fp64 expression, rounded once to bf16),
    evaluated once per distinct q: a column drawn with replacement holds few of them."""
    q = np.asarray(q, dtype=np.float32)
    k = q.shape[0]
    if whole or k == 0 or not bool(((q > 0) & np.isfinite(q)).all()):
        return np.ones(k, dtype=np.float32)
    inv = 1.0 / q.astype(np.float64)
    tot = math.fsum(inv.tolist())
    uq, idx = np.unique(q, return_inverse=True)
    vals = [wref.fraction_to_bf16(Fraction(float((1.0 / np.float64(u)) * float(k) / tot))) for u in uq]
    return np.array(vals, dtype=np.float32)[idx]


def sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, prob_bits=None, r_override=None):
    """One node-wise layer.  ``prob_bits``: uint16 bf16 bit patterns by CSC position, or None (uniform).  ``r_override``: Python
    ints / uint64, the variate of draw j of column s at ``s * fanout + j``.  A seed id outside the graph is an empty column.
    Returns neighbor_ref.sample_layer's dict + ``picks`` (int32 per block edge), ``q_ij`` (uint16), ``weights`` (fp32 values of
    bf16), ``whole`` and ``fallback`` (bool per column)."""
    if fanout == 0 or fanout > MAX_FANOUT:
        raise ValueError("fanout")
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    V, S = len(indptr) - 1, len(seeds)
    cols, pks, fallback, E = [], [], np.zeros(S, dtype=bool), 0
    for s, v in enumerate(seeds.tolist()):
        if not 0 <= v < V:
            cols.append(np.zeros(0, dtype=np.int64)); pks.append(np.zeros(0, dtype=np.int64))
            continue
        a, d = int(indptr[v]), int(indptr[v + 1] - indptr[v])
        E += d
        if fanout < 0 or d == 0:
            pk = np.arange(d, dtype=np.int64)
        else:
            rs = ([int(r_override[s * fanout + j]) for j in range(fanout)] if r_override is not None
                  else variates(seed, step, layer, v, fanout))
            w = None if prob_bits is None else fixed_weights(np.asarray(prob_bits)[a:a + d])
            fallback[s] = w is not None and sum(w) == 0
            pk = np.sort(np.array(picks(rs, w, d), dtype=np.int64), kind="stable")     # ascending (position, j)
        cols.append(a + pk); pks.append(pk)
    n_col = [len(c) for c in cols]
    b_indptr = np.zeros(S + 1, dtype=np.int64)
    b_indptr[1:] = np.cumsum(n_col)
    pos = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, dtype=np.int64)
    dst = np.repeat(np.arange(S), n_col)
    src_g = indices[pos]
    new = np.setdiff1d(np.unique(src_g), seeds)                      # ascending node id, each once
    kept_nid = np.concatenate([seeds, new])
    local = np.full(V, -1, dtype=np.int64)
    ok = (kept_nid >= 0) & (kept_nid < V)
    local[kept_nid[ok][::-1]] = np.arange(len(kept_nid))[ok][::-1]    # (the first occurrence wins)
    src = local[src_g]
    K, B = len(kept_nid), len(pos)
    t_edge = np.argsort(src, kind="stable")
    t_indptr = np.searchsorted(src[t_edge], np.arange(K + 1))
    i32 = lambda x: np.asarray(x).astype(np.int32)
    lay = dict(indptr=i32(b_indptr), src=i32(src), dst=i32(dst), pos=i32(pos), eid=i32(pos if eid is None else np.asarray(eid)[pos]),
               kept_nid=i32(kept_nid), t_indptr=i32(t_indptr), t_edge=i32(t_edge), S=S, E=E, K=K, B=B,
               picks=i32(np.concatenate(pks) if pks else np.zeros(0)), fallback=fallback,
               whole=np.full(S, fanout < 0, dtype=bool))
    if prob_bits is None:
        lay["q_ij"] = np.full(B, 0x3F80, dtype=np.uint16)
        lay["weights"] = np.ones(B, dtype=np.float32)
    else:
        lay["q_ij"] = np.asarray(prob_bits, dtype=np.uint16)[pos]
        q = wref.from_bits(lay["q_ij"])
        w = np.ones(B, dtype=np.float32)
        for s in range(S):
            o, e = int(b_indptr[s]), int(b_indptr[s + 1])
            w[o:e] = column_weights(q[o:e], fanout < 0)
        lay["weights"] = w
    return lay


def sample_blocks(indptr, indices, eid, seeds, fanouts, seed, step, prob_bits=None):
    """L layers, ``fanouts`` in SAMPLING order; layer n's seeds are layer n - 1's kept nodes."""
    out = []
    for n, f in enumerate(fanouts):
        lay = sample_layer(indptr, indices, eid, seeds, int(f), seed, step, n, prob_bits=prob_bits)
        out.append(lay)
        seeds = lay["kept_nid"]
    return out


def mn_draw(p_bits, fanout, seed, step, layer, r_override=None):
    """The layer-wise draw over the candidates with bf16 importances ``p_bits``: (picks, int32 [min(fanout, C)]; drawn, int32 [C])."""
    C = len(p_bits)
    n = min(int(fanout), C)
    rs = [int(r_override[j]) for j in range(n)] if r_override is not None else variates(seed, step, layer, LAYER_IDENT, n)
    pk = np.array(picks(rs, fixed_weights(p_bits), C), dtype=np.int32)
    drawn = np.zeros(C, dtype=np.int32)
    drawn[pk] = 1
    return pk, drawn


def sigma_deviation(counts, probs, n_draws):
    """Largest |count - n p| / sqrt(n p (1 - p)) over the entries with 0 < p < 1; entries with p == 0 must have no count."""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    assert int(counts.sum()) == n_draws and bool((counts[probs == 0] == 0).all())
    m = (probs > 0) & (probs < 1)
    return float(np.max(np.abs(counts[m] - n_draws * probs[m]) / np.sqrt(n_draws * probs[m] * (1 - probs[m])), initial=0.0))


def compare(got, want):
    """A device layer ``got`` against the restatement ``want``: every integer array, the picks and q_ij equal; the weights as
    wneighbor_ref.compare holds them (one bf16 ulp, unit weights where the rule says so, |sum_e W_e - k_s| <= k_s * 2^-8)."""
    assert np.array_equal(np.asarray(got["picks"]), np.asarray(want["picks"])), "picks"
    wref.compare(got, want)
