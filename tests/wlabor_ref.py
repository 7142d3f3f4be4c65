"""CPU restatement of the weighted device-side LABOR sampler's rule (csrc/labor_w.hip).  Unsigned integers
from the bf16 bits of the edge probabilities up to the weights; ONE = 2^32.

For sampling layer ``layer`` of draw step ``step`` with seeds s_0 .. s_{S-1} and fanout f; column s has CSC positions [a, b),
d = b - a, sources u = indices[pos]; it is WHOLE if f < 0 or d <= f (every edge kept, no key computed, unit weights).
  q_pos        prob_pos[pos] (raw mode: bf16, unnormalised), or tests/wneighbor_ref.py's ``exp3_q_pos`` (EXP3 mode)
  valid        q_pos positive and finite; from its bf16 bits (exponent field E, 7-bit mantissa M): m = E ? 128 + M : M, e = max(E, 1)
  a_pos        (m << 24) >> (e_max - e), e_max the largest e over the column's valid edges; 0 when the shift is >= 32 and for an
               invalid edge
  p_pos(c)     min(ONE - 1, (c * a_pos) >> 24)
  scale        c_s = the largest c in [0, ONE - 1] with sum_pos p_pos(c) <= f * ONE: 32 bisection steps from bit 31 down
  draw         kept iff key(u) < p_pos(c_s), key = tests/labor_ref.py's; an edge with a_pos = 0 is never kept in a non-whole column
  block        tests/labor_ref.py's
  q_ij         q_pos of every kept edge (whole columns too);  p_ij = bf16(fp32(p_pos) * 2^-32), 1.0 in whole columns
  edge_weights W_e = (ONE / p_e) * k_s / sum_{kept e' of the column} (ONE / p_e') in fp64, the sum in column order; 1.0 in whole columns
"""
import numpy as np

import labor_is_ref
import wneighbor_ref
from labor_is_ref import bf16_of_f64, bf16_of_p  # noqa: F401  (the two roundings of the outputs are LABOR-i's)
from labor_ref import keys
from wneighbor_ref import exp3_q_pos  # noqa: F401  (EXP3 mode's q is the weighted neighbor draw's)

ONE = 1 << 32
_U = np.uint64


def q_bits(q):
    """uint16 bf16 bits of fp32 values that are bf16 values (a NaN becomes 0x7FC0, torch's)."""
    return wneighbor_ref.bf16_bits(np.asarray(q, dtype=np.float32))


def column_weights(bits):
    """(a_pos uint64 [d], e_max) of one non-whole column from the bf16 bits of its q.  e_max = 0 without a valid edge."""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    E, M = (b >> 7) & 0xFF, b & 0x7F
    valid = ((b & 0x8000) == 0) & (E != 0xFF) & ((b & 0x7FFF) != 0)
    m = np.where(E != 0, 128 + M, M)
    e = np.maximum(E, 1)
    if not bool(valid.any()):
        return np.zeros(len(b), dtype=np.uint64), 0
    e_max = int(e[valid].max())
    sh = e_max - e
    a = np.where(valid & (sh < 32), (m << 24) >> np.minimum(np.maximum(sh, 0), 63), 0)
    return a.astype(np.uint64), e_max


def probs(c, a):
    """p_pos(c) for the integer weights ``a`` (uint64)."""
    return np.minimum((_U(c) * np.asarray(a, dtype=np.uint64)) >> _U(24), _U(ONE - 1))


def scale(a, f):
    """c_s of one non-whole column with integer weights ``a`` and fanout ``f``."""
    a = np.asarray(a, dtype=np.uint64)
    lim = int(f) << 32
    c = 0
    for bit in range(31, -1, -1):
        t = c | (1 << bit)
        if int(probs(t, a).sum(dtype=np.uint64)) <= lim:
            c = t
    return c


def sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, q_pos, keys_override=None):
    """One layer.  ``q_pos``: fp32 values of the bf16 probabilities by CSC position.  ``keys_override``: uint32 [V], by node id.
    Returns labor_ref.sample_layer's dict plus ``q_ij`` / ``p_ij`` (uint16 bf16 bits, [B]), ``edge_weights`` (fp64, [B]), ``c``
    (uint64 [S], 0 in whole columns), ``e_max`` (int64 [S]), ``p`` (uint64 [E], per frontier position in seed order, ONE in whole
    columns), ``p_e`` (uint64 [B], of the kept edges) and ``whole`` (bool [S])."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    bits = q_bits(q_pos)
    kept, ps, pes, ws, cs, ems, whole = [], [], [], [], [], [], []
    for s in seeds:
        a, b = int(indptr[s]), int(indptr[s + 1])
        pos = np.arange(a, b, dtype=np.int64)
        if fanout < 0 or b - a <= fanout:
            kept.append(pos)
            ps.append(np.full(b - a, ONE, dtype=np.uint64))
            pes.append(ps[-1])
            ws.append(np.ones(b - a))
            cs.append(0)
            ems.append(0)
            whole.append(True)
            continue
        aw, e_max = column_weights(bits[a:b])
        c = scale(aw, fanout)
        p = probs(c, aw)
        u = indices[pos]
        key = keys(seed, step, layer, u) if keys_override is None else np.asarray(keys_override, dtype=np.uint32)[u]
        take = key.astype(np.uint64) < p
        kept.append(pos[take])
        ps.append(p)
        pes.append(p[take])
        inv = float(ONE) / p[take].astype(np.float64)
        tot = 0.0
        for x in inv.tolist():                                 # in column order
            tot += x
        ws.append(inv * float(len(inv)) / tot if len(inv) else inv)
        cs.append(c)
        ems.append(e_max)
        whole.append(False)
    lay = labor_is_ref._assemble(indptr, indices, eid, seeds, kept)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    p_e = cat(pes, np.uint64)
    p_ij = bf16_of_p(np.minimum(p_e, _U(ONE - 1)))
    p_ij[p_e == _U(ONE)] = 0x3F80
    lay.update(q_ij=bits[lay["pos"].astype(np.int64)], p_ij=p_ij, edge_weights=cat(ws, np.float64),
               c=np.array(cs, dtype=np.uint64), e_max=np.array(ems, dtype=np.int64), p=cat(ps, np.uint64), p_e=p_e,
               whole=np.array(whole, dtype=bool))
    return lay


def sample_blocks(indptr, indices, eid, seeds, fanouts, seed, step, q_rows, layer_dependency=False):
    """L layers; ``fanouts`` and ``q_rows`` (one q_pos per layer, or a function layer seeds -> q_pos) in SAMPLING order.  Layer n's
    seeds are layer n - 1's kept nodes.  ``layer_dependency``: every layer draws with layer 0's keys."""
    out = []
    for n, f in enumerate(fanouts):
        q = q_rows[n](seeds) if callable(q_rows[n]) else q_rows[n]
        lay = sample_layer(indptr, indices, eid, seeds, int(f), seed, step, 0 if layer_dependency else n, q)
        out.append(lay)
        seeds = lay["kept_nid"]
    return out
