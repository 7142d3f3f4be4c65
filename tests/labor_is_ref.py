"""CPU restatement of the device-side LABOR-i sampler's rule (csrc/labor_is.hip).  Unsigned integers up to
the weights; ONE = 2^32.

For sampling layer ``layer`` of draw step ``step`` with seeds s_0 .. s_{S-1}, fanout f and I >= 0 iterations; column s has CSC
positions [a, b), d = b - a, sources u = indices[pos]; it is WHOLE if f < 0 or d <= f (every edge kept, no key computed).  Every
position is its own term in the sums (a multi-edge is m equal terms, kept or dropped as one).
  importances  pi_u in [1, ONE]; pi^(0)_u = ONE
  scale        c_s(pi) = the largest c in [0, ONE - 1] with sum_pos (c * pi_{indices[pos]}) >> 32 <= f * ONE   (non-whole columns)
  iteration    pi^(i+1)_u = max(1, max over the frontier edges u -> s of P), P = ONE if s is whole, else (c_s(pi^(i)) * pi^(i)_u) >> 32;
               the maximum is over the new values only; vertices outside the frontier are never read
  draw         p_pos = (c_s(pi^(I)) * pi^(I)_u) >> 32; kept iff key(u) < p_pos, key = tests/labor_ref.py's (I = 0 is LABOR-0 bit for bit)
  block        tests/labor_ref.py's
  q_ij         bf16(fp32(p_pos) * 2^-32), both roundings to nearest even; 1.0 in whole columns
  edge_weights W_e = (ONE / p_e) * k_s / sum_{kept e' of the column} (ONE / p_e') in fp64, the sum in column order; 1.0 in whole columns
"""
import numpy as np

import labor_ref
from labor_ref import keys, mix  # noqa: F401  (the key and the (seed, step, layer) mixing are LABOR-0's)

ONE = 1 << 32
_U = np.uint64


def scale(pis, f):
    """c_s of one non-whole column: ``pis`` = the importance of every position's source (ints in [1, ONE]), ``f`` the fanout.
    32 bisection steps from bit 31 down (the sum is nondecreasing in c)."""
    pis = np.asarray(pis, dtype=np.uint64)
    lim = int(f) << 32
    c = 0
    for bit in range(31, -1, -1):
        t = c | (1 << bit)
        if int(((_U(t) * pis) >> _U(32)).sum(dtype=np.uint64)) <= lim:
            c = t
    return c


def _columns(indptr, seeds):
    return [(int(indptr[s]), int(indptr[s + 1])) for s in seeds]


def _scales(indices, cols, fanout, pi):
    return [None if fanout < 0 or b - a <= fanout else scale(pi[indices[a:b]], fanout) for a, b in cols]


def importances(indptr, indices, seeds, fanout, iterations):
    """pi^(I) (uint64 [V]; entries outside the frontier are meaningless and stay ONE) and c_s(pi^(I)) per column (None: whole)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    cols = _columns(indptr, seeds)
    pi = np.full(len(indptr) - 1, ONE, dtype=np.uint64)
    c = _scales(indices, cols, fanout, pi)
    for _ in range(int(iterations)):
        new = np.zeros_like(pi)
        for (a, b), cs in zip(cols, c):
            u = indices[a:b]
            P = np.full(b - a, ONE, dtype=np.uint64) if cs is None else (_U(cs) * pi[u]) >> _U(32)
            np.maximum.at(new, u, P)
        front = np.unique(np.concatenate([indices[a:b] for a, b in cols])) if cols else np.zeros(0, dtype=np.int64)
        pi = pi.copy()
        pi[front] = np.maximum(new[front], _U(1))
        c = _scales(indices, cols, fanout, pi)
    return pi, c


def bf16_of_p(p):
    """uint16 bf16 bits of fp32(p) * 2^-32 for uint32-range integers p: uint -> fp32 and fp32 -> bf16, both to nearest even."""
    x = (np.asarray(p, dtype=np.uint64).astype(np.float32) * np.float32(2.0 ** -32)).view(np.uint32)
    return ((x + np.uint32(0x7FFF) + ((x >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_of_f64(x):
    """uint16 bf16 bits of positive normal fp64 values, ONE rounding to nearest even (no detour through fp32)."""
    b = np.asarray(x, dtype=np.float64).view(np.uint64)
    e = ((b >> _U(52)) & _U(0x7FF)).astype(np.int64) - 1023 + 127
    m = b & _U((1 << 52) - 1)
    q, rem = (m >> _U(45)).astype(np.int64), m & _U((1 << 45) - 1)
    q = q + ((rem > _U(1 << 44)) | ((rem == _U(1 << 44)) & ((q & 1) == 1)))
    e, q = e + (q >> 7), q & 127
    return ((e << 7) | q).astype(np.uint16)


def _assemble(indptr, indices, eid, seeds, cols):
    """labor_ref.sample_layer's block assembly around the kept positions ``cols`` (one array per seed column): the function is
    called as it stands, with its per-column draw answered from ``cols``."""
    it = iter(cols)
    saved = labor_ref.kept_positions
    labor_ref.kept_positions = lambda *a, **k: next(it)
    try:
        return labor_ref.sample_layer(indptr, indices, eid, seeds, 1, 0, 0, 0)
    finally:
        labor_ref.kept_positions = saved


def sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, iterations, keys_override=None, pi_override=None):
    """One layer: labor_ref.sample_layer's dict plus ``q_ij`` (uint16 bf16 bits, [B]), ``edge_weights`` (fp64, [B]), ``c`` (uint64
    [S], 0 in whole columns), ``p`` (uint64 [E], per frontier position in seed order, ONE in whole columns) and ``p_e`` (uint64
    [B], of the kept edges).  ``keys_override``: uint32 [V], by node id.  ``pi_override`` (tests of the draw alone): uint64 [V]
    importances that take pi^(I)'s place, the scales found for them."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    pi, cs = importances(indptr, indices, seeds, fanout, iterations)
    if pi_override is not None:
        pi = np.asarray(pi_override, dtype=np.uint64)
        cs = _scales(indices, _columns(indptr, seeds), fanout, pi)
    kept, ps, pes, ws = [], [], [], []
    for (a, b), c in zip(_columns(indptr, seeds), cs):
        pos = np.arange(a, b, dtype=np.int64)
        if c is None:
            kept.append(pos)
            ps.append(np.full(b - a, ONE, dtype=np.uint64))
            pes.append(ps[-1])
            ws.append(np.ones(b - a))
            continue
        u = indices[pos]
        p = (_U(c) * pi[u]) >> _U(32)
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
    lay = _assemble(indptr, indices, eid, seeds, kept)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    p_e = cat(pes, np.uint64)
    q = bf16_of_p(np.minimum(p_e, _U(ONE - 1)))
    q[p_e == _U(ONE)] = 0x3F80
    lay.update(q_ij=q, edge_weights=cat(ws, np.float64), c=np.array([0 if c is None else c for c in cs], dtype=np.uint64),
               p=cat(ps, np.uint64), p_e=p_e)
    return lay


def sample_blocks(indptr, indices, eid, seeds, fanouts, seed, step, iterations, layer_dependency=False):
    """L layers; ``fanouts`` in SAMPLING order.  Layer n's seeds are layer n - 1's kept nodes; the importances start again from
    ONE in every layer.  ``layer_dependency``: every layer draws with layer 0's keys."""
    out = []
    for n, f in enumerate(fanouts):
        lay = sample_layer(indptr, indices, eid, seeds, int(f), seed, step, 0 if layer_dependency else n, iterations)
        out.append(lay)
        seeds = lay["kept_nid"]
    return out
