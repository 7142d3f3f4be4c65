"""What a block is, whether or not a capacity clamped it: invariants I1 - I7 of include/bliss_gnn.h ("clamped blocks") and DESIGN.md
section 35, as one pure-NumPy checker.  tests/test_block_invariants.py pins it on the CPU (it accepts the oracle's blocks and
rejects planted single-entry faults under the right invariant) before tests/test_gpu_clamped_blocks.py lets it judge a kernel.

``check(arrays, caps, graph, seeds, clamped)``
  arrays   one layer: the counts ``S K B`` (ints; optional ``C``, optional ``err`` = the record's error word) and the arrays
           ``indptr src dst pos eid kept_nid`` plus, where the kind writes them, ``t_indptr t_edge edge_weights q p_ij node_prob``.
           Arrays may be longer than the counts say -- the capacity-sized buffers as they are; bf16 arrays come as 16-bit integers
           (the bit patterns) or as floats.
  caps     ``dict(S=, K=, B=[, C=])``: the capacities the arrays were written under (an exact-size block: its own counts).
  graph    ``(indptr, indices, eid)`` of the message graph, ``eid`` None = identity.
  seeds    the layer's seeds in order (may be longer than S when the seed capacity clamped), or None: I4's seed prefix is skipped.
  clamped  which capacities were exceeded, a subset of "SKBC".
Raises ``Violation`` (an AssertionError) whose message starts with the invariant's name and names the first offending index."""
import numpy as np

ERR_BITS = {"C": 2, "K": 4, "B": 8, "S": 64}            # BLISS_ERR_CAP_CAND / _KEPT / _EDGES / _SEEDS
CAP_MASK = 2 | 4 | 8 | 64


class Violation(AssertionError):
    def __init__(self, invariant, what):
        super().__init__("%s: %s" % (invariant, what))
        self.invariant = invariant


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def _need(inv, ok, what, *args):
    if not ok:
        raise Violation(inv, what % args)


def _all(inv, mask, what, values=None):
    """Every entry of ``mask`` holds, or the first that does not is named."""
    mask = np.asarray(mask)
    if not mask.all():
        i = _first(~mask)
        raise Violation(inv, "%s at index %d%s" % (what, i, "" if values is None else " (value %s)" % (values[i],)))


def nonfinite(a):
    """Per entry: NaN or infinity.  16-bit integers are bf16 bit patterns (exponent field all ones)."""
    a = np.asarray(a)
    if a.dtype.kind in "iu":
        return (a.astype(np.int64) & 0x7F80) == 0x7F80
    return ~np.isfinite(a.astype(np.float64))


def check_index(src, t_indptr, t_edge, K, B, cap_k):
    """I3's ``0 <= src[e] < K`` and I6, the by-source index, alone: what the per-sampler overflow tests add to their own checks."""
    src, t_indptr, t_edge = (np.asarray(x).astype(np.int64) for x in (src, t_indptr, t_edge))
    _need("I3", len(src) >= B, "src holds %d entries, B = %d", len(src), B)
    src = src[:B]
    _all("I3", (src >= 0) & (src < K), "src outside [0, K = %d)" % K, src)
    _need("I6", len(t_indptr) >= cap_k + 1, "t_indptr holds %d entries, cap_k + 1 = %d", len(t_indptr), cap_k + 1)
    _need("I6", len(t_edge) >= B, "t_edge holds %d entries, B = %d", len(t_edge), B)
    t_indptr, t_edge = t_indptr[:cap_k + 1], t_edge[:B]
    _need("I6", t_indptr[0] == 0, "t_indptr[0] = %d", t_indptr[0])
    _all("I6", np.diff(t_indptr) >= 0, "t_indptr decreases after", t_indptr)
    _all("I6", t_indptr[K:] == B, "t_indptr (offset from K = %d) is not B = %d" % (K, B), t_indptr[K:])
    _all("I6", (t_edge >= 0) & (t_edge < B), "t_edge outside [0, B = %d)" % B, t_edge)
    seen = np.bincount(t_edge, minlength=B)
    if (seen != 1).any():
        e = _first(seen > 1) if (seen > 1).any() else _first(seen == 0)
        raise Violation("I6", "t_edge is no permutation: edge %d appears %d times (first at index %d)"
                        % (e, seen[e], _first(t_edge == e) if seen[e] else -1))
    owner = np.repeat(np.arange(cap_k), np.diff(t_indptr))           # the list every slot of t_edge lies in
    _all("I6", src[t_edge] == owner, "list holds an edge of another source", t_edge)
    inside = owner[1:] == owner[:-1]
    _all("I6", ~inside | (np.diff(t_edge) > 0), "by-source list not in ascending edge index after", t_edge)


def check(arrays, caps, graph, seeds, clamped=""):
    g_indptr, g_indices, g_eid = graph
    g_indices = np.asarray(g_indices).astype(np.int64)
    V, Eg = len(g_indptr) - 1, len(g_indices)
    clamped = set(clamped)
    _need("I1", clamped <= set("SKBC"), "clamped names %s", sorted(clamped))
    S, K, B = int(arrays["S"]), int(arrays["K"]), int(arrays["B"])
    cs, ck, cb = int(caps["S"]), int(caps["K"]), int(caps["B"])
    get = lambda name: None if arrays.get(name) is None else np.asarray(arrays[name])
    i64 = lambda name: np.asarray(arrays[name]).astype(np.int64)

    # ---- I1: the counts are within the capacities, a clamped count sits AT its capacity, the error word says which
    for name, n, cap in (("S", S, cs), ("K", K, ck), ("B", B, cb)):
        _need("I1", 0 <= n <= cap, "%s = %d outside [0, cap_%s = %d]", name, n, name.lower(), cap)
    for name, n, cap in (("S", S, cs), ("K", K, ck), ("B", B, cb)):
        _need("I1", name not in clamped or n == cap, "%s = %d was clamped but is not the capacity %d", name, n, cap)
    if arrays.get("C") is not None and caps.get("C") is not None:
        _need("I1", int(arrays["C"]) <= int(caps["C"]), "C = %d above cap_c = %d", int(arrays["C"]), int(caps["C"]))
    if arrays.get("err") is not None:
        want = sum(ERR_BITS[c] for c in clamped)
        _need("I1", int(arrays["err"]) & CAP_MASK == want, "error word 0x%x, capacity bits 0x%x expected", int(arrays["err"]), want)

    # ---- I2: indptr over [0, cap_s]
    indptr = i64("indptr")
    _need("I2", len(indptr) >= cs + 1, "indptr holds %d entries, cap_s + 1 = %d", len(indptr), cs + 1)
    indptr = indptr[:cs + 1]
    _need("I2", indptr[0] == 0, "indptr[0] = %d", indptr[0])
    _all("I2", np.diff(indptr) >= 0, "indptr decreases after", indptr)
    _need("I2", indptr[S] == B, "indptr[S = %d] = %d, B = %d", S, indptr[S], B)
    _all("I2", indptr[S:] == B, "padding row of indptr (offset from S = %d) is not B = %d" % (S, B), indptr[S:])

    # ---- I3: every edge below B
    src, dst, pos, eid = (i64(n) for n in ("src", "dst", "pos", "eid"))
    for name, a in (("src", src), ("dst", dst), ("pos", pos), ("eid", eid)):
        _need("I3", len(a) >= B, "%s holds %d entries, B = %d", name, len(a), B)
    src, dst, pos, eid = src[:B], dst[:B], pos[:B], eid[:B]
    _all("I3", (src >= 0) & (src < K), "src outside [0, K = %d)" % K, src)
    _all("I3", dst == np.repeat(np.arange(S), np.diff(indptr[:S + 1])), "dst is not the row indptr puts the edge in,", dst)
    _all("I3", (pos >= 0) & (pos < Eg), "pos outside [0, |E| = %d)" % Eg, pos)
    _all("I3", eid == (pos if g_eid is None else np.asarray(g_eid).astype(np.int64)[pos]), "eid != g.eid[pos]", eid)

    # ---- I4: kept_nid
    kept = i64("kept_nid")
    _need("I4", len(kept) >= ck, "kept_nid holds %d entries, cap_k = %d", len(kept), ck)
    _all("I4", (kept[:K] >= 0) & (kept[:K] < V), "kept_nid outside [0, |V| = %d)" % V, kept)
    order = np.argsort(kept[:K], kind="stable")
    rep = np.flatnonzero(np.diff(kept[:K][order]) == 0)
    if rep.size:
        i = int(order[rep + 1].min())
        raise Violation("I4", "kept_nid repeats node %d at index %d" % (kept[i], i))
    if seeds is not None:
        m = min(S, K)
        want = np.asarray(seeds).astype(np.int64)
        _need("I4", len(want) >= m, "%d seeds given, min(S, K) = %d", len(want), m)
        _all("I4", kept[:m] == want[:m], "kept_nid is not the seed", kept)
    _all("I4", kept[K:ck] == 0, "kept_nid padding (offset from K = %d) is not 0" % K, kept[K:ck])

    # ---- I5: an edge's source id names its true source (every edge unless K clamped; then those whose source was kept)
    true_src = g_indices[pos]
    named = kept[src]
    must = np.ones(B, dtype=bool) if "K" not in clamped else np.isin(true_src, kept[:K])
    _all("I5", ~must | (named == true_src), "kept_nid[src] != g.indices[pos]", named)

    # ---- I6: the by-source index
    if get("t_indptr") is not None:
        check_index(src, arrays["t_indptr"], arrays["t_edge"], K, B, ck)

    # ---- I7: no NaN, no infinity
    for name, n in (("edge_weights", B), ("q", B), ("p_ij", B), ("node_prob", ck)):
        a = get(name)
        if a is not None:
            _need("I7", len(a) >= n, "%s holds %d entries, %d expected", name, len(a), n)
            _all("I7", ~nonfinite(a[:n]), name + " is NaN or infinite", a)
