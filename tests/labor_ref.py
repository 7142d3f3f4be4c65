"""CPU restatement of the device-side LABOR-0 sampler's rule (csrc/labor.hip).  Integers only.

For sampling layer ``layer`` of draw step ``step``, seed column s with CSC positions [a, b), d = b - a:
  key(u)   = (uint32)(z >> 32), z = SplitMix64 finaliser of mix(seed, step, layer') ^ (uint64)u, u = indices[pos] -- the neighbor
             sampler's key (tests/neighbor_ref.py) with the edge's SOURCE NODE ID in the CSC position's place; layer' = layer, or 0
             for every layer with ``layer_dependency``
  kept     = every edge if fanout < 0 or d <= fanout (no key is computed); otherwise thr = (fanout << 32) // d and the edge at pos
             is kept iff key(indices[pos]) < thr -- a multi-edge is kept or dropped as one, a column may keep nothing
  block    = columns in seed order, ascending position inside a column; sources = the seeds (0 .. S-1, in the order given), then
             the other sources of kept edges, each once, in ascending node id; eid = eid[pos] (or pos); unit weights
"""
import numpy as np

from neighbor_ref import keys as _hash_keys, mix  # noqa: F401  (mix: the (seed, step, layer) mixing, = neighbor.hip:nb_mdkey)


def keys(seed, step, layer, nid):
    """uint32 key of every node id in ``nid``."""
    return _hash_keys(seed, step, layer, nid)


def threshold(fanout, d):
    return (int(fanout) << 32) // int(d)


def kept_positions(indices, a, b, fanout, seed, step, layer, keys_override=None):
    """The kept CSC positions of the column [a, b), ascending.  ``keys_override``: uint32 [V], by node id."""
    pos = np.arange(a, b, dtype=np.int64)
    d = b - a
    if fanout < 0 or d <= fanout:
        return pos
    u = np.asarray(indices)[pos].astype(np.int64)
    key = keys(seed, step, layer, u) if keys_override is None else np.asarray(keys_override, dtype=np.uint32)[u]
    return pos[key.astype(np.uint64) < np.uint64(threshold(fanout, d))]


def sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, keys_override=None):
    """One layer.  Returns a dict of int32 arrays (indptr, src, dst, pos, eid, kept_nid, t_indptr, t_edge) and the counts
    S, E, K, B -- the return dict of neighbor_ref.sample_layer."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    S = len(seeds)
    cols = [kept_positions(indices, int(indptr[s]), int(indptr[s + 1]), fanout, seed, step, layer, keys_override) for s in seeds]
    b_indptr = np.zeros(S + 1, dtype=np.int64)
    b_indptr[1:] = np.cumsum([len(c) for c in cols])
    pos = (np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)).astype(np.int64)
    dst = np.repeat(np.arange(S), [len(c) for c in cols])
    src_g = indices[pos]
    new = np.setdiff1d(np.unique(src_g), seeds)          # ascending node id, each once
    kept_nid = np.concatenate([seeds, new])
    local = {int(v): i for i, v in enumerate(kept_nid)}
    src = np.array([local[int(v)] for v in src_g], dtype=np.int64)
    K, B = len(kept_nid), len(pos)
    t_edge = np.argsort(src, kind="stable")
    t_indptr = np.searchsorted(src[t_edge], np.arange(K + 1))
    i32 = lambda x: np.asarray(x).astype(np.int32)
    return dict(indptr=i32(b_indptr), src=i32(src), dst=i32(dst), pos=i32(pos),
                eid=i32(pos if eid is None else np.asarray(eid)[pos]), kept_nid=i32(kept_nid), t_indptr=i32(t_indptr),
                t_edge=i32(t_edge), S=S, E=int((indptr[seeds + 1] - indptr[seeds]).sum()), K=K, B=B)


def sample_blocks(indptr, indices, eid, seeds, fanouts, seed, step, layer_dependency=False):
    """L layers; ``fanouts`` in SAMPLING order (last block first).  Returns the layers in sampling order: layer n's seeds are
    layer n - 1's kept nodes.  ``layer_dependency``: every layer draws with layer 0's keys."""
    out = []
    for n, f in enumerate(fanouts):
        lay = sample_layer(indptr, indices, eid, seeds, int(f), seed, step, 0 if layer_dependency else n)
        out.append(lay)
        seeds = lay["kept_nid"]
    return out
