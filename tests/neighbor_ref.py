"""CPU restatement of the device-side neighbor sampler's rule (csrc/neighbor.hip).  Integers only.

For sampling layer ``layer`` of draw step ``step``, seed column s with CSC positions [a, b), d = b - a:
  key(pos) = (uint32)(z >> 32), z = SplitMix64 finaliser of mix(seed, step, layer) ^ (uint64)pos -- the (seed, step, layer)
             mixing of ``oracle.bliss_oracle.keyed_uniform`` with the CSC position in the node id's place, top 32 bits
  k        = d if fanout < 0 or d <= fanout, else fanout; kept = the k smallest pairs (key(pos), pos)
  block    = columns in seed order, ascending position inside a column; sources = the seeds (0 .. S-1, in the order given), then
             the other sources of kept edges, each once, in ascending node id; eid = eid[pos] (or pos); unit weights
"""
import numpy as np

M64 = (1 << 64) - 1


def mix(seed, step, layer):
    key = ((int(seed) * 0x9E3779B97F4A7C15) + int(step)) & M64
    key = ((key ^ (key >> 30)) * 0xBF58476D1CE4E5B9) & M64
    key = ((key ^ (key >> 27)) * 0x94D049BB133111EB) & M64
    key ^= key >> 31
    return key ^ ((int(layer) & 0xFF) << 56)


def keys(seed, step, layer, pos):
    """uint32 key of every CSC position in ``pos``."""
    z = np.uint64(mix(seed, step, layer)) ^ np.asarray(pos).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def kept_positions(a, b, fanout, seed, step, layer, keys_override=None):
    """The kept CSC positions of the column [a, b), ascending."""
    pos = np.arange(a, b, dtype=np.int64)
    d = b - a
    if fanout < 0 or d <= fanout:
        return pos
    key = keys(seed, step, layer, pos) if keys_override is None else np.asarray(keys_override, dtype=np.uint32)[pos]
    order = np.lexsort((pos, key))                       # by key, ties to the lower position
    return np.sort(pos[order[:fanout]])


def sample_layer(indptr, indices, eid, seeds, fanout, seed, step, layer, keys_override=None):
    """One layer.  Returns a dict of int32 arrays (indptr, src, dst, pos, eid, kept_nid, t_indptr, t_edge) and the counts
    S, E, K, B."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    S = len(seeds)
    cols = [kept_positions(int(indptr[s]), int(indptr[s + 1]), fanout, seed, step, layer, keys_override) for s in seeds]
    b_indptr = np.zeros(S + 1, dtype=np.int64)
    b_indptr[1:] = np.cumsum([len(c) for c in cols])
    pos = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    pos = pos.astype(np.int64)
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


def sample_blocks(indptr, indices, eid, seeds, fanouts, seed, step):
    """L layers; ``fanouts`` in SAMPLING order (last block first).  Returns the layers in sampling order: layer n's seeds are
    layer n - 1's kept nodes."""
    out = []
    for n, f in enumerate(fanouts):
        lay = sample_layer(indptr, indices, eid, seeds, int(f), seed, step, n)
        out.append(lay)
        seeds = lay["kept_nid"]
    return out
