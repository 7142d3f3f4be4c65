"""Restatement in NumPy of the rules of SAGE.inference(path="csc") (csrc/sage_infer.hip): the batch table and
EC_b of GCN.inference's batch structure (tests/gcn_infer_ref.py), the chunk-order float32 sum of 'mean' and the first-wins maximum
of 'pool'.  A plain helper module like gcn_infer_ref.py.

    batch b = rows [b * bs, min(V, (b + 1) * bs)),  E0_b = indptr[b * bs],  n_b edges,  EC_b = chunk_edges(n_b)
    mean: out[i] = bf16((1 / max(deg_i, 1)) * S_i): the batch's positions are cut into chunks of EC_b counted from E0_b; inside a
          chunk a row's terms are added in edge order from +0; a row's chunk partials are added in chunk order from the first
          partial; one product with the float32 scale; one rounding (nearest even).  A row without edges is +0.
    max:  out[i, c] = the running best over the row's edges, which starts at the first edge's value and moves on strict >.  A row
          without edges is +0.
"""
import numpy as np

from gcn_infer_ref import batch_table, chunk_edges, rbf


def mean_f32(indptr, indices, bs, h, chunks=True):
    """float32 emulation of the exact order -> [V, dim] float32 holding bf16 numbers.  The sequential float32 sum of a chunk's terms
    is NumPy's add.accumulate over (+0, term, term, ...).  ``chunks=False`` ignores the chunk grid (a planted fault: the plain
    edge-order sum of the whole row)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V = indptr.size - 1
    H = np.ascontiguousarray(h, dtype=np.float32)
    _, off = batch_table(indptr, bs)
    out = np.zeros((V, H.shape[1]), dtype=np.float32)
    zero = np.zeros((1, H.shape[1]), dtype=np.float32)
    for i in range(V):
        b = i // bs
        base = int(off[b])
        ec = chunk_edges(int(off[b + 1] - off[b])) if chunks else 1 << 62
        rs, re = int(indptr[i]) - base, int(indptr[i + 1]) - base
        if re <= rs:
            continue
        total, s = None, rs
        while s < re:
            e = min(re, (s // ec + 1) * ec)
            terms = H[indices[base + s:base + e]]
            part = np.add.accumulate(np.concatenate([zero, terms]), axis=0, dtype=np.float32)[-1]
            total = part if total is None else (total + part).astype(np.float32)
            s = e
        scale = np.float32(1.0) / np.float32(max(re - rs, 1))
        out[i] = rbf((scale * total).astype(np.float32))
    return out


def max_f32(indptr, indices, h):
    """The first-wins maximum -> [V, dim] float32 (the values of h, untouched: signed zeros kept)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V = indptr.size - 1
    H = np.ascontiguousarray(h, dtype=np.float32)
    out = np.zeros((V, H.shape[1]), dtype=np.float32)
    for i in range(V):
        rs, re = int(indptr[i]), int(indptr[i + 1])
        if re <= rs:
            continue
        best = H[indices[rs]].copy()
        for e in range(rs + 1, re):
            m = H[indices[e]]
            best = np.where(m > best, m, best)
        out[i] = best
    return out


def mean_edge_loop(indptr, indices, bs, h):
    """The mean rule as the kernel walks it, one float32 scalar at a time: a position on the batch's chunk grid that is not the row's
    first closes the open partial; the first partial starts the sum."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V = indptr.size - 1
    H = np.ascontiguousarray(h, dtype=np.float32)
    out = np.zeros((V, H.shape[1]), dtype=np.float32)
    for i in range(V):
        b0 = (i // bs) * bs
        b1 = min(V, b0 + bs)
        E0 = int(indptr[b0])
        ec = chunk_edges(int(indptr[b1]) - E0)
        rs, re = int(indptr[i]), int(indptr[i + 1])
        if re <= rs:
            continue
        for c in range(H.shape[1]):
            acc, total = np.float32(0), None
            for e in range(rs, re):
                if (e - E0) % ec == 0 and e != rs:
                    total = acc if total is None else np.float32(total + acc)
                    acc = np.float32(0)
                acc = np.float32(acc + H[indices[e], c])
            total = acc if total is None else np.float32(total + acc)
            out[i, c] = np.float32(np.float32(1.0) / np.float32(re - rs)) * total
    return rbf(out)


def max_edge_loop(indptr, indices, h):
    """The max rule, one Python float at a time."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V = indptr.size - 1
    H = np.ascontiguousarray(h, dtype=np.float32)
    out = np.zeros((V, H.shape[1]), dtype=np.float32)
    for i in range(V):
        for c in range(H.shape[1]):
            best = None
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                m = H[indices[e], c]
                if best is None or float(m) > float(best):
                    best = m
            if best is not None:
                out[i, c] = best
    return out


DESIGNED_ROW = 1


def designed_graph():
    """(indptr int64 [5], indices int32 [E], h float32 [4, 2] of bf16 numbers): four nodes, one batch of 16-edge chunks at any batch
    size >= 2.  Row 0 has 5 edges, so row DESIGNED_ROW = 1 starts mid-chunk at position 5; its 40 edges carry, in column 0,
    +2^24, then 38 times 1.0, then -2^24 (column 1: ones throughout).  Plain edge order: every 1.0 is absorbed by 2^24 (the tie
    rounds to even), the sum is 0.  Chunk order: [5, 16) gives 2^24, [16, 32) gives 16, [32, 45) gives 12 - 2^24; 2^24 + 16 is
    exact, the sum is 28 and the mean bf16(28 / 40).  Rows 2 and 3: one edge each."""
    big, one, neg = 0, 1, 2                                        # the nodes that carry +2^24, 1.0 and -2^24 in column 0
    rows = [[one] * 5, [big] + [one] * 38 + [neg], [3], [big]]
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    indices = np.array([j for r in rows for j in r], dtype=np.int32)
    h = np.array([[2.0 ** 24, 1.0], [1.0, 1.0], [-(2.0 ** 24), 1.0], [0.5, -3.0]], dtype=np.float32)
    return indptr, indices, h
