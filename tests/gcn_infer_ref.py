"""Restatement in NumPy of the rules of GCN.inference(path="csc") (csrc/gcn_infer.hip): the batch table,
the per-edge source count of the batch structure, the fp32 norms, and the chunked sum -- in float64 with magnitudes (for
gcn_ref.GCN_SPMM_K) and as a float32 emulation of the exact summation order.  A plain helper module like gcn_ref.py.

    batch b   = rows [b * bs, min(V, (b + 1) * bs)),  E0_b = indptr[b * bs],  n_b edges
    cnt(b, j) = positions of [E0_b, E0_b + n_b) whose source is j                       (parallel edges count once each)
    ns_e = 1 / sqrt(max(cnt, 1))   nd_i = 1 / sqrt(max(indeg_i, 1))                     (float32: IEEE sqrt, one division)
    out[i] = bf16(nd_i * sum_e ns_e h[indices[e]]): chunks of EC_b = chunk_edges(n_b) positions counted from E0_b; inside a chunk a
    row's terms are added in edge order from zero; a row's chunk partials are added in chunk order from the first partial.

``fault`` plants one error (tests/test_gcn_infer_ref.py shows that each lands outside GCN_SPMM_K); the float64 value and the
magnitudes never see a fault."""
import numpy as np


def chunk_edges(n):
    """bliss_spmm_chunk_edges."""
    return 64 if n >= 200000 else (32 if n >= 50000 else 16)


def batch_table(indptr, bs):
    """(bounds [nb + 1] = the first row of every batch, then V;  off [nb + 1] = E0_b of every batch, then E)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    V = indptr.size - 1
    bounds = np.append(np.arange(0, V, bs, dtype=np.int64), V)
    return bounds, indptr[bounds]


def batch_chunks(indptr, bs):
    """EC_b of every batch."""
    _, off = batch_table(indptr, bs)
    return [chunk_edges(int(n)) for n in np.diff(off)]


def edge_dst(indptr):
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def counts(indptr, indices, bs, fault=None):
    """cnt [E] int64.  fault: whole_graph (the source's out-degree in the graph); range = (row0, row1): counted over that range
    of whole batches for the edges inside it; parallel_once: parallel edges of one destination count once; spill: the positions
    of the NEXT batch count into this one."""
    fault = fault or {}
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V, E = indptr.size - 1, indices.size
    dst = edge_dst(indptr)
    group = dst // bs                                                   # the batch of every edge
    if fault.get("whole_graph"):
        group = np.zeros(E, dtype=np.int64)
    if "range" in fault:
        r0, r1 = fault["range"]
        group = np.where((dst >= r0) & (dst < r1), -1, group)
    key = group * V + indices
    if fault.get("parallel_once"):
        _, first = np.unique(dst * V + indices, return_index=True)
        uniq, c = np.unique(key[first], return_counts=True)
    else:
        uniq, c = np.unique(key, return_counts=True)
    cnt = c[np.searchsorted(uniq, key)]
    if fault.get("spill"):
        nxt = (group + 1) * V + indices                                 # the same source in the next batch
        pos = np.clip(np.searchsorted(uniq, nxt), 0, uniq.size - 1)
        cnt = cnt + np.where(uniq[pos] == nxt, c[pos], 0)
    return cnt.astype(np.int64)


def norms(indptr, indices, bs, fault=None):
    """(ns [E], nd [V]) float32 with the kernel's expressions.  fault: those of ``counts``; nd_unclamped: 1 / sqrt(indeg)."""
    fault = fault or {}
    cnt = counts(indptr, indices, bs, fault)
    indeg = np.diff(np.asarray(indptr, dtype=np.int64))
    ind = indeg if fault.get("nd_unclamped") else np.maximum(indeg, 1)
    with np.errstate(divide="ignore"):
        ns = np.float32(1.0) / np.sqrt(np.maximum(cnt, 1).astype(np.float32))
        nd = np.float32(1.0) / np.sqrt(ind.astype(np.float32))
    return ns.astype(np.float32), nd.astype(np.float32)


def spmm_f64(indptr, indices, bs, h):
    """(ref, mag) float64 [V, dim]: the sum with float64 norms, and the same formula on absolute values."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V = indptr.size - 1
    H = np.asarray(h, dtype=np.float64)
    cnt = counts(indptr, indices, bs)
    ns = 1.0 / np.sqrt(np.maximum(cnt, 1).astype(np.float64))
    nd = 1.0 / np.sqrt(np.maximum(np.diff(indptr), 1).astype(np.float64))
    dst = edge_dst(indptr)
    ref, mag = np.zeros((V, H.shape[1])), np.zeros((V, H.shape[1]))
    np.add.at(ref, dst, ns[:, None] * H[indices])
    np.add.at(mag, dst, ns[:, None] * np.abs(H[indices]))
    return nd[:, None] * ref, nd[:, None] * mag


def rbf(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def spmm_f32(indptr, indices, bs, h, fault=None, origin="batch", rows=None, range_row0=0):
    """float32 emulation of the exact order -> [V, dim] float32 holding bf16 numbers (rows outside ``rows`` = (lo, hi) stay zero).
    The sequential float32 sum of a chunk's terms is NumPy's add.accumulate; the product ns_e * h is rounded to float32 before
    it is added (no fused multiply-add).  origin: "batch" counts the chunks from E0_b (the rule); "range": from the first edge of
    row ``range_row0`` with the batch's EC (a planted fault).  fault: see ``norms``; with nd_unclamped a row without edges is
    nd * 0 instead of 0."""
    fault = fault or {}
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    V = indptr.size - 1
    H = np.ascontiguousarray(h, dtype=np.float32)
    ns, nd = norms(indptr, indices, bs, fault)
    bounds, off = batch_table(indptr, bs)
    out = np.zeros((V, H.shape[1]), dtype=np.float32)
    lo, hi = (0, V) if rows is None else rows
    for i in range(lo, hi):
        b = i // bs
        ec = chunk_edges(int(off[b + 1] - off[b]))
        base = int(off[b]) if origin == "batch" else int(indptr[range_row0])
        rs, re = int(indptr[i]) - base, int(indptr[i + 1]) - base
        if re <= rs:
            if fault.get("nd_unclamped"):
                with np.errstate(invalid="ignore"):
                    out[i] = nd[i] * np.float32(0)
            continue
        total, s = None, rs
        while s < re:
            e = min(re, (s // ec + 1) * ec)
            sl = slice(base + s, base + e)
            part = np.add.accumulate(ns[sl, None] * H[indices[sl]], axis=0, dtype=np.float32)[-1]
            total = part if total is None else (total + part).astype(np.float32)
            s = e
        out[i] = rbf(nd[i] * total)
    return out


def small_multigraph():
    """(indptr int64 [61], indices int32 [E]): 60 nodes, a multigraph.  In-degrees 0, 1, 15, 16, 17, 31, 32, 33, 64, 65 on rows
    0 .. 9 (row 0 edgeless); row 12: source 40 five times (and two others); source 50 into rows 15 and 16 (one batch of 7) and
    row 21 (the next); a self loop on row 20; the last row edgeless.  Sources 40 and 50 appear nowhere else."""
    rng = np.random.RandomState(5)
    pool = np.array([j for j in range(60) if j not in (40, 50)])
    deg = {0: 0, 1: 1, 2: 15, 3: 16, 4: 17, 5: 31, 6: 32, 7: 33, 8: 64, 9: 65, 59: 0}
    rows = []
    for i in range(60):
        if i == 12:
            r = [40, 3, 40, 40, 7, 40, 40]
        elif i in (15, 16):
            r = [50, int(pool[i])]
        elif i == 21:
            r = [int(pool[4]), 50]
        elif i == 20:
            r = [20, 11, 2]
        else:
            r = list(rng.choice(pool, deg.get(i, int(rng.randint(0, 5))), replace=True))
        rows.append(r)
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    return indptr, np.array([j for r in rows for j in r], dtype=np.int32)


def full_neighbor_block(indptr, indices, b0, b1):
    """(src, dst, K, S, src_nid) of graph.full_neighbor_block: destinations first among the sources, the others in ascending id."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    e0, e1 = int(indptr[b0]), int(indptr[b1])
    col = indices[e0:e1]
    S = b1 - b0
    outside = (col < b0) | (col >= b1)
    others = np.unique(col[outside])
    src = np.where(outside, S + np.searchsorted(others, col), col - b0)
    dst = np.repeat(np.arange(S, dtype=np.int64), np.diff(indptr[b0:b1 + 1]))
    return src, dst, S + others.size, S, np.concatenate([np.arange(b0, b1), others])
