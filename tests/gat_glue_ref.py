"""NumPy restatement of csrc/gat_glue.hip: the glue around a GATv2 layer's message passing -- residual
add, ELU, flatten / head mean, keyed dropout -- with the bf16 rounding points and the mask of the kernels.  Values travel as
float32 arrays that hold bf16 numbers; nothing here imports the package."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def rbf(x):
    """float32 -> nearest-even bf16 -> float32 (finite inputs)."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def drop_hash(seed, ctr, idx):
    """drop_hash of csrc/spmm.hip on uint32 (computed in uint64, masked after every step)."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed, ctr = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64(int(ctr) & 0xFFFFFFFF)
    x = (idx * np.uint64(0x9E3779B1) + seed) & M32
    x ^= (ctr * np.uint64(0x85EBCA77) + np.uint64(0x165667B1)) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    x = (x + ctr) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x2C1B3C6D)) & M32
    x ^= x >> np.uint64(12)
    return x


def drop_threshold(p):
    return int(float(np.float32(p)) * 4294967296.0)


def keep_mask(rows, width, p, seed, ctr):
    """bool [rows, width]: element (r, c) is kept iff hash(seed, ctr, r * width + c) >= p * 2^32 -- a function of the element's
    position in the logical [rows, width] tensor, of nothing else."""
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    return drop_hash(seed, ctr, idx & M32) >= np.uint64(drop_threshold(p))


def drop_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _preact(rst, res):
    x = np.asarray(rst, dtype=np.float32)
    return x if res is None else rbf(x + np.asarray(res, dtype=np.float32))


def _elu(x):
    neg = rbf(np.expm1(x.astype(np.float64)).astype(np.float32))
    return np.where(x <= 0, neg, x).astype(np.float32)


def _head_sum(y):
    """[n, H, D] -> [n, D]: four running fp32 sums (head h into sum h & 3) combined in order -- the sequential sum up to four heads."""
    n, H, D = y.shape
    acc = np.zeros((4, n, D), dtype=np.float32)
    for h in range(H):
        acc[h & 3] = acc[h & 3] + y[:, h]
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def glue_fwd(rst, res, H, D, act, head_mean, p=0.0, seed=0, ctr=0, n_live=None):
    """(out, pre) [rows, width]: rows >= n_live are zeros and their inputs are not looked at."""
    rows = rst.shape[0]
    n = rows if n_live is None else max(0, min(int(n_live), rows))
    width = D if head_mean else H * D
    out, pre = np.zeros((rows, width), np.float32), np.zeros((rows, width), np.float32)
    x = _preact(rst[:n], None if res is None else res[:n])
    y = _elu(x) if act else x
    if head_mean:
        z = rbf(_head_sum(y.reshape(n, H, D)) * (np.float32(1.0) / np.float32(H)))
    else:
        z = y
    pre[:n] = z
    if p > 0:
        keep = keep_mask(rows, width, p, seed, ctr)[:n]
        z = np.where(keep, rbf(z * drop_scale(p)), np.float32(0))
    out[:n] = z
    return out, pre


def glue_bwd(dout, rst, res, H, D, act, head_mean, p=0.0, seed=0, ctr=0, n_live=None):
    """din [rows, H*D], the gradient w.r.t. rst (and res)."""
    rows = dout.shape[0]
    n = rows if n_live is None else max(0, min(int(n_live), rows))
    width = D if head_mean else H * D
    din = np.zeros((rows, H * D), np.float32)
    g = np.asarray(dout[:n], dtype=np.float32)
    if p > 0:
        keep = keep_mask(rows, width, p, seed, ctr)[:n]
        g = np.where(keep, rbf(g * drop_scale(p)), np.float32(0))
    if head_mean:
        g = np.tile(rbf(g * (np.float32(1.0) / np.float32(H))), (1, H))
    if act:
        x = _preact(rst[:n], None if res is None else res[:n])
        g = np.where(x <= 0, rbf((g.astype(np.float64) * np.exp(x.astype(np.float64))).astype(np.float32)), g)
    din[:n] = g
    return din


def head_mean(e):
    """a_ij [B] from the logits [B, H]."""
    e = np.asarray(e, dtype=np.float32)
    return rbf(_head_sum(e[:, :, None])[:, 0] * (np.float32(1.0) / np.float32(e.shape[1])))
