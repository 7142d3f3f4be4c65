"""The row kernels of csrc/spmm.hip (k_embed_norm, k_gather_rows_norm, k_sage_epilogue, k_sage_epilogue_bwd) restated in plain
numpy, plus the designed inputs the CPU and GPU suites share.  No GPU and no library is involved; imported
like bounds.py and mt_ref.py.

bf16 values travel as uint16 bit patterns (``bits``) or as torch.bfloat16 CPU tensors; every function takes either.

The summation-order contract: a bf16 row norm is  bf16(sqrtf(s))  with s the fp32 sum of the (exact) fp32 squares taken in one of
two orders, picked from how the rows are STORED -- ``norm_path(dim, stride, addr)``:
  "scalar": lane l of 64 adds columns l, l + 64, l + 128, ... in turn;
  "vec4":   lane l adds columns 4l, 4l + 1, 4l + 2, 4l + 3, then 4l + 256 ..., in turn;
then the xor butterfly s += s[lane ^ d] for d = 32, 16, 8, 4, 2, 1; lane 0 holds the sum.  Every kernel that promises
"bliss_embed_norm's bits" promises the order norm_path gives for the tensor it stores."""
import functools

import numpy as np

LANES = 64
BUTTERFLY = (32, 16, 8, 4, 2, 1)
U = 2.0 ** -24                              # fp32 unit roundoff
SENTINEL = 0xFFFF                           # a NaN no kernel here produces (f2bf writes 0x7FC0): an untouched output element
PAD = 2.0 ** 60                             # what lies between dim and stride of an input: its square alone is 2^120


# ------------------------------------------------------------------------------------------------------------ bf16 <-> numpy
def bits_of(t):
    """uint16 bit patterns of a torch.bfloat16 tensor (any device) or of an array that already holds them."""
    if isinstance(t, np.ndarray):
        assert t.dtype == np.uint16, t.dtype
        return t
    import torch
    return (t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int32) & 0xFFFF).astype(np.uint16)


def to_torch(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def f32_of(bits):
    return (np.asarray(bits).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f2bf(x):
    """common.cuh's f2bf on fp32: round to nearest even, every NaN becomes 0x7FC0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def rbf(x):
    return f32_of(f2bf(x))


def bf_bits(x):
    """The bf16 bit pattern of one number."""
    return int(f2bf(np.array([x], dtype=np.float32))[0])


def rbf64(x):
    """An fp64 value rounded ONCE to bf16's grid (8 significant bits, nearest even), as fp64.  For normal bf16 magnitudes; 2^128
    and above become inf."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.ldexp(np.rint(m * 256.0) / 256.0, e)
    r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


# ------------------------------------------------------------------------------------------------------------ the row norm
def norm_path(dim, stride, addr):
    """bliss_embed_norm's choice for rows of ``dim`` bf16 elements, ``stride`` elements apart, the first at byte address ``addr``."""
    return "vec4" if dim % 4 == 0 and stride % 4 == 0 and addr % 8 == 0 else "scalar"


def embed_norm_bits(h, path, butterfly=BUTTERFLY):
    """bf16 bits [n] of the row norms of h [n, dim] as k_embed_norm computes them on ``path``.  The squares of bf16 values are exact
    in fp32 (16 significant bits) wherever they are normal, so it does not matter whether the compiler fuses multiply and add.
    ``butterfly`` is the kernel's; the suite passes a shorter one to show what a skipped step does."""
    assert path in ("vec4", "scalar"), path
    x = f32_of(bits_of(h))
    n, dim = x.shape
    group = LANES * (4 if path == "vec4" else 1)
    steps = -(-dim // group)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq = np.zeros((n, max(steps, 1) * group), dtype=np.float32)      # (columns past dim: + 0.0f changes no non-negative sum)
        sq[:, :dim] = x * x
        s = np.zeros((n, LANES), dtype=np.float32)
        if path == "vec4":
            sq = sq.reshape(n, -1, LANES, 4)
            for j in range(sq.shape[1]):
                for i in range(4):
                    s = s + sq[:, j, :, i]
        else:
            sq = sq.reshape(n, -1, LANES)
            for j in range(sq.shape[1]):
                s = s + sq[:, j, :]
        lane = np.arange(LANES)
        for d in butterfly:
            s = s + s[:, lane ^ d]
        return f2bf(np.sqrt(s[:, 0]))


def norm_delta(dim):
    """The relative half-width of embed_norm_interval.

    u = 2^-24.  The squares are exact.  A lane adds its terms into 0.0f one by one: ceil(dim / 64) terms on the scalar path, 4 *
    ceil(dim / 256) <= ceil(dim / 64) + 3 on the vec4 path (dim > 256 (c - 1) gives ceil(dim / 64) >= 4c - 3).  The first add, 0 + t,
    is exact, so a term meets at most ceil(dim / 64) + 2 roundings in its lane and 6 more in the butterfly:
    k' = ceil(dim / 64) + 8 <= 104.  All terms are >= 0, so the computed sum is s (1 + t) with |t| <= (1 + u)^k' - 1 <= k' u +
    (k' u)^2.  sqrt is monotone and |sqrt(1 + t) - 1| <= |t| / 2 + t^2 / 2; sqrtf rounds once more (correctly rounded): the fp32
    norm is sqrt(s) (1 + e) with |e| <= k' u / 2 + u + 2 (k' u)^2.  The fp64 reference itself is off by at most dim * 2^-53
    relative, and forming ref * (1 +- delta) by 2^-52.  With k = k' + 1 the bound used,
        delta = (k / 2 + 1) u = ((ceil(dim / 64) + 9) / 2 + 1) * 2^-24,
    exceeds k' u / 2 + u by u / 2 = 3.0e-8, which covers the second-order terms (2 (104 u)^2 = 7.7e-11) and the reference's own
    error (6144 * 2^-53 + 2^-52 = 6.8e-13).  The last step, rounding to bf16, is monotone: lo <= x <= hi gives rbf(lo) <=
    rbf(x) <= rbf(hi), which is the check.

    Domain: every non-zero square and the sum of squares inside fp32's normal range, i.e. non-zero |elements| in [2^-63, 2^63] and
    a sum below 2^128.  Below it a square is no longer exact (it loses bits to the subnormal grid: a relative error up to 2^-17 at
    2^-133), above it the sum is inf.  Such rows are held to the restatement's bits only."""
    return ((-(-dim // LANES) + 9) / 2.0 + 1.0) * U


def embed_norm_interval(h):
    """(lo, hi), fp64 arrays [n] of bf16-representable values: the row norm of h [n, dim], computed in fp64, must land in
    rbf(ref (1 - delta)) .. rbf(ref (1 + delta)), delta = norm_delta(dim).  A row with inf gives (inf, inf), a row with NaN (nan,
    nan)."""
    x = f32_of(bits_of(h)).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        ref = np.sqrt((x * x).sum(axis=1))
        d = norm_delta(x.shape[1])
        return rbf64(ref * (1.0 - d)), rbf64(ref * (1.0 + d))


def assert_norms(got, rows, path, what, domain=None):
    """THE assertion the CPU and the GPU suite share: ``got`` (bf16 bits [n]) are the norms of ``rows`` (bits [n, dim]) on ``path``:
    bit-equal to the restatement, and inside embed_norm_interval on the rows of ``domain`` (a bool mask; None: all rows)."""
    got, rows = bits_of(got), bits_of(rows)
    want = embed_norm_bits(rows, path)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, path, "bits differ in %d rows, first %d: got %#06x want %#06x" % (bad.size, bad[0], got[bad[0]], want[bad[0]]))
    lo, hi = embed_norm_interval(rows)
    g = f32_of(got).astype(np.float64)
    dom = np.ones(len(g), bool) if domain is None else np.asarray(domain, bool)
    nan = np.isnan(lo)
    ok = np.where(nan, np.isnan(g), (lo <= g) & (g <= hi))
    bad = np.nonzero(dom & ~ok)[0]
    assert bad.size == 0, (what, path, "outside the interval in %d rows, first %d: %r not in [%r, %r]" % (bad.size, bad[0], g[bad[0]], lo[bad[0]], hi[bad[0]]))


# ------------------------------------------------------------------------------------------------------------ designed rows
N_DESIGNED = 18
N_DOMAIN = 15                               # designed rows 0 .. 14 lie in the interval's domain (inf and NaN rows included)


def designed_rows(dim, n=777, seed=0):
    """(bits [n, dim], domain mask [n]): the rows every shape is run on.
      0-3    randn                                   4-8   randn * 2^-30, 2^-15, 1, 2^15, 2^30
      9      zeros                                   10    only the LAST column non-zero
      11     only the last column of the last full group of 4 non-zero (column 0 when dim < 4)
      12     one element 2^10 among |randn| * 2^-12  13    randn with one inf: the norm is inf
      14     randn with one NaN: the norm is NaN
      15     all 2^63 (the sum overflows from dim 4)  16   all 2^64 (every square is inf)   17   all 2^-70 (squares 2^-140: subnormal)
      18-    randn * 2^k, k cycling through -30 .. 30
    Rows 15-17 are outside embed_norm_interval's domain (norm_delta): they are held to the restatement's bits only."""
    import torch
    gen = torch.Generator().manual_seed(7919 * dim + seed)
    n_all = max(n, N_DESIGNED)
    x = torch.randn(n_all, dim, generator=gen)
    for r, k in zip(range(4, 9), (-30, -15, 0, 15, 30)):
        x[r] *= 2.0 ** k
    x[9] = 0
    x[10] = 0
    x[10, dim - 1] = 1.75
    x[11] = 0
    x[11, max(dim // 4 * 4 - 1, 0)] = -2.5
    x[12] = x[12].abs() * 2.0 ** -12
    x[12, dim // 3] = 2.0 ** 10
    x[13, dim // 2] = float("inf")
    x[14, (2 * dim) // 3] = float("nan")
    x[15], x[16], x[17] = 2.0 ** 63, 2.0 ** 64, 2.0 ** -70
    if n_all > N_DESIGNED:
        k = (torch.arange(n_all - N_DESIGNED) * 7) % 61 - 30
        x[N_DESIGNED:] *= (2.0 ** k.double()).float()[:, None]
    dom = np.ones(n_all, bool)
    dom[15:18] = False
    return bits_of(x.bfloat16())[:n], dom[:n]


# which designed rows a launch of n rows sees: small launches start at the planted rows
START = {1: 10, 3: 9, 4: 14, 5: 9}


def rows_for(n_rows, bits, dom):
    s = START.get(n_rows, 0)
    return bits[s:s + n_rows], dom[s:s + n_rows]


# ------------------------------------------------------------------------------------------------------------ order-sensitive rows
def _to_midpoint(x, rng, passes=8):
    """Move single elements of the non-negative fp64 rows x [B, dim] (bf16-representable values) by bf16 steps until the fp64 norm
    sits on a bf16 rounding midpoint, as closely as single elements allow.  Returns (rows, relative distance of the sum of squares
    from the midpoint's square)."""
    B, dim = x.shape
    s = (x * x).sum(axis=1)
    nrm = np.sqrt(s)
    m, e = np.frexp(nrm)
    target = np.ldexp((np.floor(m * 256.0) + 0.5) / 256.0, e) ** 2         # the midpoint above bf16-floor(norm), squared
    rows = np.arange(B)
    for _ in range(passes):
        r = target - (x * x).sum(axis=1)                                   # what the sum of squares lacks
        cand = rbf64(np.sqrt(np.maximum(x * x + r[:, None], 0.0)))         # every element moved to absorb it, on bf16's grid
        left = np.abs(r[:, None] - (cand * cand - x * x))
        left[cand < 2.0 ** -40] = np.inf                                   # keep the squares far inside fp32's normal range
        j = left.argmin(axis=1)
        better = left[rows, j] < np.abs(r)
        x[rows[better], j[better]] = cand[rows[better], j[better]]
    return x, np.abs(target - (x * x).sum(axis=1)) / target


@functools.lru_cache(maxsize=None)
def _order_sensitive(dim, n, seed):
    rng = np.random.default_rng(1_000_003 * seed + dim)
    found = []
    base_rows = max(16, min(400, 600_000 // dim))
    for _ in range(40):
        # magnitudes over eight binades: the small elements are what the last passes of _to_midpoint tune with
        x = np.abs(rng.standard_normal((base_rows, dim))) * 2.0 ** -rng.integers(0, 8, (base_rows, dim))
        x = rbf64(np.maximum(x, 2.0 ** -20))
        x, dist = _to_midpoint(x, rng)
        x = x[dist < 2e-8]
        for _ in range(64):                                                # a permuted row has the same fp64 norm, other fp32 sums
            p = rng.permuted(x, axis=1)
            bits = f2bf(p.astype(np.float32))
            differ = embed_norm_bits(bits, "vec4") != embed_norm_bits(bits, "scalar")
            found.extend(bits[differ])
            if len(found) >= n:
                out = np.stack(found[:n])
                out.setflags(write=False)
                return out
    raise RuntimeError("order_sensitive_rows(%d, %d, %d): found only %d rows" % (dim, n, seed, len(found)))


def order_sensitive_rows(dim, n=8, seed=0):
    """bits [n, dim] of non-negative bf16 rows whose norm depends on the order: embed_norm_bits(rows, "vec4") !=
    embed_norm_bits(rows, "scalar") in every row.  dim must be a multiple of 4 (the vec4 order exists).  A seeded search, cached per
    (dim, n, seed): random rows are moved onto a bf16 rounding midpoint of the fp64 norm (_to_midpoint), then permuted until the two
    fp32 sums fall on different sides of it."""
    assert dim % 4 == 0 and dim >= 8, dim
    return _order_sensitive(int(dim), int(n), int(seed))


# ------------------------------------------------------------------------------------------------------------ dropout hash, epilogue
_M = np.uint64(0xFFFFFFFF)


def drop_hash(seed, ctr, idx):
    """common.cuh's drop_hash(seed, ctr, idx) on uint32 (idx an array), in uint64 arithmetic masked back to 32 bits."""
    idx = np.asarray(idx).astype(np.uint64) & _M
    seed, ctr = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64(int(ctr) & 0xFFFFFFFF)
    mul = lambda a, c: (a * np.uint64(c)) & _M
    x = (mul(idx, 0x9E3779B1) + seed) & _M
    x ^= (mul(ctr, 0x85EBCA77) + np.uint64(0x165667B1)) & _M
    x ^= x >> np.uint64(16); x = mul(x, 0x7FEB352D); x ^= x >> np.uint64(15); x = mul(x, 0x846CA68B); x ^= x >> np.uint64(16)
    x = (x + ctr) & _M; x ^= x >> np.uint64(15); x = mul(x, 0x2C1B3C6D); x ^= x >> np.uint64(12)
    return x.astype(np.uint32)


def drop_threshold(p):
    """The launcher's threshold: p arrives as a C float."""
    return int(float(np.float32(p)) * 4294967296.0) if p > 0 else 0


def drop_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)


def sage_epilogue_ref(a, b, p, seed, ctr, path=None):
    """k_sage_epilogue on a, b [n, dim]: (out bits [n, dim], mask bool [n, dim] -- True where the hash keeps the element, all True
    at p = 0 --, norm bits [n] on ``path``; None: norm_path of a contiguous aligned out).
    t = rbf(fp32 a + b);  t > 0 ? t : +0  (a NaN sum is NOT positive: it stores +0);  kept: rbf(t * fp32(1 / (1 - p)))."""
    A, B = f32_of(bits_of(a)), f32_of(bits_of(b))
    n, dim = A.shape
    with np.errstate(over="ignore", invalid="ignore"):
        t = rbf(A + B)
        t = np.where(t > 0, t, np.float32(0.0))
        keep = np.ones((n, dim), bool)
        if p > 0:
            idx = (np.arange(n, dtype=np.int64)[:, None] * dim + np.arange(dim, dtype=np.int64)[None, :]) & 0xFFFFFFFF
            keep = drop_hash(seed, ctr, idx) >= np.uint32(drop_threshold(p))
            t = np.where(keep, rbf(t * drop_scale(p)), np.float32(0.0))
    out = f2bf(t)
    return out, keep, embed_norm_bits(out, path or norm_path(dim, dim, 0))


def sage_epilogue_bwd_ref(dout, out, p):
    """k_sage_epilogue_bwd: bits of rbf(dout * fp32(1 / (1 - p))) where out > 0, else +0 (NaN and -0 in out are not positive)."""
    g, o = f32_of(bits_of(dout)), f32_of(bits_of(out))
    with np.errstate(over="ignore", invalid="ignore"):
        return f2bf(np.where(o > 0, g * drop_scale(p), np.float32(0.0)))
