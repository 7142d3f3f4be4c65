"""CPU reference and case builders for the EXP3 exact row sum and its bf16 norm (csrc/exp3.hip).

The reference does not follow the kernel's algorithm: a bf16 pattern is an exact ``fractions.Fraction``; the norm is the
NEAREST entry of the ascending table of all non-negative finite bf16 values (bisection, ties to the even last mantissa
bit), not a shift and a mask; the row sum is ``sum(floor(value * 2**64))`` over Python ints.  Element arithmetic is
torch's own CPU bf16 arithmetic.  Every comparison made with these is an equality of bits or of Python ints.

The fixed point: value * 2**64 in three signed limbs of 32-bit digits, SLOTS replicas, a
term truncated PER TERM below 2**-64, terms of 2**24 and more refused (BLISS_ERR_FIXED_RANGE)."""
import bisect
import functools
import random
from fractions import Fraction

import torch

SLOTS = 32                      # BLISS_ROWSUM_SLOTS
ERR_NONFINITE, ERR_FIXED_RANGE = 16, 32
TOP = 0x4b7f                    # the largest pattern below 2**24 (row_digits: shift <= 80)
ONE = 0x3f80
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value(bits: int) -> Fraction:
    """A finite bf16 pattern as an exact Fraction (subnormals included)."""
    bits &= 0xffff
    s, e, m = bits >> 15, (bits >> 7) & 0xff, bits & 0x7f
    if e == 255:
        raise ValueError("non-finite bf16 pattern 0x%04x" % bits)
    v = Fraction(m, 128) * Fraction(2) ** -126 if e == 0 else (1 + Fraction(m, 128)) * Fraction(2) ** (e - 127)
    return -v if s else v


_TABLE = [value(b) for b in range(0x7f80)]          # pattern order is value order for non-negative patterns


def nearest_bf16(x) -> int:
    """The pattern of the bf16 nearest to ``x`` >= 0 (ties: even last mantissa bit)."""
    x = Fraction(x)
    if x < 0 or x > _TABLE[-1]:
        raise OverflowError("outside the finite non-negative bf16 range")
    hi = bisect.bisect_left(_TABLE, x)
    if _TABLE[hi] == x:
        return hi
    lo = hi - 1
    below, above = x - _TABLE[lo], _TABLE[hi] - x
    if below != above:
        return lo if below < above else hi
    return lo if lo % 2 == 0 else hi


@functools.lru_cache(maxsize=None)
def term(bits: int) -> int:
    """floor(value * 2**64) of one non-negative finite pattern."""
    v = value(bits)
    if v < 0:
        raise ValueError("negative weight 0x%04x" % bits)
    return (v * 2 ** 64).__floor__()


def pattern_list(row) -> torch.Tensor:
    """bf16 tensor (or integer patterns) -> int64 patterns 0 .. 65535."""
    row = torch.as_tensor(row)
    if row.dtype == BF:
        row = row.contiguous().view(torch.int16)
    return row.to(torch.int64).flatten() & 0xffff


def exact_sum(row) -> int:
    """sum(floor(value(b) * 2**64)) over the row, a Python int: the truncation is per term."""
    counts = torch.bincount(pattern_list(row), minlength=1 << 16)
    return sum(int(counts[b]) * term(b) for b in torch.nonzero(counts).flatten().tolist())


def limb_value(t) -> int:
    """l0 + (l1 << 32) + (l2 << 64), summed over the replicas of a [3 * SLOTS] int64 tensor."""
    total = 0
    for l0, l1, l2 in t.detach().cpu().view(SLOTS, 3).tolist():
        total += l0 + (l1 << 32) + (l2 << 64)
    return total


def bf(bits) -> torch.Tensor:
    """integer patterns -> bf16 tensor."""
    b = torch.as_tensor(bits, dtype=torch.int64) & 0xffff
    return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(BF)


def bits_of(x: torch.Tensor) -> torch.Tensor:
    return pattern_list(x.detach().cpu()).view(x.shape)


def quotient(x: torch.Tensor, norm_bits: int) -> torch.Tensor:
    """F.normalize's element: x / max(norm, 1e-12) on bf16 tensors (x itself where the norm is 1.0: the pass is skipped)."""
    if norm_bits == ONE:
        return x.clone()
    return x / bf([norm_bits]).clamp_min(1e-12)


def below_2_24(x: torch.Tensor) -> torch.Tensor:
    return torch.isfinite(x.float()) & (x.float() >= 0) & (x.float() < 2.0 ** 24)


# ---------------------------------------------------------------------------------------------------------------------
# limb encodings
# ---------------------------------------------------------------------------------------------------------------------
def encode_canonical(t: int) -> torch.Tensor:
    """``t`` as 32-bit digits in replica 0 (a negative t: its negated digits, negated)."""
    out = torch.zeros(3 * SLOTS, dtype=torch.int64)
    s, a = (-1 if t < 0 else 1), abs(t)
    out[0], out[1], out[2] = s * (a & 0xffffffff), s * ((a >> 32) & 0xffffffff), s * (a >> 64)
    return out


def encode_scattered(t: int, rng: random.Random) -> torch.Tensor:
    """``t`` spread over all replicas: signed entries far outside 32 bits, every one below 2**56 in magnitude (so that
    the int64 sum of a limb over the 32 replicas, < 2**61, cannot wrap), summing to ``t``."""
    rows = [[0, 0, 0]] + [[rng.randrange(-2 ** 55, 2 ** 55), rng.randrange(-2 ** 55, 2 ** 55), rng.randrange(-2 ** 40, 2 ** 40)]
                          for _ in range(SLOTS - 1)]
    rest = t - sum(a + (b << 32) + (c << 64) for a, b, c in rows)          # |rest| < 2**110
    l2 = rest >> 64                                                         # floor: the remainder is in [0, 2**64)
    rem = rest - (l2 << 64)
    rows[0] = [rem & 0xffffffff, rem >> 32, l2]
    assert all(abs(v) < 2 ** 56 for r in rows for v in r)
    rng.shuffle(rows)
    out = torch.tensor(rows, dtype=torch.int64).flatten()
    assert limb_value(out) == t
    return out


# ---------------------------------------------------------------------------------------------------------------------
# A. k_row_sum / row_digits
# ---------------------------------------------------------------------------------------------------------------------
def row_a() -> torch.Tensor:
    """Every pattern 0x0000 .. TOP, ascending and then descending (int64 patterns)."""
    up = torch.arange(0, TOP + 1, dtype=torch.int64)
    return torch.cat([up, up.flip(0)])


ROW_A_BYTE_OFFSETS = (0, 2, 10)
ROW_A_LENGTHS = (1, 63, 64, 65, 2047, 2048, 2049)
ROW_A_BIG = 300_000             # copies of TOP: the top limb passes 32 bits, all replicas carry it


def spread(row: torch.Tensor, n: int) -> torch.Tensor:
    """``n`` elements of ``row`` at even spacing (all of its exponents stay represented)."""
    idx = (torch.arange(n, dtype=torch.int64) * row.numel()) // n
    return row[idx]


# ---------------------------------------------------------------------------------------------------------------------
# B. limbs_to_bf16
# ---------------------------------------------------------------------------------------------------------------------
B_Q = (128, 129, 254, 255)
B_MSB = (8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 100, 104)
B_SMALL = (1, 2, 3, 255, 256, 257, 511, 513)
B_RANDOM, B_SEED = 2000, 20240229


def totals_b():
    """The totals of part B, in a fixed order."""
    out = []
    for q in B_Q:
        for msb in B_MSB:
            sh = msb - 7
            half = 1 << (sh - 1)
            for r in (0, half - 1, half, half + 1, 2 * half - 1):
                out.append((q << sh) + r)
    out += list(B_SMALL) + [1 << 64, 0]
    rng = random.Random(B_SEED)
    for _ in range(B_RANDOM):
        n = rng.randint(1, 104)
        out.append(rng.getrandbits(n) | (1 << (n - 1)) | 1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# C. the F.normalize pass
# ---------------------------------------------------------------------------------------------------------------------
NORMS_C = (1.0078125, 0.99609375, 113988365.0, 2.0 ** -20, 3.0, 2.0 ** -60, 2.0 ** 59, 0.0, 1.0, 0.5, 1.9921875)
SMALL_NORMS_C = tuple(x for x in NORMS_C if x < 1.0)
OFFSETS_C = (0, 1, 5)
LENGTHS_C = (1, 7, 8, 9, 2047, 2048, 2049, 6149)
LENGTH_NORMS_C = (1.0078125, 2.0 ** -20, 3.0)


def norm_bits(norm: float) -> int:
    return int(bits_of(torch.tensor([norm], dtype=torch.float32).bfloat16())[0])


def norm_total(nb: int) -> int:
    """The exact bf16 norm as a total (value * 2**64)."""
    t = value(nb) * 2 ** 64
    assert t.denominator == 1
    return int(t)


def filtered(nb: int) -> torch.Tensor:
    """The patterns 0 .. TOP whose quotient by the norm is finite and below 2**24, ascending."""
    pats = torch.arange(0, TOP + 1, dtype=torch.int64)
    return pats[below_2_24(quotient(bf(pats), nb))]


def row_c(nb: int) -> torch.Tensor:
    f = filtered(nb)
    return torch.cat([f, f.flip(0)])


def classes_c(x_bits: torch.Tensor, nb: int) -> dict:
    """Masks of the classes of elements the pass treats differently."""
    q = bits_of(quotient(bf(x_bits), nb))
    xf, qf = x_bits >> 7, q >> 7
    return dict(zero=x_bits == 0,
                subnormal_input=(xf == 0) & (x_bits != 0),
                subnormal_quotient=(qf == 0) & (x_bits != 0),
                table_slow_sum=(xf >= 2) & (qf >= 1) & ((qf < 70) | (qf > 125)),
                pair=(xf >= 2) & (qf >= 70) & (qf <= 125))


def subnormal_quotient_possible(nb: int) -> bool:
    """The smallest positive input, 2**-133, has a quotient below the smallest normal 2**-126 iff the divisor
    max(norm, bf16(1e-12)) is above 2**-7 (a norm of 1.0 leaves the subnormal inputs themselves)."""
    denom = max(value(nb), value(int(bits_of(torch.tensor([1e-12]).bfloat16())[0])))
    return denom > Fraction(1, 128)


def interleaved_c(nb: int) -> torch.Tensor:
    """(in-range normal, zero or subnormal) pairs and then the same the other way round: one half of a 32-bit word can
    take the table, the other forces the division."""
    f = filtered(nb)
    inr = f[classes_c(f, nb)["pair"]]
    low = torch.arange(inr.numel(), dtype=torch.int64) % 0x80          # 0x0000 .. 0x007f
    return torch.cat([torch.stack([inr, low], 1).flatten(), torch.stack([low, inr], 1).flatten()])


def out_of_range_c(nb: int) -> torch.Tensor:
    """A short in-range row with ONE element, in the middle, whose quotient reaches 2**24 (and is finite)."""
    pats = torch.arange(0, TOP + 1, dtype=torch.int64)
    q = quotient(bf(pats), nb).float()
    over = pats[torch.isfinite(q) & (q >= 2.0 ** 24)]
    row = spread(filtered(nb), 600)
    return torch.cat([row[:300], over[:1], row[300:]])


def chained_reference(row_bits: torch.Tensor, calls: int):
    """[(norm pattern, row patterns)] after each of ``calls`` F.normalize calls, every norm from the exact sum of the row
    the call before it left."""
    out, x = [], bf(row_bits)
    for _ in range(calls):
        nb = nearest_bf16(Fraction(exact_sum(x), 2 ** 64))
        x = quotient(x, nb)
        out.append((nb, bits_of(x)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# D. incremental deltas
# ---------------------------------------------------------------------------------------------------------------------
FACTORS_D = (1.0, 0.5, 2.0 ** -40, 1.0078125, 3.0, 0.0, 2.0 ** -133)


def apply_case():
    """(row patterns, positions, factors bf16): the row of A, one factor per position in a cycle, only the positions
    whose product stays below 2**24."""
    row = row_a()
    fac = torch.tensor(FACTORS_D, dtype=torch.float32).bfloat16()[torch.arange(row.numel()) % len(FACTORS_D)]
    keep = below_2_24(bf(row) * fac)
    pos = torch.nonzero(keep).flatten()
    return row, pos.to(torch.int32), fac[pos]


def ranks_case():
    """Two ranks, two blocks: every list is a stretch of apply_case's positions, the stretches of the two ranks overlap
    (identical positions) and are contiguous (neighbours share a 32-bit word).  Only positions whose weight stays below
    2**24 after either rank.  Returns (row patterns [2, E], lists[rank][block] = (pos, fac), expected patterns [2, E])."""
    row, pos, fac = apply_case()
    w = bf(row)
    ok = below_2_24(w * torch.tensor(3.0).bfloat16() * torch.tensor(3.0).bfloat16())
    sel = ok[pos.long()]
    pos, fac = pos[sel], fac[sel]
    n = pos.numel()
    cut = {(0, 0): (0, 9000), (1, 0): (4001, 13000), (0, 1): (n - 9001, n), (1, 1): (n - 12000, n - 3000)}
    lists = [[None, None], [None, None]]
    want = torch.stack([w, w]).clone()
    for r in range(2):
        for b in range(2):
            lo, hi = cut[(r, b)]
            # the second rank meets the factors one step on in the cycle, so that its products differ from the first's
            f = fac[lo:hi] if r == 0 else torch.roll(fac, 1)[lo:hi]
            lists[r][b] = (pos[lo:hi].clone(), f.clone())
    for r in range(2):                                                      # rank after rank: bf16 products do not commute
        for b in range(2):
            p, f = lists[r][b]
            want[b, p.long()] = want[b, p.long()] * f
    assert bool(below_2_24(want).all())
    return torch.stack([row, row]), lists, bits_of(want)


# ---------------------------------------------------------------------------------------------------------------------
# E. the reward chain of k_exp3_update
# ---------------------------------------------------------------------------------------------------------------------
E_LISTS = dict(alpha=(0.0, 2.0 ** -70, 0.0039, 1.0, 1.0078125, 255.0, 3e19),
               k_i=(1, 2, 3, 255, 257, 383, 385, 1025),
               q_ij=(0.0, 2.0 ** -70, 2.0 ** -20, 0.5, 1.0, 1.0078125),
               embed_norm=(0.0, 2.0 ** -70, 1.0, 181.0, 1.8e19),
               node_prob=(0.0, 2.0 ** -126, 2.0 ** -20, 0.33, 1.0),
               # (the last one is an addition to the issue's list: int -> float lands on a bf16 tie, 2^25 + 2^17, which then goes to
               # the even 2^25, while the integer itself is nearer to 2^25 + 2^18 -- the only entry that a single rounding moves)
               n_i=(1, 3, 257, 65537, 2 ** 24 + 1, 2 ** 25 + 3, 2 ** 25 + 2 ** 17 + 1),
               delta=(0.01, 1.0),
               w_old=(2.0 ** -70, 1.0 / 3.0, 1.0, 2.0 ** 23 / 1.5))
E_NEUTRAL = dict(alpha=1.0, k_i=1, q_ij=1.0, embed_norm=1.0, node_prob=1.0, n_i=1, delta=1.0, w_old=1.0)
E_COMBOS, E_SEED = 4096, 77


def update_cases():
    """One dict of operands per case: each operand swept over its list with the others at 1, then E_COMBOS draws."""
    cases = []
    for name, vals in E_LISTS.items():
        for v in vals:
            cases.append(dict(E_NEUTRAL, **{name: v}))
    rng = random.Random(E_SEED)
    for _ in range(E_COMBOS):
        cases.append({name: rng.choice(vals) for name, vals in E_LISTS.items()})
    return cases


class UpdateBlock:
    """The cases of ONE delta as a block: every case is an edge with a source node of its own (embed_norm and node_prob
    are per source), and sits in a destination whose block in-degree is the case's k_i (real edges: filler edges with
    neutral operands complete a destination) and whose graph node has in-degree n_i (only the graph's indptr exists).
    Positions in the weight row are a fixed shuffle, so that neighbouring edges do not rewrite neighbouring weights."""

    def __init__(self, cases, delta, neutralise=None):
        self.delta = delta
        groups = {}
        for c in cases:
            groups.setdefault((c["k_i"], c["n_i"]), []).append(c)
        n_list = list(E_LISTS["n_i"])
        self.g_indptr = torch.tensor([0] + n_list, dtype=torch.int64).cumsum(0)
        edges, dst_nid, indptr = [], [], [0]
        for (k, n), cs in sorted(groups.items()):
            cs = cs + [dict(E_NEUTRAL, k_i=k, n_i=n, filler=True)] * (-len(cs) % k)
            for d in range(len(cs) // k):
                edges += cs[d * k:(d + 1) * k]
                dst_nid.append(n_list.index(n))
                indptr.append(len(edges))
        B = self.B = len(edges)
        self.is_case = torch.tensor([not c.get("filler", False) for c in edges])
        if neutralise is not None:                  # same block, the marked edges' operands replaced by the neutral ones
            edges = [dict(E_NEUTRAL, k_i=c["k_i"], n_i=c["n_i"]) if neutralise[i] else c for i, c in enumerate(edges)]
        col = lambda name: torch.tensor([c[name] for c in edges], dtype=torch.float32).bfloat16()
        self.alpha, self.q_ij, self.embed_norm, self.node_prob, self.w_old = (col(n) for n in ("alpha", "q_ij", "embed_norm", "node_prob", "w_old"))
        self.indptr = torch.tensor(indptr, dtype=torch.int64)
        self.dst = torch.repeat_interleave(torch.arange(len(dst_nid)), self.indptr[1:] - self.indptr[:-1])
        self.src = torch.arange(B, dtype=torch.int64)
        self.dst_nid = torch.tensor(dst_nid, dtype=torch.int64)
        self.E = B + 37                             # the row is a little longer than the block
        self.pos = torch.randperm(self.E, generator=torch.Generator().manual_seed(5))[:B]
        self.row = torch.full((self.E,), 2.0 ** -12, dtype=BF)
        self.row[self.pos] = self.w_old
        self.edge_w = torch.ones(self.E, dtype=BF)  # alpha by position, for the launch that reads edge_w[pos]
        self.edge_w[self.pos] = self.alpha

    def oblock(self):
        from oracle import bliss_oracle as bo
        return bo.OBlock(n_src=self.B, n_dst=self.dst_nid.numel(), indptr=self.indptr, src=self.src, dst=self.dst, eid=self.pos,
                         edge_weights=torch.ones(self.B, dtype=BF), q_ij=self.q_ij, node_prob=self.node_prob, src_nid=self.src,
                         dst_nid=self.dst_nid)

    def csc(self):
        from oracle import bliss_oracle as bo
        return bo.CSC(self.g_indptr, torch.zeros(0, dtype=torch.int32))

    def reference(self, row=None):
        """(rewards, factors, new row, intermediates), from ``row`` if given instead of the block's own:
        oracle.bliss_oracle.exp3_rewards, then the statements of exp3_update_row up to the weight update, copied one by
        one (the oracle's function goes on to the norm, which refuses the non-finite weights that some of these cases
        are there to produce)."""
        from oracle import bliss_oracle as bo
        blk, g = self.oblock(), self.csc()
        rewards = bo.exp3_rewards(blk, self.alpha, self.embed_norm)
        n_i = g.in_degrees()[blk.dst_nid].to(torch.int32).bfloat16()          # :223
        r_hat = rewards / blk.node_prob[blk.src]                              # :240 e_div_u
        d_r = r_hat * (self.delta / n_i)[blk.dst]                             # :242 e_mul_v
        d_r = d_r.clone()
        d_r[d_r > 1] = 1                                                      # :244
        ex = torch.exp(d_r)                                                   # :246
        row = (self.row if row is None else row).clone()
        row[blk.eid] = row[blk.eid] * ex                                      # :248
        return rewards, ex, row, dict(alpha2_over_k=(self.alpha ** 2) / (blk.indptr[1:] - blk.indptr[:-1]).to(torch.int32).bfloat16()[blk.dst],
                                      r_hat=r_hat, d_r_unclamped=r_hat * (self.delta / n_i)[blk.dst], d_r=d_r)


@functools.lru_cache(maxsize=None)
def update_blocks():
    """{delta: (block of all cases, the same block with the cases whose new weight is not finite neutralised)}."""
    out = {}
    for delta in E_LISTS["delta"]:
        cases = [c for c in update_cases() if c["delta"] == delta]
        full = UpdateBlock(cases, delta)
        row = full.reference()[2]
        bad = ~torch.isfinite(row.float())[full.pos]
        out[delta] = (full, UpdateBlock(cases, delta, neutralise=bad.tolist()))
    return out


def same_bits_or_nan(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise: equal patterns, or both NaN."""
    return (bits_of(a) == bits_of(b)) | (torch.isnan(a.float().cpu()) & torch.isnan(b.float().cpu()))


# ---------------------------------------------------------------------------------------------------------------------
# F. normalized_edata
# ---------------------------------------------------------------------------------------------------------------------
DEGREES_F = (0, 1, 2, 3, 127, 129, 255, 257, 383, 385, 1023, 1025, 65537)
