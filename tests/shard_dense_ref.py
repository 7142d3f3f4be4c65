"""TEST SUPPORT: a plain host restatement of the static-shape sharded sampler's entry points (csrc/shard_dense.hip and their
routed twins in csrc/shard.hip), one function per entry point, built on the oracle's arithmetic (oracle/numerics.py,
oracle/bliss_oracle.py, both through the CPU test double tests/shard_cpu_ops.py).  Every result is an integer or a bf16 bit pattern:
the restatement is exact and the comparison (``compare``) knows no tolerance.

Also here, because the GPU module (tests/test_gpu_shard_dense_edges.py) and the CPU module (tests/test_shard_dense_ref.py, which
plants faults and shows that ``compare`` catches them) must use the SAME inputs: the generators of those inputs."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import numerics as nx
from shard_cpu_ops import OracleShardOps

ERR_CAP_CAND, ERR_CAP_KEPT, ERR_CAP_SEEDS, ERR_FLAG_TIMEOUT = 2, 4, 64, 256
SEED_MARK = 1 << 32
HIST_BINS = 32768
BLOCK = 1024                                                  # elements per look-back block (SD_TPB)
ONE = 0x3F80                                                  # bf16 1.0


def bits(t):
    """bf16 tensor -> int32 tensor of its 16 raw bits."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def canon_nan(b):
    """torch's CPU kernels leave the payload of a bf16 NaN to the code path (0x7fc0 from c10::BFloat16's scalar conversion, 0xffff
    from the vectorised one, the operand's own bits from torch.minimum).  The kernels promise the scalar form, 0x7fc0, for every
    NaN they compute (common.cuh:f2bf): the restatement's NaNs are brought to that pattern and the kernel must give exactly it."""
    return torch.where(((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0), torch.full_like(b, 0x7FC0), b)


def from_bits(b):
    return nx.bits_to_bf16(b.to(torch.int64))


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def scratch_words(num_nodes, cap_c):
    """64-bit words the two passes index: the candidate pass's status words, the kept pass's, one ticket."""
    return blocks(num_nodes) + blocks(cap_c) + 1


# ---------------------------------------------------------------------------------------------------------------- restatement
def local_seeds(seeds_g, n_seeds, lo, hi, cap_s):
    """bliss_shard_local_seeds.  ``n_seeds``: the count the kernel sees (host argument or *n_seeds_dev)."""
    err, S = 0, int(n_seeds)
    if S > cap_s:
        err, S = ERR_CAP_SEEDS, cap_s
    g = seeds_g[:S].to(torch.int32)
    pos = torch.nonzero((g >= lo) & (g < hi)).flatten().to(torch.int32)
    n = int(pos.numel())
    pad = int(seeds_g[0]) if S > 0 else lo
    seeds_l = torch.full((cap_s,), pad, dtype=torch.int32)
    seeds_l[:n] = g[pos.long()]
    seed_pos = torch.zeros(cap_s, dtype=torch.int32)
    seed_pos[:n] = pos
    return dict(seeds_l=seeds_l, seeds_l_copy=seeds_l[:n].clone(), seed_pos=seed_pos, n_local=n, err=err)   # (the copy gets no padding)


def scatter(seeds_l, seed_p2, n_local, touched_key, touched_sum, n_touched, V, dense=None):
    """bliss_shard_scatter_partials onto ``dense`` [V, 2] = (sum, mark) (zero when not given).  One writer per node."""
    dense = torch.zeros(V, 2, dtype=torch.int64) if dense is None else dense.clone()
    ids = torch.cat([seeds_l[:n_local].long(), (touched_key[:n_touched] & 0xFFFFFFFF).to(torch.int32).long()])
    sums = torch.cat([seed_p2[:n_local], touched_sum[:n_touched]])
    marks = torch.cat([torch.full((n_local,), SEED_MARK + 1, dtype=torch.int64), torch.ones(n_touched, dtype=torch.int64)])
    ok = (ids >= 0) & (ids < V)
    dense[ids[ok], 0] = sums[ok]
    dense[ids[ok], 1] = marks[ok]
    return dict(dense=dense, err=0 if bool(ok.all()) else ERR_CAP_CAND)


def importance(sums, uniform_nodes):
    """p of a list of Q.44 sums: OracleShardOps.importance (bandit_sampler.py:75, :79-81), as bf16 bits."""
    return canon_nan(bits(OracleShardOps.importance(SimpleNamespace(imp=not uniform_nodes), sums)))


def histogram(p_bits):
    return torch.bincount((p_bits & 0x7FFF).long(), minlength=HIST_BINS).to(torch.int32)


def candidates(dense, uniform_nodes, cap_c):
    """bliss_shard_candidates on ``dense`` [V, 2].  Lists hold the entries below cap_c only."""
    cand = torch.nonzero(dense[:, 1]).flatten()
    C_true = int(cand.numel())
    C = min(C_true, cap_c)
    cand = cand[:C]
    p = importance(dense[cand, 0], uniform_nodes)
    return dict(cand_nid=cand.to(torch.int32), p=p, is_seed=(dense[cand, 1] >= SEED_MARK).to(torch.uint8), hist=histogram(p),
                C=C, counts_err=0, iters=0, all_one=0, err=ERR_CAP_CAND if C_true > cap_c else 0, dense=torch.zeros_like(dense))


def scale(hist, n_cand, fanout, eps=0.9999):
    """bliss_poisson_scale: OracleShardOps.scale on the histogram -> (c, all_one, iters); the histogram is zero afterwards."""
    o = SimpleNamespace()
    OracleShardOps.scale(o, hist.long(), n_cand, fanout, eps)
    c, all_one, iters = OracleShardOps.scale_result(o)
    return dict(c=c, all_one=int(all_one), iters=iters, hist=torch.zeros_like(hist))


def inclusion(cand_nid, p_bits, is_seed, c, all_one, seed, step, layer):
    """P (bits) and the keep bits of a candidate list: OracleShardOps.keyed_select (= bliss_keyed_select, and the per-candidate
    part of bliss_shard_select_kept)."""
    o = SimpleNamespace(_c=c, _all_one=bool(all_one))
    P, keep = OracleShardOps.keyed_select(o, cand_nid, from_bits(p_bits), is_seed.bool(), seed, step, layer)
    return canon_nan(bits(P)), keep


def select_kept(cand_nid, p_bits, is_seed, C, c, all_one, seed, step, layer, seeds_g, S, cap_k, kept_map, n_local, bump_step):
    """bliss_shard_select_kept.  ``kept_map``: the map before the call ([V]); ``S``: the seed count the kernel sees."""
    cand, pb, sd = cand_nid[:C], p_bits[:C], is_seed[:C]
    P, keep = inclusion(cand, pb, sd, c, all_one, seed, step, layer)
    new = keep & ~sd.bool()
    kept = torch.cat([seeds_g[:S].to(torch.int32), cand[new]])
    prob = torch.cat([torch.full((S,), ONE, dtype=torch.int32), P[new]])
    K_true = int(kept.numel())
    K = min(K_true, cap_k)
    kept, prob = kept[:K], prob[:K]
    kept_map = kept_map.clone()
    kept_map[kept.long()] = torch.arange(K, dtype=torch.int32)
    return dict(P=P, kept_nid=kept, node_prob=prob, kept_map=kept_map, K=K, layer_C=int(n_local), err=ERR_CAP_KEPT if K_true > cap_k else 0,
                step=int(step) + (1 if bump_step else 0))


def pack_rows(nid, n_rows, lo, hi, table, row_len):
    """bliss_shard_pack_rows: [cap_rows, row_len] bits; rows i < n_rows that this rank owns = the table's, +0 elsewhere."""
    cap = int(nid.numel())
    out = torch.zeros(cap, row_len, dtype=torch.int32)
    i = torch.arange(cap)
    mine = (i < n_rows) & (nid >= lo) & (nid < hi)
    out[mine] = bits(table)[(nid[mine] - lo).long(), :row_len]
    return out


def place_rows(src, pos, n, cap_s, n_rows, row_len):
    """bliss_shard_place_rows: out[pos[j]] = src[j] for j < min(n, cap_s), +0 bits for every other row."""
    n = min(int(n), cap_s)
    out = torch.zeros(n_rows, row_len, dtype=torch.int32)
    out[pos[:n].long()] = bits(src)[:n, :row_len]
    return out


def take_rows(src, pos, n, cap_s, row_len):
    """bliss_shard_take_rows: out[j] = bf16(src[pos[j]]) for j < min(n, cap_s) (n None: cap_s), a +0 row where pos[j] is past the
    source's rows and for every row behind."""
    n = cap_s if n is None else min(int(n), cap_s)
    out = torch.zeros(cap_s, row_len, dtype=torch.int32)
    p = pos[:n].long()
    ok = (p >= 0) & (p < src.shape[0])
    rows = src[p[ok], :row_len]
    conv = bits(rows.to(torch.bfloat16))
    out[torch.nonzero(ok).flatten()] = canon_nan(conv) if src.dtype == torch.float32 else conv      # (bf16 rows are copied: any payload stays)
    return out


# ----------------------------------------------------------------------------------------------------------------- comparison
def compare(got, want):
    """THE comparison of the GPU module: every key of ``want`` against ``got``, integers only, no tolerance.  Returns the list of
    differences (empty = equal), each with the first differing index."""
    out = []
    for k, w in want.items():
        if k not in got:
            out.append(f"{k}: missing")
            continue
        g = got[k]
        if isinstance(w, torch.Tensor):
            g = torch.as_tensor(g)
            assert not w.dtype.is_floating_point and not g.dtype.is_floating_point, f"{k}: compare integer views"
            if g.shape != w.shape:
                out.append(f"{k}: shape {tuple(g.shape)} != {tuple(w.shape)}")
            elif not torch.equal(g.long(), w.long()):
                d = torch.nonzero((g.long() != w.long()).flatten()).flatten()
                i = int(d[0])
                out.append(f"{k}: {d.numel()} differ, first at {i}: got {int(g.flatten()[i])} want {int(w.flatten()[i])}")
        elif isinstance(w, float):
            if np.float64(g).tobytes() != np.float64(w).tobytes():
                out.append(f"{k}: got {g!r} want {w!r}")
        elif int(g) != int(w):
            out.append(f"{k}: got {int(g)} want {int(w)}")
    return out


def padded(values, length, sentinel):
    """The expected contents of an output buffer of ``length`` entries pre-filled with ``sentinel``: ``values``, then sentinels."""
    out = torch.full((length,) + tuple(values.shape[1:]), sentinel, dtype=values.dtype)
    out[: values.shape[0]] = values
    return out


# ------------------------------------------------------------------------------------------------------- inputs of the GPU tests
CAND_SIZES = [1, 1023, 1024, 1025, 64 * 1024, 64 * 1024 + 1, 65 * 1024 + 1, 129 * 1024 + 5, 232965]
CAND_BIG = 2449029
PATTERNS = ["all", "none", "first", "last", "one_per_block", "gap64", "gap65", "gap130", "random", "seed_boundary"]


def mark_mask(V, pattern, gen):
    """Which nodes are marked.  gapN: one full block, N empty blocks, the rest marked -- None when V has too few blocks."""
    nb = blocks(V)
    m = torch.zeros(V, dtype=torch.bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "first":
        m[0] = True
    elif pattern == "last":
        m[V - 1] = True
    elif pattern == "one_per_block":
        if nb < 2:
            return None
        off = torch.randint(0, BLOCK, (nb,), generator=gen)
        m[(torch.arange(nb) * BLOCK + off).clamp(max=V - 1)] = True
    elif pattern.startswith("gap"):
        gap = int(pattern[3:])
        if nb < gap + 2:
            return None
        first = (nb - gap - 2) // 2                              # the full block in front of the gap
        m[first * BLOCK: (first + 1) * BLOCK] = True
        m[(first + 1 + gap) * BLOCK:] = True
    elif pattern in ("random", "seed_boundary"):
        m = torch.rand(V, generator=gen) < 0.3
    elif pattern != "none":
        raise ValueError(pattern)
    return m


def make_dense(V, pattern, ranks, seed):
    """A dense [V, 2] buffer as it comes out of the all-reduce over ``ranks`` ranks: mark k for a node touched on k ranks,
    2^32 + k for a seed; sums 0 (some of them on seeds), 1, ordinary Q.44 values and values >= 2^46 (p >= 2: outside the LDS
    histogram window).  seed_boundary adds the marks 2^32 (a seed: >=) and 2^32 - 1 (none).  None: pattern impossible at V."""
    gen = torch.Generator().manual_seed(seed)
    m = mark_mask(V, pattern, gen)
    if m is None:
        return None
    k = torch.randint(1, ranks + 1, (V,), generator=gen)
    is_seed = torch.rand(V, generator=gen) < 0.1
    mark = torch.where(m, k + is_seed.long() * SEED_MARK, torch.zeros(V, dtype=torch.int64))
    kind = torch.randint(0, 8, (V,), generator=gen)
    ordinary = torch.randint(1 << 20, 1 << 44, (V,), generator=gen)
    big = torch.randint(1 << 46, 1 << 50, (V,), generator=gen)
    s = torch.where(kind == 0, torch.zeros_like(ordinary), torch.where(kind == 1, torch.ones_like(ordinary), torch.where(kind == 2, big, ordinary)))
    s = torch.where(m, s, torch.zeros_like(s))
    if pattern == "seed_boundary":
        idx = torch.nonzero(m).flatten()
        mark[idx[0::3]] = SEED_MARK
        mark[idx[1::3]] = SEED_MARK - 1
    return torch.stack([s, mark], dim=1).contiguous()


def cap_choices(C, V):
    """cap_c in {C, C - 1, 1, V}, deduplicated, positive."""
    return sorted({c for c in (C, C - 1, 1, V) if c >= 1})


def hand_list(C, V, S, seed):
    """A hand-made candidate list for bliss_shard_select_kept: C ascending node ids below V, p from a palette that holds 0, two NaN
    patterns, tiny, ordinary and > 1 values, S of the candidates as seeds in an order that is NOT ascending."""
    gen = torch.Generator().manual_seed(seed)
    cand = torch.sort(torch.randperm(V, generator=gen)[:C]).values.to(torch.int32)
    palette = torch.tensor([0x0000, 0x7FC0, 0xFFC0, 0x3480, 0x3C23, 0x3D80, 0x3E99, 0x3F00, 0x3F7F, 0x3F80, 0x4049, 0x0001], dtype=torch.int32)
    p = palette[torch.randint(0, palette.numel(), (C,), generator=gen)]
    spos = torch.randperm(C, generator=gen)[:S]
    if S > 1 and bool((spos[1:] > spos[:-1]).all()):
        spos = spos.flip(0)
    is_seed = torch.zeros(C, dtype=torch.uint8)
    is_seed[spos] = 1
    return cand, p, is_seed, cand[spos].clone()


def take_rows_f32_values():
    """fp32 values around bf16's rounding: exact ties towards even both ways, one fp32 ulp either side of a tie, +-inf, NaN, -0.0,
    fp32 subnormals, the largest finite float (rounds to inf)."""
    u = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000,
                  0x7F800000, 0xFF800000, 0x7FC00000, 0x80000000, 0x00000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x00008000,
                  0x00018000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x3F7FFFFF], dtype=np.uint32)
    return torch.from_numpy(u.view(np.float32).copy())


# ------------------------------------------------------------------------- what the GPU tests expect in their (over-long) buffers
TAIL = 37                                                     # entries behind every output's capacity; they must keep the sentinel
SENT = dict(cand_nid=-7, p=0x5A5A, is_seed=0xEE, P=0x6B6B, kept_nid=-9, node_prob=0x4C4C, kept_map=-1)


def want_candidates(dense, uniform_nodes, cap_c):
    """The contents of every buffer after bliss_shard_candidates, sentinels included, and the counts / error words."""
    r = candidates(dense, uniform_nodes, cap_c)
    for k in ("cand_nid", "p", "is_seed"):
        r[k] = padded(r[k].to(torch.int32), cap_c + TAIL, SENT[k])
    return r


def want_select(cand_nid, p_bits, is_seed, C, c, all_one, seed, step, layer, seeds_g, S, cap_k, cap_c, V, n_local, bump_step):
    """The contents of every buffer after bliss_shard_select_kept (kept_map pre-filled with -1, TAIL entries behind V)."""
    r = select_kept(cand_nid, p_bits, is_seed, C, c, all_one, seed, step, layer, seeds_g, S, cap_k,
                    torch.full((V + TAIL,), -1, dtype=torch.int32), n_local, bump_step)
    r["P"] = padded(r["P"], cap_c + TAIL, SENT["P"])
    r["kept_nid"] = padded(r["kept_nid"], cap_k + TAIL, SENT["kept_nid"])
    r["node_prob"] = padded(r["node_prob"], cap_k + TAIL, SENT["node_prob"])
    return r


def row_case(D, seed, cap=40, n_table=64, lo=1000):
    """Inputs of the row kernels' tests at row length D: a bf16 table of n_table owned rows (node ids lo .. lo + n_table) that holds
    -0.0, an id list with entries on lo, hi - 1, hi, lo - 1 and padding rows whose id IS owned."""
    gen = torch.Generator().manual_seed(seed)
    hi = lo + n_table
    table = torch.randn(n_table, D, generator=gen).bfloat16()
    table[:, 0] = -0.0
    nid = torch.randint(lo - 20, hi + 20, (cap,), generator=gen).to(torch.int32)
    nid[:4] = torch.tensor([lo, hi - 1, hi, lo - 1], dtype=torch.int32)
    nid[cap - 6:] = lo + 3                                    # (padding rows when n_rows < cap: an owned id)
    return dict(table=table, nid=nid, lo=lo, hi=hi, cap=cap)
