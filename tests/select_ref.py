"""TEST SUPPORT: a plain host restatement of the candidate -> kept stage of the single-GPU LADIES / bandit samplers
(csrc/sampler.hip: k_poisson_scale, k_select_fused / k_select_keyed, k_mn_prepare / k_mn_mark / k_mn_copy_p / k_mn_select), one
function per entry point, on CPU tensors.  Built on oracle.bliss_oracle.poisson_scale's text, poisson_draw and keyed_uniform and
on oracle.numerics; inputs are bit patterns (bf16 as int32 values 0 .. 0xffff).  Every result is an integer or a bf16 pattern (c:
a double compared by its bytes), so ``compare`` knows no tolerance.

Also here, because the GPU module (tests/test_gpu_select_edges.py) and the CPU module (tests/test_select_ref.py, which pins the
restatement, checks the exact-sum condition of every input and plants faults) must use the SAME inputs: the generator of those
inputs (``make_list`` and the case tables), and a structural model of select_fused_body (``model_select``)."""
import math

import numpy as np
import torch

from oracle import bliss_oracle as bo
from oracle import numerics as nx

ERR_CAP_CAND, ERR_CAP_KEPT = 2, 4
CHUNK = 1024                                                  # candidates per look-back chunk (TPB * ITEMS)
WAVES, ITEMS, LANES = 4, 4, 64                                # a chunk: 4 waves x 4 items x 64 lanes, in index order
ROUND = 64                                                    # predecessors per look-back round
SEL_AGG, SEL_PFX = 1, 2
ONE = 0x3F80                                                  # bf16 1.0
NAN = 0x7FC0
HIST_BINS = 32768
HWIN_LO, HWIN_N = 0x3000, 4096                                # k_cand_number's LDS window of the histogram


def bits(t):
    """bf16 tensor -> int32 tensor of its 16 raw bits."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def canon_nan(b):
    """torch's CPU kernels leave the payload of a bf16 NaN to the code path; the kernels promise 0x7fc0
    for every NaN they compute (common.cuh:f2bf).  The restatement's NaNs are brought to that pattern."""
    return torch.where(((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0), torch.full_like(b, NAN), b)


def from_bits(b):
    return nx.bits_to_bf16(b.to(torch.int64))


def chunks(n):
    return (n + CHUNK - 1) // CHUNK


def histogram(p_bits, C):
    """ws->hist as bliss_frontier_prob leaves it: the count of every pattern of p over [0, C)."""
    return torch.bincount(p_bits[:C].long(), minlength=HIST_BINS).to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- restatement
def _terms(c):
    """min(p * c, 1) for every non-negative bf16 pattern, in torch's own arithmetic (bandit_sampler.py:397): bf16 [32768]."""
    vals = from_bits(torch.arange(HIST_BINS))
    return torch.minimum(vals * c, torch.ones_like(vals))


def scale_trace(p_bits, C, fanout, eps=0.9999):
    """bo.poisson_scale's loop (bandit_sampler.py:391-401) with the sum of :397 computed EXACTLY (math.fsum over count x term,
    each product exact in a double) -> (c, iters, all_one, per-iteration list of (c, nonzero term values fp64, their counts))."""
    if C <= fanout:                                                               # :392
        return 1.0, 0, 1, []
    cnt = histogram(p_bits, C).to(torch.float64)
    nz = torch.nonzero(cnt).flatten()
    c, iters, trace = 1.0, 0, []
    for _ in range(50):                                                           # :396
        t = _terms(c)[nz].to(torch.float64)
        trace.append((c, t, cnt[nz]))
        S = math.fsum((t * cnt[nz]).tolist())                                     # :397
        iters += 1
        if min(S, fanout) / max(S, fanout) >= eps:                                # :398
            break
        c *= fanout / S                                                           # :401
    if c != c:
        c = float("nan")                                                          # one NaN: the positive quiet one, no payload
    return c, iters, 0, trace


def scale(p_bits, C, fanout, eps=0.9999):
    """k_poisson_scale / poisson_scale_body -> (c, iters, all_one)."""
    return scale_trace(p_bits, C, fanout, eps)[:3]


def inclusion(p_bits, S, c, all_one):
    """P (bits) of a candidate list: bandit_sampler.py:403-406 in torch's arithmetic; seeds and all_one give 1."""
    if all_one:
        return torch.full_like(p_bits, ONE)
    p = from_bits(p_bits)
    P = canon_nan(bits(torch.minimum(p * c, torch.ones_like(p))))
    P[:S] = ONE
    return P


def draw_uniforms(uniforms, cand_nid, C):
    """A planted fp32 vector, or (seed, step, layer): keyed_uniform of the candidates' node ids."""
    if isinstance(uniforms, tuple):
        seed, step, layer = uniforms
        return bo.keyed_uniform(seed, step, layer, cand_nid[:C].long())
    return uniforms[:C]


def _emit(cand_nid, member, drawn, prob_bits, cap_k, num_nodes):
    """The ordered compaction both selects end with: rank in ``member``; entries below cap_k only; padding from K to cap_k."""
    C = int(member.numel())
    rank = torch.cumsum(member.to(torch.int64), 0) - 1
    K_true = int(member.sum())
    K = min(K_true, cap_k)
    ok = member & (rank < cap_k)
    new_id = torch.full((C,), -1, dtype=torch.int32)
    new_id[ok & drawn] = rank[ok & drawn].to(torch.int32)
    new_id[ok & ~drawn] = (-2 - rank[ok & ~drawn]).to(torch.int32)
    kept_nid = torch.zeros(cap_k, dtype=torch.int32)
    node_prob = torch.full((cap_k,), ONE, dtype=torch.int32)
    kept_nid[:K] = cand_nid[:C][ok]
    node_prob[:K] = prob_bits[ok]
    out = dict(new_id=new_id, kept_nid=kept_nid, node_prob=node_prob, K=K, err=ERR_CAP_KEPT if K_true > cap_k else 0)
    if num_nodes is not None:
        km = torch.full((num_nodes,), -1, dtype=torch.int32)
        km[cand_nid[:C][ok & drawn].long()] = rank[ok & drawn].to(torch.int32)
        out["kept_map"] = km
    return out


def select(p_bits, cand_nid, S, C, c, all_one, uniforms, cap_c, cap_k, num_nodes=None):
    """k_select_fused / k_select_keyed.  P, new_id: [min(C, cap_c)]; kept_nid, node_prob: [cap_k]; kept_map: [num_nodes]."""
    C = min(C, cap_c)
    P = inclusion(p_bits[:C], min(S, C), c, all_one)
    keep = torch.zeros(C, dtype=torch.bool)
    keep[bo.poisson_draw(from_bits(P), draw_uniforms(uniforms, cand_nid, C))] = True      # :422-424  u < float(P)
    out = _emit(cand_nid, keep, keep, P, cap_k, num_nodes)
    out["P"] = P
    return out


def mn_select(p_bits, cand_nid, S, C, marks, cap_c, cap_k, num_nodes=None, chosen=None):
    """bliss_multinomial_select (``chosen``: candidate-local ids) / bliss_multinomial_select_marked (``marks``: 0 / 1 per
    candidate): P = p, u_nodes = union(drawn, seeds) in candidate order, new_id = r / -2 - r / -1, kept_map for drawn nodes."""
    C = min(C, cap_c)
    err = 0
    if chosen is not None:
        marks = torch.zeros(C, dtype=torch.int32)
        ch = chosen.long()
        ok = (ch >= 0) & (ch < C)
        marks[ch[ok]] = 1
        if not bool(ok.all()):
            err |= ERR_CAP_CAND
    drawn = marks[:C] == 1
    member = drawn | (torch.arange(C) < S)
    out = _emit(cand_nid, member, drawn, p_bits[:C], cap_k, num_nodes)
    out["P"] = p_bits[:C].clone()
    out["err"] |= err
    return out


# ----------------------------------------------------------------------------------------------------------------- comparison
def compare(got, want):
    """THE comparison of the GPU module: every key of ``want`` against ``got``, integers only (a float: its bytes), no tolerance.
    Returns the list of differences (empty = equal), each with the first differing index."""
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
    out = torch.full((length,), sentinel, dtype=torch.int32)
    out[: values.shape[0]] = values
    return out


TAIL = 37                                                     # entries behind every output's capacity; they must keep the sentinel
SENT = dict(P=0x6B6B, new_id=-77, kept_nid=-9, node_prob=0x4C4C, kept_map=-1, chunk_cnt=0x0BADBEEF)


def want_buffers(r, cap_c, cap_k):
    """The whole (over-long) buffers a call must leave, sentinels included, from a restatement's result."""
    w = dict(r)
    for k, cap in (("P", cap_c), ("new_id", cap_c), ("kept_nid", cap_k), ("node_prob", cap_k)):
        w[k] = padded(r[k], cap + TAIL, SENT[k])
    if "kept_map" in r:
        w["kept_map"] = padded(r["kept_map"], r["kept_map"].numel() + TAIL, SENT["kept_map"])
    return w


# ------------------------------------------------------------------------------------------------- the exact-sum input condition
def exact_sum_condition(p_bits, C, fanout, eps=0.9999):
    """For every iteration the restatement runs on (p, fanout): q such that every term min(rbf(c p), 1) is a multiple of 2^-q, and
    log2 of the sum.  q + log2(sum) < 53 => every partial sum of non-negative terms is a double, whatever the order (the kernel's
    per-thread, shuffle and cross-wave order, torch.sum's).  Returns [(q, sum)]; a NaN term (c is NaN from then on: NaN + x is
    NaN in any order) ends the list with (None, nan)."""
    out = []
    for c, t, n in scale_trace(p_bits, C, fanout, eps)[3]:
        if bool(torch.isnan(t).any()):
            out.append((None, float("nan")))
            break
        pos = t[t > 0]
        if pos.numel() == 0:
            out.append((0, 0.0))
            continue
        m, e = torch.frexp(pos)                                # t = m 2^e, m in [0.5, 1): 8 significant bits => multiple of 2^(e - 8)
        q = int((8 - e).max())                                 # (an upper bound on q: trailing zero bits are not taken off)
        out.append((q, math.fsum((t * n).tolist())))
    return out


# ------------------------------------------------------------------------------------------------------- inputs of the GPU tests
SIZES = [1, 1023, 1024, 1025, 64 * 1024, 64 * 1024 + 1, 65 * 1024 + 1, 129 * 1024 + 5, 150000]
SEEDS_LADDER = [0, 1, 64, 1024, 1025, 4000]
KINDS = ["window", "zeros", "high", "tiny", "nan", "payload", "unsettled"]
MARKS = ["none", "all", "seeds", "non_seeds", "one_per_chunk", "random"]


def fanouts(C):
    """all_one (C + 3, C), one iteration or a few (C - 1), several (C / 3, C / 50); deduplicated, >= 1 (the reference's loop
    divides by the sum, which a fanout of 0 drives to 0: not a defined input)."""
    return sorted({f for f in (C + 3, C, C - 1, C // 3, C // 50) if f >= 1}, reverse=True)


def seeds_for(C, i):
    """The i-th entry of the S ladder that fits C."""
    fit = [s for s in SEEDS_LADDER if s <= C]
    return fit[i % len(fit)]


def make_list(C, kind, seed):
    """A hand-made candidate list -> (p bits int32 [C], cand_nid int32 [C] distinct, not ascending, num_nodes).
    window:    p in [2^-9, 1): inside k_cand_number's LDS window, a narrow exponent range (the exact-sum condition);
    zeros:     a fifth of them p = 0;
    high:      a tenth of them in [2, 2^15) (bins >= 0x4000);
    tiny:      ALL of them in [2^-34, 2^-32) (below the window; the terms stay in three binades, c grows to about 2^32) -- short lists;
    nan:       window with three 0x7fc0: c becomes NaN;
    payload:   the select-alone palette: 0, 0xffc0, 0x7fc0, a denormal, tiny, ordinary and > 1 values (never through the scale);
    unsettled: one pattern everywhere: the sum moves in steps of 2^-8 relative and never comes within 1 - eps of the fanout."""
    gen = torch.Generator().manual_seed(seed)
    V = 2 * C + 11
    cand = torch.randperm(V, generator=gen)[:C].to(torch.int32)
    rnd = lambda lo, hi: torch.randint(lo, hi, (C,), generator=gen).to(torch.int32)
    p = rnd(0x3B00, 0x3F80)
    pick = torch.rand(C, generator=gen)
    if kind == "zeros":
        p[pick < 0.2] = 0
    elif kind == "high":
        p = torch.where(pick < 0.1, rnd(0x4000, 0x4700), p)
    elif kind == "tiny":
        p = rnd(0x2E80, 0x2F80)
    elif kind == "nan":
        p[torch.randperm(C, generator=gen)[:3]] = NAN
    elif kind == "payload":
        palette = torch.tensor([0x0000, 0x7FC0, 0xFFC0, 0x3480, 0x3C23, 0x3D80, 0x3E99, 0x3F00, 0x3F7F, 0x3F80, 0x4049, 0x0001, 0x2F00],
                               dtype=torch.int32)
        p = palette[torch.randint(0, palette.numel(), (C,), generator=gen)]
    elif kind == "unsettled":
        p[:] = 0x3E99
    elif kind != "window":
        raise ValueError(kind)
    return p, cand, V


def make_uniforms(p_bits, seed):
    """torch.rand's 24-bit uniforms, with u = 0 planted on a few candidates (where p = 0: P = 0 and ``u < P`` must not keep)."""
    gen = torch.Generator().manual_seed(seed + 1000)
    u = torch.rand(p_bits.numel(), generator=gen)
    zero = torch.nonzero(p_bits == 0).flatten()[-5:]               # (the last ones: not among the seeds)
    u[zero] = 0.0
    if p_bits.numel() > 7:
        u[7] = 0.0
    return u


def mark_list(C, S, pattern, seed):
    """0 / 1 marks over the C candidates."""
    gen = torch.Generator().manual_seed(seed + 2000)
    m = torch.zeros(C, dtype=torch.int32)
    if pattern == "all":
        m[:] = 1
    elif pattern == "seeds":
        m[:S] = 1
    elif pattern == "non_seeds":
        m[S:] = 1
    elif pattern == "one_per_chunk":
        nb = chunks(C)
        off = torch.randint(0, CHUNK, (nb,), generator=gen)
        m[(torch.arange(nb) * CHUNK + off).clamp(max=C - 1)] = 1
    elif pattern == "random":
        m = (torch.rand(C, generator=gen) < 0.3).to(torch.int32)
    elif pattern != "none":
        raise ValueError(pattern)
    return m


def scale_inputs():
    """Every (C, kind, list seed, fanout, eps) the GPU module sends through k_poisson_scale: the ladder on window lists, the kinds
    on short lists (and the two-candidate window list: the smallest on which the scale iterates, C = 1 being all_one), the re-use rounds.  test_select_ref.py asserts the exact-sum condition on each."""
    out = []
    for C in SIZES:
        for f in fanouts(C):
            out.append((C, "window", C, f, 0.9999))
    for C, kind in KIND_CASES:
        for f in fanouts(C):
            out.append((C, kind, C + 7, f, 0.9999))
        out.append((C, kind, C + 7, max(C // 3, 1), 0.99))
    for C, f in REUSE_ROUNDS:
        out.append((C, "window", C, f, 0.9999))
    return out


KIND_CASES = [(2, "window"), (1025, "zeros"), (3000, "zeros"), (1025, "high"), (3000, "high"), (700, "tiny"), (1025, "tiny"), (1025, "nan"),
              (3000, "nan"), (1000, "unsettled")]
REUSE_ROUNDS = [(66561, 22187), (1025, 341), (1, 1), (150000, 3000), (1024, 1027), (65537, 1310), (1, 4), (3000, 1000),
                (132101, 44033), (1023, 20), (1, 1), (66561, 1331)]


# ------------------------------------------------------------------------------------------ structural model of select_fused_body
def _f2bf_np(x, truncate=False):
    """common.cuh:f2bf on a float32 array: round to nearest even on the bits, every NaN -> 0x7fc0."""
    u = x.view(np.uint32).astype(np.uint64)
    r = (u >> 16) if truncate else ((u + 0x7FFF + ((u >> 16) & 1)) >> 16)
    return np.where(np.isnan(x), NAN, r & 0xFFFF).astype(np.int64)


def _bf2f_np(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def model_select(p_bits, cand_nid, S, C, c, all_one, uniforms, cap_c, cap_k, num_nodes=None, bump_step=0, fault=None):
    """select_fused_body, structurally: per-candidate P and keep bit in the kernel's own fp32 steps, 1024-candidate chunks of 4 waves
    x 4 items x 64 lanes in the kernel's index order, a ballot per (wave, item), wave offsets inside the chunk, one status word
    per chunk and the 64-wide look-back rounds -- under the schedule with the LONGEST walks: when a chunk looks back, every
    predecessor but chunk 0 (which has none and publishes its prefix at once) has published only its aggregate.
    -> the restatement's dictionary + ``rounds`` (look-back rounds per chunk) + ``step`` (keyed: the step word afterwards).
    ``fault``: one planted fault (see FAULTS)."""
    C = min(C, cap_c)
    nch = chunks(C)
    pb, nid = p_bits[:C].numpy().astype(np.int64), cand_nid[:C].numpy()
    step_after = None
    if isinstance(uniforms, tuple):
        seed, step, layer = uniforms
        step_after = step + (1 if bump_step else 0)
        if fault == "bump_before_key" and bump_step:
            step = step + 1
        u = bo.keyed_uniform(seed, step, layer, cand_nid[:C].long()).numpy()
    else:
        u = uniforms[:C].numpy()
    # incl_prob
    j = np.arange(C)
    c32 = np.float32(c)
    with np.errstate(all="ignore"):
        v = _bf2f_np(_f2bf_np(_bf2f_np(pb) * c32, truncate=fault == "truncate"))
    P = np.where((v < 1) | np.isnan(v), _f2bf_np(v), ONE)
    seed_mask = (j <= S) if fault == "seed_le" else (j < S)
    P = np.where(seed_mask | bool(all_one), ONE, P)
    Pf = _bf2f_np(P)
    with np.errstate(invalid="ignore"):
        keep = (u <= Pf) if fault == "bernoulli_le" else (u < Pf)
    # ballots: index j = chunk * 1024 + wave * 256 + item * 64 + lane
    full = np.zeros(nch * CHUNK, dtype=np.int64)
    full[:C] = keep
    ballots = full.reshape(nch, WAVES, ITEMS, LANES)
    wave_total = ballots.sum(axis=(2, 3))                                        # [chunk, wave]
    tot = wave_total.sum(axis=1)
    woff = np.cumsum(wave_total, axis=1) - wave_total                            # chunk_wave_offset
    # status words and the look-back
    state = np.zeros(nch, dtype=np.int64)
    excl_of = np.zeros(nch, dtype=np.int64)
    rounds = np.zeros(nch, dtype=np.int64)
    dropped = nch // 2 if fault == "agg_dropped" and nch > 2 else -1
    for ch in range(nch):
        excl = 0
        if ch > 0:
            top = ch - 1
            while top >= 0:
                lane = np.arange(ROUND)
                jj = top - lane
                w = np.where(jj >= 0, state[np.maximum(jj, 0)], SEL_PFX)
                pfx = (w & 3) == SEL_PFX
                stop = int(np.argmax(pfx)) if pfx.any() else ROUND - 1
                use = ((lane < stop) if fault == "lane_lt_stop" else (lane <= stop)) & (jj >= 0)
                excl += int(((w >> 2) * use).sum())
                rounds[ch] += 1
                if pfx.any():
                    break
                top -= 65 if fault == "top_65" else ROUND
        excl_of[ch] = excl
        # what the successors will read: chunk 0's inclusive prefix; everybody else's aggregate (the longest-walk schedule)
        if ch == 0:
            state[0] = ((0 if fault == "pfx_exclusive" else int(tot[0])) << 2) | SEL_PFX
        else:
            state[ch] = ((0 if ch == dropped else int(tot[ch])) << 2) | SEL_AGG
    K_true = int(excl_of[nch - 1] + tot[nch - 1]) if nch else 0
    K = min(K_true, cap_k)
    # emit
    in_wave = np.cumsum(ballots.reshape(nch, WAVES, ITEMS * LANES), axis=2) - ballots.reshape(nch, WAVES, ITEMS * LANES)
    r = (excl_of[:, None, None] + woff[:, :, None] + in_wave).reshape(-1)[:C]
    new_id = np.where(keep & (r < cap_k), r, -1)
    kept_nid = np.full(cap_k, SENT["kept_nid"], dtype=np.int64)
    node_prob = np.full(cap_k, SENT["node_prob"], dtype=np.int64)
    ok = new_id >= 0
    kept_nid[new_id[ok]] = nid[ok]
    node_prob[new_id[ok]] = P[ok]
    pad = K + 1 if fault == "pad_from_K1" else K
    kept_nid[pad:] = 0
    node_prob[pad:] = ONE
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32)
    out = dict(P=t(P), new_id=t(new_id), kept_nid=t(kept_nid), node_prob=t(node_prob), K=K, err=ERR_CAP_KEPT if K_true > cap_k else 0)
    if num_nodes is not None:
        km = np.full(num_nodes, -1, dtype=np.int64)
        km[nid[ok]] = new_id[ok]
        out["kept_map"] = t(km)
    return out, dict(rounds=rounds, step=step_after)


FAULTS = ["top_65", "lane_lt_stop", "agg_dropped", "pfx_exclusive", "seed_le", "bernoulli_le", "pad_from_K1", "truncate",
          "bump_before_key"]
