"""Per-element error bounds for the bf16 message-passing kernels and the dense SAGE kernels, their fp64 references, and
designed blocks and inputs.

A plain helper module, imported by the tests like shard_cpu_ops.py.  Every check has the form

    |got - ref| <= k_ulp * ulp_bf16(ref) + k_mag * 2^-8 * mag            (element by element)

``ref`` is the fp64 value of the operation on the same bf16 operands, ``mag`` the same formula evaluated on the absolute
values of its terms (so an element 100x smaller than the tensor's largest is held to its own scale), ``k_ulp`` covers the
final rounding to bf16 and ``k_mag`` the roundings of intermediate values, in units of one bf16 half-spacing pair (2^-8).
The constants of each tensor are written in the docstring of the test that uses them.

The references work on any device (the GPU tests run them on the GPU in float64, the CPU tests in tests/test_bounds.py on
small blocks).  ``gat_terms`` restates model.py:82-99 and its backward formula by formula, so that a test can round the
intermediates the kernels store in bf16 (``sim=True``) or plant a fault in one sum; ``gat_autograd`` is the same forward
differentiated by torch autograd, the reference the GPU tests compare against.
"""
import torch

NEG_SLOPE = 0.2


# ------------------------------------------------------------------------------------------------ the bound
def ulp_bf16(x):
    """Spacing of bf16 at |x| (float64, same shape): 2^(e - 8) for |x| in [2^(e-1), 2^e); 2^-133 (the subnormal spacing) for
    zero and every |x| below the smallest normal."""
    x = x.detach().double().abs()
    _, e = torch.frexp(x)
    u = torch.ldexp(torch.ones_like(x), (e - 8).to(torch.int32))
    return torch.where(x < 2.0 ** -126, torch.full_like(x, 2.0 ** -133), u)


def rbf(x):
    """Round to bf16 (nearest even) and back, keeping the dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def assert_within(got, ref, mag, k_ulp, k_mag, what):
    """Every element: |got - ref| <= k_ulp * ulp_bf16(ref) + k_mag * 2^-8 * mag.  Returns the largest |got - ref| / bound (0 where
    got == ref exactly).  On failure the message names the worst element (index, got, ref, bound, ratio) and how many elements are
    over the bound.  A non-finite ``got`` counts as over."""
    got, ref, mag = got.detach().double(), ref.detach().double().to(got.device), mag.detach().double().to(got.device)
    assert got.shape == ref.shape == mag.shape, (what, tuple(got.shape), tuple(ref.shape), tuple(mag.shape))
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    bound = k_ulp * ulp_bf16(ref) + k_mag * 2.0 ** -8 * mag
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    over = int((ratio > 1).sum())
    worst = int(ratio.reshape(-1).argmax())
    if over:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), tuple(got.shape)))
        raise AssertionError("%s: %d of %d elements over the bound; worst at %s: got %.9g ref %.9g bound %.3g ratio %.3g"
                             % (what, over, got.numel(), idx, float(got.reshape(-1)[worst]), float(ref.reshape(-1)[worst]),
                                float(bound.reshape(-1)[worst]), float(ratio.reshape(-1)[worst])))
    return float(ratio.reshape(-1)[worst])


# ------------------------------------------------------------------------------------------------ SpMM (weighted_aggregate)
def spmm_terms(src, dst, n_rows, h, w=None, mean=True, by_src=False, n_out=None, deg=None, scale=None):
    """fp64 reference and magnitude of weighted_aggregate and of its transposed backward.

    Forward (by_src=False): out[i] = (1/deg_i if mean) sum_{e -> i} w_e h[src_e]          (h: [K, dim], rows = destinations)
    Backward (by_src=True): gh[j] = sum_{e : src_e = j} (w_e / deg_{dst_e} if mean) h[dst_e]  (h = d out: [S, dim])
    ``deg``: in-degrees of the destinations (default: counted from dst).  ``scale``: a per-edge factor that replaces 1/deg
    (planted faults only).  Returns (ref, mag), both float64 [n_out, dim]."""
    h = h.double()
    src, dst = src.long(), dst.long()
    if deg is None:
        deg = torch.bincount(dst, minlength=n_rows).double()
    c = torch.ones(src.numel(), dtype=torch.float64, device=h.device) if w is None else w.double().reshape(-1)
    if mean:
        c = c * (scale if scale is not None else 1.0 / deg.clamp(min=1)[dst])
    rows, nbrs = (src, dst) if by_src else (dst, src)
    n = n_out if n_out is not None else (int(h.shape[0]) if by_src else n_rows)
    ref = torch.zeros(n, h.shape[1], dtype=torch.float64, device=h.device).index_add_(0, rows, c[:, None] * h[nbrs])
    mag = torch.zeros(n, h.shape[1], dtype=torch.float64, device=h.device).index_add_(0, rows, (c.abs()[:, None] * h[nbrs].abs()))
    return ref, mag


# ------------------------------------------------------------------------------------------------ GATv2 message passing
def _seg_max(v, dst, S):
    H = v.shape[1]
    return torch.full((S, H), -float("inf"), dtype=v.dtype, device=v.device).scatter_reduce(
        0, dst[:, None].expand(-1, H), v, "amax", include_self=True)


def _seg_sum(v, dst, S):
    return torch.zeros((S,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device).index_add_(0, dst, v)


def gat_terms(src, dst, S, feat, attn, H, D, g=None, slope=NEG_SLOPE, mask=None, p=0.0, sim=False, fault=None):
    """model.py:82-99 and its backward, formula by formula, in float64, with magnitudes.

    feat [K, H*D] (= fc_src(h)), attn [H*D], g = d rst [S, H*D] or None; ``mask`` [B, H] bool (attention dropout kept, with
    p > 0).  Per edge k = (j = src, i = dst) and head:  x = el_j + er_i, e = attn . lrelu(x), a = softmax_i(e),
    ad = a mask / (1 - p), rst_i = sum ad el_j;  da = mask / (1 - p) (g_i . el_j), t_i = sum a da, de = a (da - t_i),
    d er_i = attn sum de lrelu'(x), d el_j = sum_out (de attn lrelu'(x) + ad g_i), d attn = sum de lrelu(x),
    d feat = d el with d er added on the first S rows.

    sim=True rounds to bf16 what the kernels store in bf16 (e, a, a_drop, da, de, d_er, rst, d el, d feat, d attn) and goes on
    from the rounded values.  ``fault`` (planted faults of tests/test_bounds.py), a dict of
      drop_fwd:   edge ids left out of the destination side (never seen: their e stays 0, no softmax, aggregation or d er term)
      drop_agg:   edge ids left out of the aggregation sum only
      drop_t:     edge ids left out of t (the softmax backward's row sum)
      drop_der:   edge ids left out of d er
      drop_src:   edge ids left out of the by-source sum d el
      no_drop_scale: the dropout backward multiplies by the mask without 1 / (1 - p)
    Returns a dict of float64 tensors: e, a, ad, rst, mag_e, mag_rst and, with g, da, t, de, d_er, d_el, d_feat, d_attn,
    mag_de, mag_der, mag_del, mag_dfeat, mag_dattn.  The magnitudes never see the fault or the rounding."""
    fault = fault or {}
    dev = feat.device
    src, dst = src.long(), dst.long()
    B, K = src.numel(), feat.shape[0]
    f = feat.double().view(K, H, D)
    at = attn.double().reshape(1, H, D)
    R = rbf if sim else (lambda x: x)

    def keep(name):
        m = torch.ones(B, dtype=torch.float64, device=dev)
        if name in fault:
            m[torch.as_tensor(fault[name], dtype=torch.long, device=dev)] = 0.0
        return m[:, None]

    k_fwd, k_agg, k_t, k_der, k_src = keep("drop_fwd"), keep("drop_agg"), keep("drop_t"), keep("drop_der"), keep("drop_src")
    el, er = f[src], f[dst]
    x = el + er
    lr = torch.where(x > 0, x, slope * x)
    lp = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))
    e_exact = (at * lr).sum(-1)
    out = dict(mag_e=(at.abs() * lr.abs()).sum(-1))
    e = R(e_exact) * k_fwd
    # softmax over the in-edges that are seen (an unseen edge gets no coefficient)
    m = _seg_max(torch.where(k_fwd > 0, e, torch.full_like(e, -float("inf"))), dst, S)
    ex = torch.exp(e - m[dst]) * k_fwd
    a = R(ex / _seg_sum(ex, dst, S)[dst])
    a = torch.nan_to_num(a)
    if mask is not None:
        ms = mask.double() / (1.0 - p)
    else:
        ms = torch.ones_like(a)
    ad = R(a * ms)
    rst = R(_seg_sum((ad * k_agg)[:, :, None] * el, dst, S))
    out.update(e=e, a=a, ad=ad, rst=rst.view(S, H * D))
    out["mag_rst"] = _seg_sum(ad.abs()[:, :, None] * el.abs(), dst, S).view(S, H * D)
    if g is None:
        return out
    gd = g.double().view(S, H, D)[dst]
    dot = (gd * el).sum(-1)
    dscale = (mask.double() if fault.get("no_drop_scale") else ms) if mask is not None else ms
    da = R(R(dot) * dscale) * k_fwd
    t = _seg_sum(a * da * k_t, dst, S)
    de = R(a * (da - t[dst])) * k_fwd
    d_er = R(at[0] * _seg_sum((de * k_der)[:, :, None] * lp, dst, S))
    d_el = R(torch.zeros(K, H, D, dtype=torch.float64, device=dev).index_add_(
        0, src, k_src[:, :, None] * (de[:, :, None] * at * lp + ad[:, :, None] * gd)))
    d_feat = d_el.clone()
    d_feat[:S] = R(d_feat[:S] + d_er)
    d_attn = R((de[:, :, None] * lr).sum(0).reshape(-1))
    # magnitudes: the softmax backward's d e = a (da - t) enters as a (|da| + sum a |da|) (the cancellation in da - t)
    a_abs, da_abs = a.abs(), da.abs()
    mag_de = a_abs * (da_abs + _seg_sum(a_abs * da_abs, dst, S)[dst])
    mag_der = at[0].abs() * _seg_sum(mag_de[:, :, None] * lp, dst, S)
    mag_del = torch.zeros(K, H, D, dtype=torch.float64, device=dev).index_add_(
        0, src, mag_de[:, :, None] * at.abs() * lp + ad.abs()[:, :, None] * gd.abs())
    mag_dfeat = mag_del.clone()
    mag_dfeat[:S] += mag_der
    out.update(da=da, t=t, de=de, d_er=d_er.view(S, H * D), d_el=d_el.view(K, H * D), d_feat=d_feat.view(K, H * D), d_attn=d_attn,
               mag_de=mag_de, mag_der=mag_der.view(S, H * D), mag_del=mag_del.view(K, H * D), mag_dfeat=mag_dfeat.view(K, H * D),
               mag_dattn=(mag_de[:, :, None] * lr.abs()).sum(0).reshape(-1))
    return out


def gat_autograd(src, dst, S, feat, attn, H, D, g, slope=NEG_SLOPE, mask=None, p=0.0):
    """fp64 autograd of model.py:82-99 (share_weights: feat_dst = feat_src[:S]) on the bf16 operands: (e, rst, d feat, d attn)."""
    src, dst = src.long(), dst.long()
    K = feat.shape[0]
    f = feat.detach().double().requires_grad_(True)
    at = attn.detach().double().reshape(1, H, D).requires_grad_(True)
    fs = f.view(K, H, D)
    x = torch.nn.functional.leaky_relu(fs[src] + fs[dst], slope)
    e = (x * at).sum(-1)
    m = _seg_max(e.detach(), dst, S)
    ex = torch.exp(e - m[dst])
    a = ex / _seg_sum(ex, dst, S)[dst]
    if mask is not None:
        a = a * mask.double() / (1.0 - p)
    rst = _seg_sum(a[:, :, None] * fs[src], dst, S).view(S, H * D)
    (rst * g.double()).sum().backward()
    return e.detach(), rst.detach(), f.grad, at.grad.reshape(-1)


# ------------------------------------------------------------------------------------------------ designed blocks
class Spec:
    """A block as plain CPU tensors: n_src K, n_dst S, CSR by destination (indptr int64 [S+1], src, dst int64 [B])."""

    def __init__(self, K, S, indptr, src, dst):
        self.K, self.S, self.indptr, self.src, self.dst = int(K), int(S), indptr, src, dst

    @property
    def B(self):
        return int(self.src.numel())

    def in_degrees(self):
        return self.indptr[1:] - self.indptr[:-1]

    def out_degrees(self):
        return torch.bincount(self.src, minlength=self.K)


def from_degrees(degs, K, seed, hub_src=None, hub_every=0, n_unused=0):
    """Destination i gets degs[i] in-edges; sources drawn uniformly from [0, K - n_unused) (the last n_unused sources never
    send), every ``hub_every``-th edge from source ``hub_src``.  Deterministic in ``seed``."""
    gen = torch.Generator().manual_seed(seed)
    degs = torch.as_tensor(degs, dtype=torch.int64)
    S, B = degs.numel(), int(degs.sum())
    indptr = torch.zeros(S + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(degs, 0)
    dst = torch.repeat_interleave(torch.arange(S), degs)
    src = torch.randint(0, K - n_unused, (B,), generator=gen)
    if hub_src is not None and hub_every:
        src[::hub_every] = hub_src
    return Spec(K, S, indptr, src, dst)


EDGE_DEGREES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 512, 513, 1500]
HUB_DEGREE = 12000                     # ~47 segments of 256 edges


def edge_shape_spec(seed=11):
    """In-degrees 0, 1, 2, 15..17, 63..65, 255..257, 512, 513, 1500, one hub of 12 000 (47 segments) and 240 ordinary rows
    (3..94); source S + 5 sends every 6th edge (> 3000 out-edges), the last 16 sources send none, the first S sources are the
    destinations.  ~27 K edges."""
    degs = EDGE_DEGREES + [HUB_DEGREE] + [3 + (7 * i) % 92 for i in range(240)]
    S = len(degs)
    return from_degrees(degs, S + 1400, seed, hub_src=S + 5, hub_every=6, n_unused=16)


def many_hubs_spec(seed=12, n_hubs=1536):
    """1536 destinations of 257..1100 in-edges (4 953 virtual workgroups, far more than the chip holds at
    once) beside 64 short rows; ~1.05 M edges."""
    degs = [257 + (613 * i) % 844 for i in range(n_hubs)] + [1 + i % 9 for i in range(64)]
    S = len(degs)
    return from_degrees(degs, S + 20000, seed, n_unused=8)


def row_count_spec(S, seed=13):
    """S destinations (16 384: the one-sweep branch of k_gat_segments; 16 385: the two-pass branch), rows of 0..7 in-edges and
    six hubs of 300..1400."""
    degs = [i % 8 for i in range(S)]
    for q, d in enumerate((300, 513, 800, 1024, 1100, 1400)):
        degs[(q * 2731 + 17) % S] = d
    return from_degrees(degs, S + 3000, seed, n_unused=8)


def spmm_band_spec(B, seed):
    """~B edges over 4 000 destinations (row lengths 1..2B/4000, none above 16 384), one source with >= 3000 out-edges."""
    S = 4000
    mean = B // S
    degs = [1 + (i * 37) % (2 * mean - 1) for i in range(S)]
    degs[0] += B - sum(degs)
    assert 0 < degs[0] <= 16384
    return from_degrees(degs, S + 6000, seed, hub_src=S + 1, hub_every=max(1, B // 3500), n_unused=8)


def to_block(spec, device):
    """A bliss Block of ``spec`` on ``device``."""
    from bliss_gnn_amd.graph import Block
    i32 = lambda t: t.to(torch.int32).to(device)
    z = torch.zeros(spec.B, dtype=torch.int32, device=device)
    return Block(None, spec.K, spec.S, i32(spec.indptr), i32(spec.src), i32(spec.dst), z, z.clone(),
                 torch.arange(spec.K, dtype=torch.int32, device=device))


def padded_block(spec, device, extra_s=37, extra_k=101, extra_b=777):
    """The capacity-padded copy of ``spec`` as the static-shape sampler leaves it: src / dst longer than the true edge count,
    their padding holding valid but wrong ids (the hub rows' and the hub source's); indptr rows past the true S repeating the
    edge count (csrc/sampler.hip); n_src / n_dst the capacities; _counts_dev an int32[10] laid out as bliss_layer_counts_t
    (S at word 0, B at word 4) and _nnz_ptr at its word 4 (_engine.py)."""
    from bliss_gnn_amd.graph import Block
    S, K, B = spec.S, spec.K, spec.B
    Sc, Kc, Bc = S + extra_s, K + extra_k, B + extra_b
    deg = spec.in_degrees()
    hub_row = int(deg.argmax())
    hub_src = int(spec.out_degrees().argmax())
    indptr = torch.cat([spec.indptr, torch.full((extra_s,), B, dtype=torch.int64)])
    src = torch.cat([spec.src, torch.full((extra_b,), hub_src, dtype=torch.int64)])
    dst = torch.cat([spec.dst, torch.full((extra_b,), hub_row, dtype=torch.int64)])
    counts = torch.zeros(10, dtype=torch.int32)
    counts[0], counts[4] = S, B
    counts = counts.to(device)
    i32 = lambda t: t.to(torch.int32).to(device)
    z = torch.zeros(Bc, dtype=torch.int32, device=device)
    blk = Block(None, Kc, Sc, i32(indptr), i32(src), i32(dst), z, z.clone(), torch.arange(Kc, dtype=torch.int32, device=device))
    blk._counts, blk._counts_dev = None, counts
    blk._nnz_ptr = counts.data_ptr() + 16
    return blk


def gat_inputs(spec, H, D, seed, device, positive=False, loud=None, loud_scale=64.0):
    """bf16 operands of the message passing on ``spec``: feat [K, H*D] (= fc_src(h)), attn [1, H, D] scaled so that every logit's
    magnitude sum_d |attn| |lrelu(x)| is at most 1 (the GATv2 constants below assume it), g = d rst [S, H*D].  ``positive``:
    feat and g > 0 (no cancellation: what some planted faults need to be seen).  ``loud``: source ids whose feature rows are
    multiplied by ``loud_scale`` (the dedicated sources of loud_segments)."""
    gen = torch.Generator().manual_seed(seed)
    K, S = spec.K, spec.S
    feat = torch.randn(K, H * D, generator=gen) * 0.5
    g = torch.randn(S, H * D, generator=gen)
    if positive:
        feat, g = feat.abs() + 0.05, g.abs() + 0.05
    if loud is not None and len(loud):
        feat[torch.as_tensor(loud, dtype=torch.long)] *= loud_scale
    attn = torch.randn(H * D, generator=gen)
    feat, g = feat.bfloat16().to(device), g.bfloat16().to(device)
    attn = attn.double().to(device)
    f = feat.double().view(K, H, D)
    src, dst = spec.src.to(device), spec.dst.to(device)
    mag = torch.zeros(H, dtype=torch.float64, device=device)
    for b0 in range(0, spec.B, 1 << 16):                   # (in slices: [B, H, D] at once is large on the many-hubs block)
        x = f[src[b0:b0 + (1 << 16)]] + f[dst[b0:b0 + (1 << 16)]]
        lr = torch.where(x > 0, x, NEG_SLOPE * x)
        mag = torch.maximum(mag, (attn.view(1, H, D).abs() * lr.abs()).sum(-1).amax(0))
    attn = (attn.view(1, H, D) * (0.9 / mag.clamp(min=1e-30)).view(1, H, 1)).bfloat16()
    return feat, attn, g


SEG = 256                                # edges per workgroup of the fused GATv2 kernels (GF_SEG): longer rows are shared


def loud_segments(spec, which="cycle"):
    """A copy of ``spec`` in which one 256-edge segment of every shared row (in-degree > 256) takes all its edges from a source of
    its own, appended after the last source: with gat_inputs(positive=True, loud=ids) that segment carries 64x the features of
    the others, so losing it from t, from d er or from the aggregation moves the row by far more than the bound (shown on the
    CPU by tests/test_bounds.py for every block the GPU runs with this pattern).  ``which``: the segment of a row with G
    segments -- "first" (0), "middle" (G // 2), "last" (G - 1) or "cycle" (row mod G: every position on a block with many
    shared rows).  Returns (spec, loud source ids, [(row, first edge, end)] of the loud segments)."""
    deg = spec.in_degrees()
    rows = (deg > SEG).nonzero().reshape(-1).tolist()
    src = spec.src.clone()
    ids, segs = [], []
    for n, r in enumerate(rows):
        G = (int(deg[r]) + SEG - 1) // SEG
        q = {"first": 0, "middle": G // 2, "last": G - 1, "cycle": r % G}[which]
        b0 = int(spec.indptr[r]) + q * SEG
        b1 = min(b0 + SEG, int(spec.indptr[r + 1]))
        src[b0:b1] = spec.K + n
        ids.append(spec.K + n)
        segs.append((r, b0, b1))
    return Spec(spec.K + len(rows), spec.S, spec.indptr, src, spec.dst), ids, segs


def gat_k(me):
    """(k_ulp, k_mag) per GATv2 tensor for logits of magnitude sum_d |attn| |lrelu(x)| <= me (derivation: the docstring of
    tests/test_gpu_grad_edges.py).  The softmax's relative error E_A = 8 for me <= 1 (logit error <= 2 * 2^-8) and 7 me + 2
    above (logit error <= 2.5 me 2^-8, twice, plus the rounding of e - max, 2 me 2^-8, and the exp / sum / division
    roundings, 2): rst E_A + 1, d e 2 E_A + 1.5, d feat and d attn 2 E_A + 2, d feat's destination rows one more."""
    ea = 8.0 if me <= 1 else 7.0 * me + 2.0
    return {"e": (1, 2), "rst": (1, ea + 1), "d_feat_src": (1, 2 * ea + 2), "d_feat_dst": (1, 2 * ea + 3), "d_attn": (1, 2 * ea + 2)}


# Constants of the bound per tensor: (k_ulp, k_mag).  Derivations are in the docstrings of the tests that use them
# (tests/test_gpu_grad_edges.py); tests/test_bounds.py shows on designed blocks that the planted faults fail them.
GAT_K = gat_k(1.0)
SPMM_K = {"bf16": (1, 0.25), "fp32": (0, 0.25)}
GCN_K = (1, 4)
SPMM_MAX_ROW = 16384                     # the SpMM constant holds for rows (by destination or by source) up to this length


def check_gat_layer(layer, blk, h, out, e, gout, feat, d_feat, what, mask=None, p=0.0):
    """Per-element checks of a GATv2Conv layer (no fc_src bias): the message passing on the layer's own feat = fc_src(h) against
    fp64 autograd with gat_k(largest logit magnitude of this data), then the layer's output and the gradients of h and of
    fc_src's weight through the GEMMs, on magnitudes.  The GEMMs take d feat with |error| <= (k + 2) 2^-8 mag (its ulp term
    is at most 2^-7 |ref| <= 2^-7 mag) to |W| or |h|, and add their own rounding and the residual's: k_mag = k(d feat, rows
    < S) + 3 for d h and d W.  The output adds the residual's GEMM rounding and the final add: k(rst) + 1.  Returns the
    largest ratio of each tensor."""
    import torch.nn as nn
    H, D = layer._num_heads, layer._out_feats
    S, HD = blk.num_dst_nodes(), layer._num_heads * layer._out_feats
    src, dst = blk.src, blk.dst
    g64 = gout.reshape(S, HD).double()
    attn = layer.attn.detach()
    ref_e, ref_rst, ref_df, ref_da = gat_autograd(src, dst, S, feat, attn, H, D, g64, mask=mask, p=p)
    T = gat_terms(src, dst, S, feat, attn, H, D, g64, mask=mask, p=p)
    k = gat_k(float(T["mag_e"].max()))
    hd = h.detach().double()
    ref_out, mag_out, dres = ref_rst.clone(), T["mag_rst"].clone(), None
    if isinstance(layer.res_fc, nn.Linear):
        rW = layer.res_fc.weight.detach().double()
        ref_out += hd[:S] @ rW.t()
        mag_out += hd[:S].abs() @ rW.abs().t()
        dres = (g64 @ rW, g64.abs() @ rW.abs())
    elif layer.res_fc is not None:
        ref_out += hd[:S]
        mag_out += hd[:S].abs()
        dres = (g64, g64.abs())
    W = layer.fc_src.weight.detach().double()
    ref_dh, mag_dh = ref_df @ W, T["mag_dfeat"] @ W.abs()
    if dres is not None:
        ref_dh[:S] += dres[0]
        mag_dh[:S] += dres[1]
    kg = k["d_feat_dst"][1] + 3
    r = {"e": assert_within(e.reshape(-1, H), ref_e, T["mag_e"], *k["e"], what + " e"),
         "out": assert_within(out.reshape(S, HD), ref_out, mag_out, 1, k["rst"][1] + 1, what + " out"),
         "d_feat_dst": assert_within(d_feat[:S], ref_df[:S], T["mag_dfeat"][:S], *k["d_feat_dst"], what + " d feat (rows < S)"),
         "d_feat_src": assert_within(d_feat[S:], ref_df[S:], T["mag_dfeat"][S:], *k["d_feat_src"], what + " d feat (rows >= S)"),
         "d_attn": assert_within(layer.attn.grad.reshape(-1), ref_da, T["mag_dattn"], *k["d_attn"], what + " d attn"),
         "d_h": assert_within(h.grad, ref_dh, mag_dh, 1, kg, what + " d h"),
         "d_W": assert_within(layer.fc_src.weight.grad, ref_df.t() @ hd, T["mag_dfeat"].t() @ hd.abs(), 1, kg, what + " d W")}
    return r


# ------------------------------------------------------------------------------------------------ dense SAGE kernels
# csrc/sage.hip (k_tile_gemm), csrc/sage_bwd.hip (k_dgrad, k_wgrad + k_wgrad_reduce).  They accumulate in fp32 and round to
# bf16 once: k_ulp = 1 (half a spacing of the fp32 sum, which may lie one binade above ref) and k_mag = n_terms * 2^-16
# (n_terms fp32 roundings of relative size 2^-24, in units of 2^-8).  A bf16 value stored between two launches adds 1 to k_mag
# (half a spacing <= 2^-8 of its magnitude); a stored SpMM result adds SPMM_K's 0.25 as well.
TILE, KSTEP, SLAB = 32, 16, 64           # output tile of a wave, k of one MFMA, k of one W slab in LDS
WGRAD_TARGET, WGRAD_COLS, WGRAD_MIN_ROWS, WGRAD_STEP = 80, 128, 64, 32


def dense_k(n_terms, stored=0.0):
    """(k_ulp, k_mag) of an fp32-accumulated sum of ``n_terms`` terms rounded to bf16 once, whose operands carry ``stored``
    bf16 roundings (in units of 2^-8 of the magnitude) from earlier launches."""
    return 1, stored + n_terms * 2.0 ** -16


def _dual(a1, b1, a2, b2, bias, m2, fault, acc):
    """a1 @ b1 (+ a2 @ b2 on rows < m2) + bias with b = [k, n], accumulated in ``acc``; (value with the planted fault, fp64
    magnitude without it)."""
    fault = fault or {}
    M = a1.shape[0]
    A1, B1 = a1.to(acc), b1.to(acc)
    if fault.get("drop_w_tail"):                                               # the k beyond the last full 64-slab never loaded
        kk = A1.shape[1] // SLAB * SLAB
        A1, B1 = A1[:, :kk], B1[:kk]
    ref = A1 @ B1
    mag = a1.double().abs() @ b1.double().abs()
    if "drop_kstep" in fault:                                                  # (row0, col0, k0): one MFMA of one tile skipped
        r0, c0, k0 = fault["drop_kstep"]
        ref[r0:r0 + TILE, c0:c0 + TILE] -= A1[r0:r0 + TILE, k0:k0 + KSTEP] @ B1[k0:k0 + KSTEP, c0:c0 + TILE]
    if a2 is not None:
        m = min(M if m2 is None else int(m2), M, a2.shape[0])
        mf = max(0, min(m + int(fault.get("m2_shift", 0)), M, a2.shape[0]))
        ref[:mf] += a2[:mf].to(acc) @ b2.to(acc)
        mag[:m] += a2[:m].double().abs() @ b2.double().abs()
    if bias is not None:
        ref += float(fault.get("bias_times", 1)) * bias.to(acc)
        mag += bias.double().abs()
    if "swap_tile" in fault:                                                   # (row0, col0): a full tile stored transposed
        r0, c0 = fault["swap_tile"]
        ref[r0:r0 + TILE, c0:c0 + TILE] = ref[r0:r0 + TILE, c0:c0 + TILE].t().clone()
    return ref, mag


def gemm_terms(a1, w1, a2=None, w2=None, bias=None, m2=None, fault=None, acc=torch.float64):
    """The forward product of k_tile_gemm, W = [out, in]: a1 @ w1^T (+ a2 @ w2^T on rows < m2) + bias -> (ref, mag) [M, out].
    ``acc=torch.float32`` is the kernel's restatement (fp32 accumulation; round the result with rbf).  ``fault``: drop_kstep
    (row0, col0, k0), drop_w_tail, m2_shift +-1, bias_times 0 | 2, swap_tile (row0, col0); the magnitude never sees it."""
    return _dual(a1, w1.t(), a2, None if w2 is None else w2.t(), bias, m2, fault, acc)


def dgrad_terms(a1, w1, a2=None, w2=None, m2=None, fault=None, acc=torch.float64):
    """The input gradient of k_dgrad: a1 @ w1 (+ a2 @ w2 on rows < m2) -> (ref, mag) [M, in].  Faults as gemm_terms."""
    return _dual(a1, w1, a2, w2, None, m2, fault, acc)


def wgrad_terms(d, x, rows, fault=None, acc=torch.float64):
    """The weight and bias gradients of k_wgrad: d[:rows]^T @ x[:rows] and the column sums of d[:rows] ->
    (dw, mag_dw, db, mag_db).  ``fault``: drop_rows_dw / drop_rows_db (row ids left out of the sum), extra_rows (that many rows
    at and beyond the count included)."""
    fault = fault or {}
    rows = int(rows)
    D, X = d[:rows].double(), x[:rows].double()
    mag_dw, mag_db = D.abs().t() @ X.abs(), D.abs().sum(0)
    n = rows + int(fault.get("extra_rows", 0))
    kw, kb = torch.ones(n, dtype=torch.bool, device=d.device), torch.ones(n, dtype=torch.bool, device=d.device)
    if "drop_rows_dw" in fault:
        kw[torch.as_tensor(fault["drop_rows_dw"], dtype=torch.long, device=d.device)] = False
    if "drop_rows_db" in fault:
        kb[torch.as_tensor(fault["drop_rows_db"], dtype=torch.long, device=d.device)] = False
    dw = d[:n][kw].to(acc).t() @ x[:n][kw].to(acc)
    db = d[:n][kb].to(acc).sum(0)
    return dw, mag_dw, db, mag_db


def wgrad_plan(problems, target=WGRAD_TARGET):
    """The chunk plan of one k_wgrad launch as csrc/sage_bwd.hip documents it, for [(rows_bound, k_in)] (one or two problems):
    chunks = target / (column tiles of all problems together, 128 columns each), at most ceil(rows_bound / 64), at least 1;
    rows_per_chunk = ceil(rows_bound / chunks) rounded up to 32; chunks = ceil(rows_bound / rows_per_chunk).  Returns
    [(chunks, rows_per_chunk)] and the fp32 workspace (floats) the launch needs: chunks * 256 * (128 * column tiles + 4) each."""
    tiles_all = sum(-(-k // WGRAD_COLS) for _, k in problems)
    plan, floats = [], 0
    for rows, k in problems:
        chunks = max(1, min(target // tiles_all, -(-rows // WGRAD_MIN_ROWS)))
        rpc = -(-(-(-rows // chunks)) // WGRAD_STEP) * WGRAD_STEP
        chunks = -(-rows // rpc)
        plan.append((chunks, rpc))
        floats += chunks * 256 * (-(-k // WGRAD_COLS) * WGRAD_COLS + 4)
    return plan, floats


def wgrad_loud_rows(rows, chunks, rpc):
    """The rows a chunked sum loses first: the last row of every chunk that holds rows, the first row of the next, and the last
    valid row."""
    ids = set()
    for c in range(1, chunks):
        if c * rpc < rows:
            ids.update((c * rpc - 1, c * rpc))
    ids.add(rows - 1)
    return sorted(ids)


def wgrad_inputs(rows_bound, n_out, k_in, seed, rows=None, loud=None, loud_scale=64.0, pad=float("nan")):
    """bf16 operands of a weight gradient (CPU): d [rows_bound, n_out] ~ 0.05 N(0, 1), x [rows_bound, k_in] ~ N(0, 1); the rows
    ``loud`` of d multiplied by ``loud_scale`` (one row then weighs as much in dW and db as 64 ordinary ones, and 4096 in their
    variance: losing it moves most elements by more than the bound, shown by tests/test_bounds.py); rows at and beyond ``rows``
    (the device-side count) filled with ``pad``."""
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(rows_bound, n_out, generator=gen) * 0.05
    x = torch.randn(rows_bound, k_in, generator=gen)
    if loud is not None and len(loud):
        d[torch.as_tensor(loud, dtype=torch.long)] *= loud_scale
    if rows is not None:
        d[rows:], x[rows:] = pad, pad
    return d.bfloat16(), x.bfloat16()


# the loud-row weight gradients the GPU suite runs and tests/test_bounds.py shows to be sensitive: (rows_bound, rows, n_out, k_in)
WGRAD_LOUD_CASES = [(11000, 10877, 256, 602), (5000, 4877, 256, 602)]


def sage_layer_terms(src, dst, S, h, w_neigh, w_self, bias, ew=None, h_dst=None, g=None, mask=None, p=0.0, relu=True, sim=False,
                     fault=None):
    """A SAGEConv('mean') layer with its tail, as model.py:321-333 / nn.SAGEConv state it, in float64 with magnitudes:

        rst = fc_self(h_dst) + fc_neigh(mean_w(h))   (in <= out: aggregate first)
        rst = fc_self(h_dst) + mean_w(fc_neigh(h))   (in > out: Linear first),        out = mask / (1 - p) * rst

    h [K, in], h_dst = h[:S] unless given, w_* [out, in], bias [out] or None, edge weights ew or None.  ``mask`` [S, out] is the
    product of the ReLU's mask and the dropout's keep mask (the tests take it from the kernel's output, out > 0, after the forward
    check has held every element of rst that is further than its bound from zero to the right side); None: rst > 0 when
    ``relu``, else ones.  The forward is plain torch on its inputs: with float64 leaves that require grad, autograd through
    ``out`` gives the reference gradients (tests/test_bounds.py checks the formulas below against it).  With ``g`` = d out the
    backward is written out: d = mask / (1 - p) g, dW_self = d^T h_dst, db = sum d, and
        aggregate first:  dW_neigh = d^T agg,  T = A^T d (the transposed aggregation),  dh = T W_neigh + [d W_self on rows < S]
        Linear first:     dZ = A^T d,  dW_neigh = dZ^T h,  dh = dZ W_neigh + [d W_self on rows < S]
    ``sim=True`` rounds to bf16 what the kernels store in bf16 between launches (Z, Y, agg, rst, out, d, dZ / T and every
    result).  ``fault``: relu_mask_wrong (the backward takes the mask of fc_self's part alone), no_drop_scale (the backward
    multiplies by the mask without 1 / (1 - p)), self_rows (fc_self's input gradient lands that many rows further down).
    Returns a dict: rst, mag_rst, out, mag_out (= mag_rst under the mask), z / agg (the stored intermediate) and with g: d, d_mid (dZ or T), d_wn, d_ws, d_b, d_h, d_hdst
    (only with h_dst given) and mag_<name> for each.  The magnitudes never see the fault or the rounding."""
    fault = fault or {}
    R = rbf if sim else (lambda t: t)
    lin_first = w_neigh.shape[1] > w_neigh.shape[0]
    K = h.shape[0]
    hd = h[:S] if h_dst is None else h_dst
    H, HD, Wn, Ws = h.double(), hd.double(), w_neigh.double(), w_self.double()
    b = None if bias is None else bias.double()
    agg_of = lambda t: spmm_terms(src, dst, S, t, ew, True)
    y, mag_y = HD @ Ws.t(), HD.abs() @ Ws.abs().t()
    if b is not None:
        y, mag_y = y + b, mag_y + b.abs()
    out = {}
    if lin_first:
        z = R(H @ Wn.t())
        agg = R(agg_of(z)[0])
        rst = R(R(y) + agg)
        mag_rst = mag_y + agg_of(H.abs() @ Wn.abs().t())[1]
        out["z"] = z
    else:
        agg = R(agg_of(H)[0])
        mag_agg = agg_of(H.abs())[1]
        rst = R(agg @ Wn.t() + y)
        mag_rst = mag_agg @ Wn.abs().t() + mag_y
    out["agg"] = agg
    if mask is None:
        mask = (rst > 0) if relu else torch.ones_like(rst, dtype=torch.bool)
    ms = mask.double() / (1.0 - p)
    out.update(rst=rst, mag_rst=mag_rst, out=R(rst * ms), mag_out=mag_rst * ms)
    if g is None:
        return out
    G = g.double()
    bmask = mask
    if fault.get("relu_mask_wrong"):
        bmask = mask & (y > 0)
    d = R(G * (bmask.double() if fault.get("no_drop_scale") else bmask.double() / (1.0 - p)))
    mag_d = G.abs() * ms
    t_of = lambda t: spmm_terms(src, dst, S, t, ew, True, by_src=True, n_out=K)
    d_mid, mag_mid = R(t_of(d)[0]), t_of(mag_d)[1]
    if lin_first:
        d_wn, mag_wn = R(d_mid.t() @ H), mag_mid.t() @ H.abs()
    else:
        d_wn, mag_wn = R(d.t() @ agg), mag_d.t() @ mag_agg
    d_ws, mag_ws = R(d.t() @ HD), mag_d.t() @ HD.abs()
    d_self, mag_self = d @ Ws, mag_d @ Ws.abs()
    d_h, mag_h = d_mid @ Wn, mag_mid @ Wn.abs()
    if h_dst is None:
        s0 = int(fault.get("self_rows", 0))
        d_h[s0:s0 + S] += d_self
        mag_h[:S] += mag_self
    else:
        out.update(d_hdst=R(d_self), mag_d_hdst=mag_self)
    out.update(d=d, mag_d=mag_d, d_mid=d_mid, mag_d_mid=mag_mid, d_wn=d_wn, mag_d_wn=mag_wn, d_ws=d_ws, mag_d_ws=mag_ws,
               d_b=R(d.sum(0)), mag_d_b=mag_d.sum(0), d_h=R(d_h), mag_d_h=mag_h)
    return out


def sage_layer_k(fin, fout, rows, dropout, lin_first, two_nodes=False):
    """(k_ulp, k_mag) per tensor of a SAGE layer on ``rows`` = max(K, S) block rows, from where the kernels round: a value stored
    in bf16 between launches costs 1 (an SpMM result 1.25, SPMM_K's fp32 sum included), the dropout multiply of the forward
    and of the backward 1 each, every fp32-accumulated GEMM its n_terms * 2^-16 (dense_k; wgrad: rows + at most 80 chunks).
    Parallel paths into one sum take the longer one; the last rounding of each tensor is k_ulp.
      Linear first:    out: Z, agg (2.25);  dZ (1.25) in front of dW_neigh and dh;  dW_self, db, d h_dst: nothing stored.
      aggregate first: out: agg (1.25);  dW_neigh: agg (1.25);  dh: T (1.25);  dW_self, db, d h_dst: nothing stored.
    ``two_nodes``: the input gradient passes one more stored value -- dZ W_neigh in front of the index_add_ of fc_self's part
    (_SageLinearSplit with gathered destinations) or of addmm_ (BLISS_SAGE_MFMA_BWD=0), d W_neigh in front of the transposed
    SpMM whose stored result addmm_ then adds to (_SageAggDual with BLISS_SAGE_MFMA_BWD=0): dh 2.25.  (_SageDualLinear stores
    d agg = d W_neigh, 1, and the transposed SpMM of ops.spmm's backward rounds last: 1.25 as well.)"""
    dr = 1.0 if dropout else 0.0
    wg = (rows + WGRAD_TARGET) * 2.0 ** -16
    fwd = (fin + 1) * 2.0 ** -16 if lin_first else (2 * fin + 1) * 2.0 ** -16
    return {"out": (1, (2.25 if lin_first else 1.25) + dr + fwd),
            "d_wn": (1, 1.25 + dr + wg), "d_ws": (1, dr + wg), "d_b": (1, dr + wg),
            "d_h": (1, (2.25 if two_nodes else 1.25) + dr + 2 * fout * 2.0 ** -16),
            "d_hdst": (1, dr + fout * 2.0 ** -16)}


# ------------------------------------------------------------------------------------------------ cross-entropy (csrc/loss.hip)
# k_cross_entropy: one wave per row of bf16 logits; max, sum of exponentials, one reciprocal, (p - onehot) * inv_n in fp32, one
# rounding to bf16; the row losses m + log s - x_y summed in row order by the last workgroup.  Derivations of ce_k / ce_k_loss:
# the docstring of tests/test_gpu_cross_entropy.py.
CE_GRID_ROWS = 4096                      # rows of one trip of the grid-stride loop (1024 workgroups of 4 waves)
_NEG_LIMIT = -1.0e4                      # a -inf logit at its limit: exp(-1e4 - m) == 0 in float64 for every finite bf16 m in use


def f32(v):
    """The fp32 value a C ``float`` argument receives, as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def ce_terms(x, labels, denom, x2=None, n_valid=None, fault=None, acc=torch.float64):
    """Mean-reduced cross-entropy on bf16 logits x [n, c] (``bf16(x + x2)``, the sum taken in fp32 as the kernel takes it, when
    ``x2`` is given) with class indices ``labels`` [n]: returns (loss, mag_loss, grad, mag_grad).

        loss = (1/denom) sum_{r < n_valid} (m_r + log s_r - x_{r,y}),   grad = (softmax(x) - onehot) / denom  (0 on rows >= n_valid)
        mag_loss = (1/denom) sum_r (|m_r| + |log s_r| + |x_{r,y}|),     mag_grad = 1 / denom  (every element)

    A row whose label is outside [0, c) is the kernel's refused row: no loss term, no one-hot (the softmax alone).  A -inf logit
    is evaluated at its limit (replaced by -1e4: its exponential is exactly 0); a -inf logit ON the label makes the loss +inf.
    ``acc=torch.float32`` is the kernel's restatement: max, exp2(fl((x - m) * log2 e)) with fp32-subnormal results flushed, sum,
    one reciprocal, (p - onehot) * inv_n, then rbf; the row losses m + log s - x_y summed in fp32 and scaled by inv_n.
    ``fault`` (tests/test_bounds.py), a dict of
      no_onehot: True;  onehot_shift: +-1 (the one-hot lands on class y + shift);  inv_n_rows: True (1 / n instead of 1 / denom);
      no_max: True (exponentials of x itself);  drop_tail: True (classes >= 64 * (c // 64) left out of the sum and the gradient);
      drop_rows_loss: True (rows >= 4096 left out of the loss sum);  no_round_sum: True (x + x2 not rounded to bf16).
    The magnitudes never see the fault."""
    fault = fault or {}
    n, c = x.shape
    dev = x.device
    if x2 is not None:
        xs = x.float() + x2.float()
        xq = xs.bfloat16()
        X = (x.double() + x2.double()).to(acc) if fault.get("no_round_sum") else xq.to(acc)
        Xm = xq.double()
    else:
        X, Xm = x.to(acc), x.double()
    n_valid = n if n_valid is None else max(0, min(int(n_valid), n))
    labels = labels.long().to(dev)
    ok = (labels >= 0) & (labels < c)
    ok[n_valid:] = False
    ys = torch.where(ok, labels, torch.zeros_like(labels))
    label_inf = bool((torch.isinf(Xm.gather(1, ys[:, None])[:, 0]) & ok).any())
    X = torch.where(torch.isinf(X) & (X < 0), torch.full_like(X, _NEG_LIMIT), X)
    Xm = torch.where(torch.isinf(Xm) & (Xm < 0), torch.full_like(Xm, _NEG_LIMIT), Xm)
    inv_n = torch.tensor(1.0 / (n if fault.get("inv_n_rows") else denom), dtype=acc, device=dev)
    m = torch.zeros(n, 1, dtype=acc, device=dev) if fault.get("no_max") else X.amax(1, keepdim=True)
    if acc == torch.float32:
        e = torch.exp2((X - m) * torch.tensor(1.4426950408889634, dtype=acc, device=dev))
        e = torch.where(e < 2.0 ** -126, torch.zeros_like(e), e)
    else:
        e = torch.exp(X - m)
    cols = torch.arange(c, device=dev)
    if fault.get("drop_tail"):
        e = e * (cols < 64 * (c // 64)).to(acc)
    s = e.sum(1, keepdim=True)
    p = e * (1.0 / s)
    shift = int(fault.get("onehot_shift", 0))
    hot = (cols[None, :] == (ys[:, None] + shift)) & ok[:, None]
    if fault.get("no_onehot"):
        hot = torch.zeros_like(hot)
    grad = (p - hot.to(acc)) * inv_n
    if fault.get("drop_tail"):
        grad = grad * (cols < 64 * (c // 64)).to(acc)
    grad[n_valid:] = 0
    xy = X.gather(1, ys[:, None])[:, 0]
    rows = torch.where(ok, m[:, 0] + torch.log(s[:, 0]) - xy, torch.zeros_like(xy))
    if fault.get("drop_rows_loss"):
        rows = rows[:CE_GRID_ROWS]
    loss = rows.sum() * inv_n
    if label_inf:
        loss = torch.full_like(loss, float("inf"))
    # magnitudes, float64 on the unfaulted operands
    mm = Xm.amax(1, keepdim=True)
    sm = torch.exp(Xm - mm).sum(1)
    mag_rows = torch.where(ok, mm[:, 0].abs() + torch.log(sm).abs() + Xm.gather(1, ys[:, None])[:, 0].abs(), torch.zeros_like(sm))
    mag_loss = mag_rows.sum() / denom
    if acc == torch.float32:
        grad = rbf(grad)
    return loss, mag_loss, grad, torch.full((n, c), 1.0 / denom, dtype=torch.float64, device=dev)


def ce_k(n_cls):
    """k of the gradient bound |got - ref| <= 1 ulp_bf16(ref) + k 2^-24 / denom (tests/test_gpu_cross_entropy.py):
    17 + 3 ln(n_cls) + ceil(n_cls / 64)."""
    import math
    return 17.0 + 3.0 * math.log(n_cls) + -(-n_cls // 64)


def ce_k_loss(n_rows, n_cls):
    """k_loss of the loss bound |got - ref| <= k_loss 2^-24 mag_loss: the row's chain 3 ln(n_cls) + ceil(n_cls / 64) + 13 plus
    the row-ordered sum's ceil(n_rows / 256) + 12."""
    import math
    return 3.0 * math.log(n_cls) + -(-n_cls // 64) + 13.0 + -(-n_rows // 256) + 12.0


def ce_check(got_loss, got_grad, x, labels, denom, what, x2=None, n_valid=None, loss_bf16=False, skip_rows=None):
    """Both bounds on one launch's results against ce_terms in float64; prints the two ratios before it asserts and returns them.
    ``loss_bf16``: the loss went through bf16 (CrossEntropyLoss.forward): one bf16 ulp on top.  ``skip_rows``: rows that hold a
    planted non-finite logit whose gradient the caller checks itself (the loss is then not held to the bound either)."""
    n, c = x.shape
    loss, mag_loss, grad, mag = ce_terms(x, labels, denom, x2=x2, n_valid=n_valid)
    got_grad = got_grad.double()
    if skip_rows is not None and len(skip_rows):
        keep = torch.ones(n, dtype=torch.bool, device=x.device)
        keep[torch.as_tensor(skip_rows, dtype=torch.long, device=x.device)] = False
        got_grad, grad, mag = got_grad[keep], grad[keep], mag[keep]
    ratio = assert_within(got_grad, grad, mag, 1, ce_k(c) * 2.0 ** -16, what + " gradient")
    got_loss = got_loss.double().reshape(())
    if skip_rows is not None and len(skip_rows):
        loss_ratio = 0.0
    elif bool(torch.isinf(loss)):
        loss_ratio = 0.0 if float(got_loss) == float("inf") else float("inf")
    else:
        bound = ce_k_loss(n, c) * 2.0 ** -24 * float(mag_loss) + (float(ulp_bf16(loss)) if loss_bf16 else 0.0)
        err = abs(float(got_loss) - float(loss))
        loss_ratio = 0.0 if err == 0 else (err / bound if bound > 0 else float("inf"))
    print("%s: gradient worst ratio %.3f, loss %.9g ref %.9g ratio %.3f" % (what, ratio, float(got_loss), float(loss), loss_ratio))
    assert loss_ratio <= 1.0, (what, float(got_loss), float(loss), loss_ratio)
    return ratio, loss_ratio


CE_SHAPES = [(256, 41), (1000, 100), (7, 1000), (32, 3), (1, 1), (5, 2), (300, 63), (300, 64), (300, 65), (33, 128), (33, 129),
             (4096, 7), (4097, 7), (9001, 3)]
CE_PLANTS = [0.0, -0.0, 88.0, -88.0, 200.0, -200.0]


def ce_case(shape, scale, confident, seed):
    """bf16 logits N(0, 1) * scale with the plants 0, -0, +-88, +-200 in the first entries, labels uniform over the classes;
    ``confident``: every row's label logit raised by 30 (p_y within 1e-13 of 1 at scale 1: the cancellation in p - 1).  CPU."""
    gen = torch.Generator().manual_seed(seed)
    n, c = shape
    x = torch.randn(n, c, generator=gen) * scale
    y = torch.randint(0, c, (n,), generator=gen)
    if confident:
        x[torch.arange(n), y] += 30.0
    x = x.bfloat16()
    k = min(len(CE_PLANTS), n * c)
    x.view(-1)[:k] = torch.tensor(CE_PLANTS[:k]).bfloat16()
    return x, y


# ------------------------------------------------------------------------------------------------ Adam (csrc/optim.hip)
ADAM_PER_WG = 2048                       # elements of one workgroup of k_adam
ADAM_SIZES = [(2047,), (2048,), (2049,), (1,), (4096,), (4097,), (0,), (256, 602)]


def adam_terms(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, fault=None, acc=torch.float64):
    """One step of torch.optim.Adam (no amsgrad, L2 weight decay) on bf16 p, g, m, v: returns (p', mag_p, m', mag_m, v', mag_v).
    ``step`` is the count BEFORE the step (what state[0] holds); lr, betas, eps, weight_decay enter as the fp32 values the C ABI
    receives (rounded here).

        gw = g + wd p;  m' = m + (gw - m)(1 - b1);  v' = b2 v + (1 - b2) gw^2;  t = step + 1
        denom = sqrt(v') / sqrt(1 - b2^t) + eps;  update = lr / (1 - b1^t) * m' / denom;  p' = p - update

    Magnitudes (the same formulas on the absolute values of their terms):
        mag_m = |m| + (1 - b1)(|g| + wd |p| + |m|)
        mag_v = b2 v + (1 - b2)(|g| + wd |p|)^2                      (= v' unless g and wd p cancel)
        mag_p = |p| + lr / (1 - b1^t) * mag_m / denom * (mag_v / v')   (= |p| + |update| unless m' or g + wd p cancels: an error
                of m' reaches p' at the scale of mag_m, not of |m'|, and one of v' at the scale of mag_v)
    ``acc=torch.float32`` is the kernel's restatement (every operation in fp32, results rounded with rbf).  ``fault``:
      no_wd, bias_at_step (corrections at ``step`` instead of step + 1), eps_inside (sqrt(v' / bc2 + eps)), beta1_swapped (beta1
      where 1 - beta1 belongs), skip_block_last (the last element of every 2048-block keeps p, m, v), g_other (a tensor read as
      the gradient instead of g).  The magnitudes never see the fault."""
    fault = fault or {}
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay)
    shape = p.shape
    P, M, V = p.reshape(-1).to(acc), m.reshape(-1).to(acc), v.reshape(-1).to(acc)
    G = (fault["g_other"] if "g_other" in fault else g).reshape(-1).to(acc)
    c = lambda val: torch.tensor(val, dtype=acc, device=p.device)
    one = c(1.0)
    gw = G if (wd == 0.0 or fault.get("no_wd")) else G + c(wd) * P
    w1 = c(b1) if fault.get("beta1_swapped") else one - c(b1)
    m2 = M + (gw - M) * w1
    v2 = c(b2) * V + (one - c(b2)) * gw * gw
    t = float(step) + (0.0 if fault.get("bias_at_step") else 1.0)
    bc1, bc2 = one - torch.pow(c(b1), c(t)), one - torch.pow(c(b2), c(t))
    if fault.get("eps_inside"):
        denom = torch.sqrt(v2 / bc2 + c(eps))
    else:
        denom = torch.sqrt(v2) / torch.sqrt(bc2) + c(eps)
    p2 = P - (c(lr) / bc1) * (m2 / denom)
    if fault.get("skip_block_last"):
        last = torch.arange(ADAM_PER_WG - 1, P.numel(), ADAM_PER_WG, device=p.device)
        p2[last], m2[last], v2[last] = P[last], M[last], V[last]
    # magnitudes: float64, exact step, no fault
    Pd, Gd, Md, Vd = p.reshape(-1).double().abs(), g.reshape(-1).double().abs(), m.reshape(-1).double().abs(), v.reshape(-1).double()
    gm = Gd + wd * Pd
    mag_m = Md + (1.0 - b1) * (gm + Md)
    mag_v = b2 * Vd + (1.0 - b2) * gm * gm
    gx = g.reshape(-1).double() + wd * p.reshape(-1).double()
    vx = b2 * Vd + (1.0 - b2) * gx * gx
    dx = vx.sqrt() / (1.0 - b2 ** (step + 1.0)) ** 0.5 + eps
    rho = torch.where(vx > 0, mag_v / vx.clamp(min=1e-300), torch.ones_like(vx))
    mag_p = Pd + lr / (1.0 - b1 ** (step + 1.0)) * mag_m / dx * rho
    if acc == torch.float32:
        p2, m2, v2 = rbf(p2), rbf(m2), rbf(v2)
    r = lambda t_: t_.reshape(shape)
    return r(p2), r(mag_p), r(m2), r(mag_m), r(v2), r(mag_v)


def adam_k(step, beta1, beta2):
    """(k_ulp, k_mag) of p', m', v' for the step count ``step`` before the update (tests/test_gpu_adam.py derives them): k_mag in
    units of 2^-8 as assert_within takes it.  C(b, t) = 1 + 4 b^t / (1 - b^t) is the conditioning of 1 - b^t in fp32."""
    b1, b2, t = f32(beta1), f32(beta2), step + 1.0
    cond = lambda b: 1.0 + 4.0 * b ** t / (1.0 - b ** t)
    return {"p": (1, (25.0 + cond(b1) + 0.5 * cond(b2)) * 2.0 ** -16), "m": (1, 5.0 * 2.0 ** -16), "v": (1, 8.0 * 2.0 ** -16)}


def adam_case(shape, g_scale, m_sign, v0, seed):
    """bf16 (p, g, m, v) of one tensor: p ~ 0.1 N(0, 1), g ~ g_scale N(0, 1) (exactly 0 with g_scale 0), m = m_sign * sign(g) *
    |0.5 g_scale N(0, 1)| (0.01 N(0, 1) where g is 0), v = v0 * (0.5 + U(0, 1)) (0 with v0 0).  CPU."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(shape, generator=gen) * 0.1
    g = torch.randn(shape, generator=gen) * g_scale
    a = torch.randn(shape, generator=gen).abs()
    m = m_sign * torch.sign(g) * a * 0.5 * g_scale if g_scale else torch.randn(shape, generator=gen) * 0.01
    v = (torch.rand(shape, generator=gen) + 0.5) * v0
    return p.bfloat16(), g.bfloat16(), m.bfloat16(), v.bfloat16()
