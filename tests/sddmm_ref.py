"""Restatement of the per-edge dot product kernel (csrc/sddmm.hip) in vectorised torch: the kernel's own
fp32 sum order (``dot_f32``, bit-equal to the kernel), the fp64 value with its magnitude (``terms``) and the constants of the
bound.  A plain helper module like bounds.py; works on any device.

    dot_e  = sum_c a[dst_e, c] * b[src_e, c]          (MAX: only the columns c with arg[dst_e, c] == e)
    out[e] = round(dot_e * coef_e)                     coef: 1 (SUM, MAX), 1 / max(deg, 1) (MEAN), 1 / (deg + 1) (SELF)

The kernel's order: the columns are cut into groups of 8; group g belongs to lane g % 16; a lane starts from +0 and adds its
products in ascending column order; the 16 lane sums are added as a balanced tree of neighbours; then the coefficient."""
import torch

import bounds

SUM, MEAN, SELF, MAX = 0, 1, 2, 3          # BLISS_SDDMM_*
LANES, GROUP = 16, 8


def _edges(spec, device, live=None):
    B = spec.B if live is None else int(live)
    return spec.src[:B].long().to(device), spec.dst[:B].long().to(device)


def coef_f32(spec, mode, device, live=None, deg=None):
    """fp32 coefficient per edge, computed as the kernel does: 1.0f / (float)n."""
    src, dst = _edges(spec, device, live)
    if mode in (SUM, MAX):
        return torch.ones(dst.numel(), dtype=torch.float32, device=device)
    if deg is None:
        deg = spec.in_degrees().to(device)
    n = deg.clamp(min=1) if mode == MEAN else deg + 1
    return (torch.ones((), dtype=torch.float32, device=device) / n.float())[dst]


def dot_f32(spec, a, b, mode, arg=None, live=None, out_fp32=False):
    """The kernel's result for the first ``live`` (default: all) edges of ``spec``, in its own fp32 order: bf16 [B] (fp32 with
    ``out_fp32``).  a bf16 [>= S, dim] by destination, b bf16 [>= K, dim] by source, arg int [>= S, dim] for MAX."""
    dev = a.device
    src, dst = _edges(spec, dev, live)
    B, dim = src.numel(), a.shape[1]
    prod = a.float()[dst] * b.float()[src]                                      # fp32 products, one rounding each
    if mode == MAX:
        e = torch.arange(B, device=dev)
        prod = torch.where(arg.to(dev).long()[dst] == e[:, None], prod, torch.zeros_like(prod))
    span = LANES * GROUP
    P = (dim + span - 1) // span
    pad = torch.zeros(B, P * span, dtype=torch.float32, device=dev)
    pad[:, :dim] = prod
    pad = pad.view(B, P, LANES, GROUP)
    acc = torch.zeros(B, LANES, dtype=torch.float32, device=dev)
    for p in range(P):                                                          # a lane: ascending columns, one add each
        for k in range(GROUP):
            acc = acc + pad[:, p, :, k]
    while acc.shape[1] > 1:                                                     # the tree: neighbours, then pairs of pairs, ...
        acc = acc[:, 1::2] + acc[:, 0::2]
    out = acc[:, 0] * coef_f32(spec, mode, dev, live)
    return out if out_fp32 else out.bfloat16()


def terms(spec, a, b, mode, arg=None, live=None, fault=None):
    """(ref, mag) float64 [B]: the value coef * sum a b and the magnitude coef * sum |a| |b| (MAX: over the won columns).
    ``fault`` (planted, for the bound's own test): "drop_col" leaves column 0 out of the sum, "wrong_deg" takes the degree of the
    NEXT destination."""
    dev = a.device
    src, dst = _edges(spec, dev, live)
    A, Bm = a.double()[dst], b.double()[src]
    keep = torch.ones_like(A, dtype=torch.bool)
    if mode == MAX:
        keep = arg.to(dev).long()[dst] == torch.arange(src.numel(), device=dev)[:, None]
    kf = keep.clone()
    if fault == "drop_col":
        kf[:, 0] = False
    deg = spec.in_degrees().to(dev).double()
    degf = torch.roll(deg, -1) if fault == "wrong_deg" else deg

    def coef(dg):
        if mode == MEAN:
            return 1.0 / dg.clamp(min=1)[dst]
        if mode == SELF:
            return 1.0 / (dg + 1)[dst]
        return torch.ones(dst.numel(), dtype=torch.float64, device=dev)

    val = (A * Bm * kf).sum(1) * coef(degf)
    mag = (A.abs() * Bm.abs() * keep).sum(1) * coef(deg)
    return val, mag


def k(dim):
    """(k_ulp, k_mag) of one kernel result: ``dim`` fp32 products and sums, the coefficient product and the reciprocal."""
    return bounds.dense_k(dim + 2)


def k_agg_dual(dim, out_feats):
    """(k_ulp, k_mag) of _SageAggDual's gw: the kernel's own terms on top of two stored bf16 operands -- d W_neigh (1) and the
    epilogue gradient it is made of (1) -- and that product's fp32 accumulation over ``out_feats`` terms."""
    return bounds.dense_k(dim + 2, stored=2.0 + out_feats * 2.0 ** -16)


def loop_ref(spec, a, b, mode, arg=None):
    """Plain Python, edge by edge, float64 (the CPU check of the restatement)."""
    out = []
    deg = spec.in_degrees().tolist()
    for e in range(spec.B):
        s, d = int(spec.src[e]), int(spec.dst[e])
        t = 0.0
        for c in range(a.shape[1]):
            if mode == MAX and int(arg[d, c]) != e:
                continue
            t += float(a[d, c]) * float(b[s, c])
        if mode == MEAN:
            t /= max(deg[d], 1)
        elif mode == SELF:
            t /= deg[d] + 1
        out.append(t)
    return torch.tensor(out, dtype=torch.float64)


def operands(spec, dim, seed, device, S=None, K=None, sliced=False):
    """bf16 a [S, dim] (d out) and b [K, dim] (features), N(0, 1); ``sliced``: columns 1 .. dim of a tensor 3 wider (row stride
    dim + 3, base 2 bytes past an aligned address)."""
    gen = torch.Generator().manual_seed(seed)
    S, K = spec.S if S is None else S, spec.K if K is None else K
    wide = dim + 3 if sliced else dim
    a = torch.randn(S, wide, generator=gen).bfloat16().to(device)
    b = torch.randn(K, wide, generator=gen).bfloat16().to(device)
    return (a[:, 1:1 + dim], b[:, 1:1 + dim]) if sliced else (a, b)
