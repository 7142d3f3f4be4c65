"""The max-reduce message passing of SAGEConv('pool') restated in vectorised torch, on any device:

    m_e[c]    = bf16(float(w_e) * float(h[src_e, c]))        (w absent: m_e = h[src_e])
    arg[i, c] = the lowest edge e among the in-edges of i whose m_e[c] is largest (float comparison: -0.0 == 0.0)
    out[i, c] = m_arg[c];  a row without edges: out = 0, arg = -1
    gh[j, c]  = sum_{e : src_e = j and arg[dst_e, c] == e} float(w_e) * float(gout[dst_e, c])      (float64 here)

A plain helper module like bounds.py.  "The lowest edge whose message equals the row's maximum" is what the serial rule -- the
running best moves on strict > only -- ends with, for finite inputs; tests/test_spmm_max_ref.py checks it against that loop."""
import torch


def messages(src, h, w=None):
    """float32 [B, dim], every value a bf16 value: the messages as DGL materialises them."""
    m = h[src.long()].float()
    if w is not None:
        m = (w.float().reshape(-1, 1) * m).bfloat16().float()       # the fp32 product of two bf16 values is exact: one rounding
    return m


def forward(src, dst, S, h, w=None):
    """(m float32 [B, dim], out bf16 [S, dim], arg int32 [S, dim]) of the block with edges (src, dst) in CSR-by-destination
    order (dst non-decreasing) and S destinations."""
    src, dst = src.long(), dst.long()
    m = messages(src, h, w)
    B, D = m.shape
    if B == 0:
        return m, torch.zeros(S, D, dtype=torch.bfloat16, device=h.device), torch.full((S, D), -1, dtype=torch.int32, device=h.device)
    idx = dst[:, None].expand(-1, D)
    mx = torch.full((S, D), -float("inf"), device=m.device).scatter_reduce(0, idx, m, "amax", include_self=True)
    e = torch.arange(B, device=m.device)[:, None].expand(-1, D)
    cand = torch.where(m == mx[dst], e, torch.full_like(e, B))
    arg = torch.full((S, D), B, dtype=torch.int64, device=m.device).scatter_reduce(0, idx, cand, "amin", include_self=True)
    empty = arg == B
    out = torch.where(empty, torch.zeros((), device=m.device), m.gather(0, arg.clamp(max=B - 1)))
    arg = torch.where(empty, torch.full_like(arg, -1), arg)
    return m, out.bfloat16(), arg.to(torch.int32)


def backward(src, K, gout, arg, w=None):
    """(gh, mag) float64 [K, dim]: every element (i, c) with arg >= 0 sends w_arg * gout[i, c] to row src[arg] of column c;
    ``mag`` is the same sum over the absolute values of the terms."""
    src = src.long()
    S, D = arg.shape
    valid = arg >= 0
    e = arg.clamp(min=0).long()
    g = gout.double()
    if src.numel() == 0:
        z = torch.zeros(K, D, dtype=torch.float64, device=g.device)
        return z, z.clone()
    coef = torch.ones(S, D, dtype=torch.float64, device=g.device) if w is None else w.double().reshape(-1)[e]
    term = torch.where(valid, coef * g, torch.zeros((), dtype=torch.float64, device=g.device))
    rows = src[e]
    gh = torch.zeros(K, D, dtype=torch.float64, device=g.device).scatter_add_(0, rows, term)
    mag = torch.zeros(K, D, dtype=torch.float64, device=g.device).scatter_add_(0, rows, term.abs())
    return gh, mag


def loop(indptr, src, S, h, w=None):
    """The definition as a plain Python loop (serial first-wins, strict >): (out float [S][dim], arg int [S][dim]) as lists."""
    D = h.shape[1]
    hf = h.float()
    out, arg = [[0.0] * D for _ in range(S)], [[-1] * D for _ in range(S)]
    for i in range(S):
        for c in range(D):
            best, be = None, -1
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                v = hf[int(src[e]), c]
                if w is not None:
                    v = (w[e].float() * v).bfloat16().float()
                v = float(v)
                if be < 0 or v > best:
                    best, be = v, e
            if be >= 0:
                out[i][c], arg[i][c] = best, be
    return out, arg
