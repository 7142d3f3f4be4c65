"""Restatement of csrc/gcn.hip: GraphConv(norm='both') message passing with the degree norms inside the
SpMM, the row-wise epilogue with the keyed dropout mask, and a whole layer -- in float64 with magnitudes (tests/bounds.py's
convention: ``mag`` is the formula on the absolute values of its terms) and, with ``sim=True``, with the roundings the kernels
store (fp32 norms and coefficients, one bf16 rounding per stored tensor).  A plain helper module like bounds.py.

    ns_j = 1 / sqrt(max(outdeg_j, 1))     nd_i = 1 / sqrt(max(indeg_i, 1))            (structural degrees of the block)
    fwd: out[i] = nd_i * sum_{e in row i}    (w_e * ns[src_e]) * h[src_e]
    bwd: gh[j]  = ns_j * sum_{e : src_e = j} (w_e * nd[dst_e]) * g[dst_e]
    epilogue:  x = bf16(a + bias);  relu;  keep ? bf16(x / (1 - p)) : 0  with keep = hash(seed, ctr, r * width + c) >= p 2^32
    epilogue backward:  g_pre = keep ? bf16(g / (1 - p)) : 0, zero where the stored output is <= 0 (relu);  db = sum_{r < live} g_pre

``fault`` plants one error (tests/test_gcn_ref.py shows that each fails the constants the GPU suite uses); the magnitudes never
see the fault or the rounding."""
import numpy as np
import torch

from bounds import rbf
from gat_glue_ref import drop_scale, keep_mask
from gat_glue_ref import rbf as rbf_np


# ------------------------------------------------------------------------------------------------ norms and SpMM
def norms(src, dst, K, S, sim=False, fault=None):
    """(ns [K], nd [S]) as float64 tensors on src's device.  ``sim``: the fp32 values of k_gcn_norms (IEEE sqrt, one division --
    NumPy's float32 sqrt and division are the same operations).  fault: ns_one = a source id whose norm is taken as 1;
    nd_unclamped = True: 1 / sqrt(indeg) without the clamp (inf on a row without edges)."""
    fault = fault or {}
    dev = src.device
    outdeg = torch.bincount(src.long(), minlength=K).cpu().numpy()
    indeg = torch.bincount(dst.long(), minlength=S).cpu().numpy()
    ind = indeg if fault.get("nd_unclamped") else np.maximum(indeg, 1)
    if sim:
        with np.errstate(divide="ignore"):
            ns = (np.float32(1.0) / np.sqrt(np.maximum(outdeg, 1).astype(np.float32))).astype(np.float64)
            nd = (np.float32(1.0) / np.sqrt(ind.astype(np.float32))).astype(np.float64)
    else:
        with np.errstate(divide="ignore"):
            ns = 1.0 / np.sqrt(np.maximum(outdeg, 1).astype(np.float64))
            nd = 1.0 / np.sqrt(ind.astype(np.float64))
    if "ns_one" in fault:
        ns[int(fault["ns_one"])] = 1.0
    return torch.from_numpy(ns).to(dev), torch.from_numpy(nd).to(dev)


def spmm_terms(src, dst, S, K, h, w=None, by_src=False, sim=False, fault=None):
    """(ref, mag) float64 of bliss_gcn_spmm_fwd (h [K, dim] -> [S, dim]) or, ``by_src``, of bliss_gcn_spmm_bwd (h = gout [S, dim] ->
    [K, dim]).  ``sim``: fp32 norms, the coefficient rounded to fp32, the result rounded to bf16.  fault: ns_one, nd_unclamped
    (see ``norms``) and drop_edges = edge ids left out of the sum."""
    fault = fault or {}
    src, dst = src.long(), dst.long()
    ns, nd = norms(src, dst, K, S, sim=sim, fault=fault)
    ns0, nd0 = norms(src, dst, K, S)
    H = h.double()
    wd = torch.ones(src.numel(), dtype=torch.float64, device=H.device) if w is None else w.double().reshape(-1)
    rows, nbrs, n_out = (src, dst, K) if by_src else (dst, src, S)
    n_nbr, n_row, m_nbr, m_row = (nd, ns, nd0, ns0) if by_src else (ns, nd, ns0, nd0)
    c = wd * n_nbr[nbrs]
    if sim:
        c = c.float().double()
    keep = torch.ones_like(c)
    if "drop_edges" in fault:
        keep[torch.as_tensor(fault["drop_edges"], dtype=torch.long, device=c.device)] = 0.0
    zero = lambda: torch.zeros(n_out, H.shape[1], dtype=torch.float64, device=H.device)
    ref = n_row[:, None] * zero().index_add_(0, rows, (c * keep)[:, None] * H[nbrs])
    mag = m_row[:, None] * zero().index_add_(0, rows, (wd.abs() * m_nbr[nbrs])[:, None] * H[nbrs].abs())
    return (rbf(ref) if sim else ref), mag


# ------------------------------------------------------------------------------------------------ epilogue (NumPy, exact)
def _f32(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32))


def epilogue_fwd(a, bias, relu, p=0.0, seed=0, ctr=0, n_live=None):
    """out [rows, width] float32 holding bf16 numbers: rows >= n_live are zeros and their inputs are not looked at."""
    a = _f32(a)
    rows, width = a.shape
    n = rows if n_live is None else max(0, min(int(n_live), rows))
    out = np.zeros((rows, width), np.float32)
    x = a[:n]
    if bias is not None:
        x = rbf_np(x + _f32(bias)[None, :])
    if relu:
        x = np.where(x > 0, x, np.float32(0))
    if p > 0:
        x = np.where(keep_mask(rows, width, p, seed, ctr)[:n], rbf_np(x * drop_scale(p)), np.float32(0))
    out[:n] = x
    return out


def epilogue_bwd(dout, out, relu, p=0.0, seed=0, ctr=0, n_live=None, fault=None):
    """(din [rows, width] float32 holding bf16 numbers, db float64 [width] = the exact column sums of din's live rows, mag_db).
    fault: no_drop_scale (the mask without 1 / (1 - p)); db_extra_rows = n: that many rows at and past the count join db."""
    fault = fault or {}
    dout = _f32(dout)
    rows, width = dout.shape
    n = rows if n_live is None else max(0, min(int(n_live), rows))
    din = np.zeros((rows, width), np.float32)
    extra = min(rows, n + int(fault.get("db_extra_rows", 0)))
    g = dout[:extra].copy()
    if p > 0:
        scale = np.float32(1.0) if fault.get("no_drop_scale") else drop_scale(p)
        g = np.where(keep_mask(rows, width, p, seed, ctr)[:extra], rbf_np(g * scale), np.float32(0))
    if relu:
        g = np.where(_f32(out)[:extra] > 0, g, np.float32(0))
    din[:n] = g[:n]
    db = g.astype(np.float64).sum(0)
    mag_db = np.abs(g[:n].astype(np.float64)).sum(0)
    return din, db, mag_db


def row_norm(out):
    """fp64 row norms of the stored rows (bliss_embed_norm's value; its fp32 summation order is checked on the device against
    bliss_embed_norm itself)."""
    return np.sqrt((_f32(out).astype(np.float64) ** 2).sum(1))


# ------------------------------------------------------------------------------------------------ a whole layer
def layer_terms(src, dst, S, K, x, W, b, w=None, g=None, mask=None):
    """GraphConv(norm='both') with edge weights, fp64 autograd of the formula on the bf16 operands:
        rst = nd * A_w(ns * (x W)) + b        (A_w: the weighted sum over in-edges; the product order does not matter in fp64)
        out = mask * rst                      (``mask``: the ReLU's, taken by the caller from the kernel's stored output; None: ones)
    x [K, in], W [in, out], b [out] or None, g = d out [S, out].  Returns a dict: rst, mag_rst and with g: d_x, d_W, d_b and
    mag_d_x, mag_d_W, mag_d_b."""
    src, dst = src.long(), dst.long()
    dev = x.device
    ns, nd = norms(src, dst, K, S)
    wd = torch.ones(src.numel(), dtype=torch.float64, device=dev) if w is None else w.double().reshape(-1)
    agg = lambda t, c: torch.zeros(S, t.shape[1], dtype=torch.float64, device=dev).index_add_(0, dst, c[:, None] * t[src])
    agg_t = lambda t, c: torch.zeros(K, t.shape[1], dtype=torch.float64, device=dev).index_add_(0, src, c[:, None] * t[dst])
    X = x.detach().double().requires_grad_(True)
    Wd = W.detach().double().requires_grad_(True)
    bd = None if b is None else b.detach().double().requires_grad_(True)
    rst = nd[:, None] * agg((X * ns[:, None]) @ Wd, wd)
    mag = nd[:, None] * agg((X.detach().abs() * ns[:, None]) @ Wd.detach().abs(), wd.abs())
    if bd is not None:
        rst = rst + bd
        mag = mag + bd.detach().abs()
    out = dict(rst=rst.detach(), mag_rst=mag)
    if g is None:
        return out
    G = g.double()
    if mask is not None:
        G = G * mask.double()
    (rst * G).sum().backward()
    mid = ns[:, None] * agg_t(nd[:, None] * G.abs(), wd.abs())                   # |d (x W)| by source row
    out.update(d_x=X.grad, d_W=Wd.grad, d_b=None if bd is None else bd.grad, mag_d_x=mid @ Wd.detach().abs().t(),
               mag_d_W=X.detach().abs().t() @ mid, mag_d_b=G.abs().sum(0))
    return out


def layer_k(fin, fout, rows):
    """(k_ulp, k_mag) per tensor of a tile GraphConv layer on ``rows`` = max(K, S) block rows, from where the kernels round
    (bounds.dense_k: an fp32-accumulated product costs n_terms 2^-16; a bf16 tensor stored between two launches 1; a stored SpMM
    result 1.25, SPMM_K's fp32 sum included); the last rounding of each tensor is k_ulp:
      out:  the product (fin terms) and the SpMM result are stored, in either order, in front of the epilogue's add: 2.25
      d x:  weight first: dZ (SpMM, 1.25) in front of the product (fout terms); aggregate first: the product stored (1) in front
            of the SpMM, whose own sum adds 0.25: 1.25 either way
      d W:  weight first: dZ (1.25); aggregate first: the stored aggregate (1.25); the row sum of bliss_sage_wgrad (rows terms + at
            most 80 chunk partials)
      d b:  fp32 sums of the epilogue's gradient rows (rows terms + rows / 32 chunk partials), nothing stored in front.
    All below the library path's GCN_K = (1, 4)."""
    return {"out": (1, 2.25 + (fin + 1) * 2.0 ** -16), "d_x": (1, 1.25 + fout * 2.0 ** -16), "d_W": (1, 1.25 + (rows + 80) * 2.0 ** -16),
            "d_b": (1, (rows + rows // 32 + 1) * 2.0 ** -16)}


# the SpMM's own constants: k_ulp = 1 for the one rounding; k_mag: the fp32 sum of at most 16 384 terms (2^14 2^-24 = 2^-10 of the
# magnitude = 0.25 units of 2^-8) -- the fp32 norms, the coefficient and the store scale add 4 2^-24, far inside it
GCN_SPMM_K = (1, 0.25)
