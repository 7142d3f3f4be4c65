"""The SAGEConv('pool') layer on the tile kernels restated in float64 torch, on any device -- a plain helper
module like bounds.py and spmm_max_ref.py.

The masked max backward (bliss_spmm_max_bwd_relu):

    gz[j, c] = act[j, c] > 0 ? sum_{e : src_e = j, arg[dst_e, c] == e} float(w_e) * float(gout[dst_e, c]) : +0

= spmm_max_ref.backward(...) times (act > 0): act = +0.0 and act = -0.0 both mask, and a masked element is +0.

The layer, with the points where the kernels round to bf16 (``sim=True`` rounds there, ``sim=False`` is plain float64):

    pooled  = R( relu(h Wp^T + bp) )                                  fp32 accumulation, bias, ReLU, one rounding
    m_e, neigh, arg                                                   spmm_max_ref.forward on pooled (section 30's, unchanged)
    out     = R( keep / (1 - p) * relu(neigh Wn^T + h[:S] Ws^T + bs) )   both products and the bias in one accumulator, ReLU,
                                                                      dropout, one rounding (``relu=False``: the last layer)
    d       = R( gout / (1 - p) ) where out > 0, else 0               the epilogue backward's single rounding (no ReLU, p = 0: d = gout)
    d_neigh = R( d Wn )
    d_z     = R( masked backward of d_neigh through arg, act = pooled )   one rounding, then the mask
    dW_neigh = R( d^T neigh ), dW_self = R( d^T h[:S] ), db_self = R( sum d ), dW_pool = R( d_z^T h ), db_pool = R( sum d_z )
    dh      = R( d_z Wp + [d Ws on rows < S] )                        one accumulator, one rounding (the fused form)
"""
import torch

import spmm_max_ref as ref
from bounds import rbf


def masked_backward(src, K, gout, arg, act, w=None):
    """(gz, mag) float64 [K, dim]: spmm_max_ref.backward under the mask act > 0 (act [K, dim]); masked elements are +0."""
    gh, mag = ref.backward(src, K, gout, arg, w)
    keep = act.double() > 0
    zero = torch.zeros((), dtype=torch.float64, device=gh.device)
    return torch.where(keep, gh, zero), torch.where(keep, mag, zero)


def layer(src, dst, S, h, ew, Wp, bp, Wn, Ws, bs, relu=True, p=0.0, keep=None, gout=None, sim=True):
    """The float64 restatement above.  h [K, in], ew [B] or None, Wp [in, in], bp [in], Wn / Ws [out, in], bs [out]; ``keep``
    [S, out] bool: the dropout's keep mask (None: everything kept); ``gout`` [S, out]: d out, or None for the forward alone.
    Returns a dict of every value at a rounding point: z (before the ReLU), pooled, m, neigh, arg, pre (before the tail's ReLU),
    out and, with gout, d, d_neigh, d_a (the unmasked routed backward), d_z, d_pool (d_z Wp), d_self (d Ws), d_feat and the five
    parameter gradients under their names in SAGEConv."""
    R = rbf if sim else (lambda t: t)
    H, WP, BP, WN, WS, BS = (t.double() for t in (h, Wp, bp, Wn, Ws, bs))
    K = H.shape[0]
    w16 = None if ew is None else ew.bfloat16()
    z = H @ WP.t() + BP
    pooled = R(z.clamp(min=0))
    m, neigh, arg = ref.forward(src, dst, S, pooled.bfloat16() if sim else pooled, w16)
    m, neigh = m.double(), neigh.double()
    pre = neigh @ WN.t() + H[:S] @ WS.t() + BS
    scale = 1.0 / (1.0 - p)
    kept = torch.ones_like(pre) if keep is None else keep.double()
    out = R((pre.clamp(min=0) if relu else pre) * kept * scale)
    pts = dict(z=z, pooled=pooled, m=m, neigh=neigh, arg=arg, pre=pre, out=out)
    if gout is None:
        return pts
    G = gout.double()
    d = R(torch.where(out > 0, G * scale, torch.zeros_like(G))) if (relu or p > 0) else G
    d_neigh = R(d @ WN)
    d_a, _ = ref.backward(src, K, d_neigh, arg, w16)
    d_z, _ = masked_backward(src, K, d_neigh, arg, pooled, w16)
    d_a, d_z = R(d_a), R(d_z)
    d_pool, d_self = d_z @ WP, d @ WS
    d_feat = d_pool.clone()
    d_feat[:S] += d_self
    pts.update({"d": d, "d_neigh": d_neigh, "d_a": d_a, "d_z": d_z, "d_pool": d_pool, "d_self": d_self, "d_feat": R(d_feat),
                "fc_pool.weight": R(d_z.t() @ H), "fc_pool.bias": R(d_z.sum(0)), "fc_neigh.weight": R(d.t() @ neigh),
                "fc_self.weight": R(d.t() @ H[:S]), "fc_self.bias": R(d.sum(0))})
    return pts
