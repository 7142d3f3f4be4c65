"""The message-passing kernels as ``torch.library`` custom ops (last row): ``torch.ops.bliss.spmm``
(the weighted g-SpMM of dglnn.SAGEConv / GraphConv, [DGL-recalled] SURVEY m3, with its transposed backward m6 registered as
the op's autograd formula), ``spmm_max`` ('pool'), ``spmm_self`` ('gcn': the sum with the destination's own row, over deg + 1) and ``lstm_agg`` ('lstm': a recurrent
cell over each destination's in-edges, csrc/lstm.hip)
and ``torch.ops.bliss.embed_norm`` (model.py:318-320).  Edge weights that require a gradient get one from the three aggregation ops:
``torch.ops.bliss.sddmm``, the per-edge dot product of d out and h (csrc/sddmm.hip).  Device tensors in, device tensors out, no host sync; fake (meta) implementations make them traceable (FakeTensor / torch.compile shape propagation); the real
implementations are the C ABI calls of include/bliss_gnn.h -- there is no other backend.

``counts`` (optional int32[10] = a bliss_layer_counts_t on the device) marks capacity-padded blocks: the true edge count is
read on the device, padded edges are inert (bliss_gnn_amd._engine)."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._engine import _stream, spmm_partials


def _p(t):
    return 0 if t is None else t.data_ptr()


def _nnz_ptr(counts):
    return 0 if counts is None else counts.data_ptr() + 16          # bliss_layer_counts_t::B


def _rs(t):
    """Row stride in elements of a matrix with unit column stride (torch leaves the stride of a one-row matrix arbitrary)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _wants_grad(w):
    """setup_context only (it runs when autograd records the op): do the edge weights want a gradient?"""
    return w is not None and w.requires_grad


@torch.library.custom_op("bliss::sddmm", mutates_args=())
def sddmm(src: Tensor, dst: Tensor, indptr: Optional[Tensor], a: Tensor, b: Tensor, arg: Optional[Tensor], counts: Optional[Tensor],
          mode: int, out_fp32: bool) -> Tensor:
    """out[e] = coef_e * sum_c a[dst_e, c] b[src_e, c], one rounding (csrc/sddmm.hip) -- the per-edge dot
    product of a destination-indexed and a source-indexed bf16 matrix.  ``mode`` (_lib.SDDMM_*): SUM coef 1; MEAN 1 / max(deg, 1)
    and SELF 1 / (deg + 1) of the destination (``indptr``); MAX coef 1 over the columns ``arg[dst_e, c] == e`` only.  bf16
    [len(src)] (fp32 with ``out_fp32``); entries past a padded block's live edge count are +0.  Rows may be strided and
    unaligned (a column slice).  Forward-only."""
    assert a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.bfloat16 and a.dim() == b.dim() == 2, "bf16 matrices on the GPU"
    assert a.shape[1] == b.shape[1] and a.stride(1) == 1 and b.stride(1) == 1
    B, D = int(src.numel()), a.shape[1]
    assert dst.numel() == B
    if arg is not None:
        assert arg.dtype == torch.int32 and arg.dim() == 2 and arg.shape[1] == D and arg.stride(1) == 1
    out = torch.empty(B, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=a.device)
    _lib.check(_lib.lib.bliss_sddmm_dot(src.data_ptr(), dst.data_ptr(), _p(indptr), _nnz_ptr(counts), B, a.data_ptr(), a.stride(0),
                                        b.data_ptr(), b.stride(0), _p(arg), 0 if arg is None else arg.stride(0), D, int(mode),
                                        out.data_ptr(), int(out_fp32), _stream()), "bliss_sddmm_dot")
    return out


@sddmm.register_fake
def _(src, dst, indptr, a, b, arg, counts, mode, out_fp32):
    return a.new_empty((src.numel(),), dtype=torch.float32 if out_fp32 else torch.bfloat16)


def _sddmm_no_grad(ctx, g):
    raise NotImplementedError("bliss::sddmm is forward-only: no gradient through the per-edge dot product (no second derivative "
                              "of the aggregation ops w.r.t. their edge weights; DESIGN.md section 36)")


sddmm.register_autograd(_sddmm_no_grad)


@torch.library.custom_op("bliss::spmm", mutates_args=())
def spmm(indptr: Tensor, src: Tensor, dst: Tensor, w: Optional[Tensor], h: Tensor, n_dst: int, counts: Optional[Tensor], mean: bool,
         out_fp32: bool, t_indptr: Optional[Tensor], t_edge: Optional[Tensor]) -> Tensor:
    """out[i] = (1/deg_i if mean) * sum_{e -> i} w_e h[src_e]  -- CSR by destination (indptr, src, dst per edge)."""
    assert h.is_cuda and h.dtype == torch.bfloat16 and h.stride(1) == 1, "bf16 features on the GPU (load_graph.py:7)"
    B, D = int(src.numel()), h.shape[1]
    out = torch.empty(n_dst, D, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=h.device)
    part = spmm_partials(B, D, h.device)
    _lib.check(_lib.lib.bliss_spmm_fwd(indptr.data_ptr(), src.data_ptr(), dst.data_ptr(), _p(w), h.data_ptr(), h.stride(0), n_dst,
                                       _nnz_ptr(counts), B, D, int(mean), out.data_ptr(), out.stride(0), int(out_fp32), _p(part),
                                       _stream()), "bliss_spmm_fwd")
    return out


@spmm.register_fake
def _(indptr, src, dst, w, h, n_dst, counts, mean, out_fp32, t_indptr, t_edge):
    return h.new_empty((n_dst, h.shape[1]), dtype=torch.float32 if out_fp32 else torch.bfloat16)


@torch.library.custom_op("bliss::spmm_t", mutates_args=())
def spmm_t(t_indptr: Tensor, t_edge: Tensor, src: Tensor, dst: Tensor, indptr: Tensor, w: Optional[Tensor], gout: Tensor, n_src: int,
           counts: Optional[Tensor], mean: bool) -> Tensor:
    """The transposed product: gh[j] = sum_{e : src_e = j} (w_e / deg_{dst_e} if mean) gout[dst_e]  (by-source index t_*)."""
    B, D = int(src.numel()), gout.shape[1]
    gh = torch.empty(n_src, D, dtype=torch.bfloat16, device=gout.device)
    part = spmm_partials(B, D, gout.device)
    _lib.check(_lib.lib.bliss_spmm_bwd(t_indptr.data_ptr(), t_edge.data_ptr(), src.data_ptr(), dst.data_ptr(), indptr.data_ptr(), _p(w),
                                       gout.data_ptr(), gout.stride(0), n_src, _nnz_ptr(counts), B, D, int(mean), gh.data_ptr(),
                                       gh.stride(0), 0, _p(part), _stream()), "bliss_spmm_bwd")
    return gh


@spmm_t.register_fake
def _(t_indptr, t_edge, src, dst, indptr, w, gout, n_src, counts, mean):
    return gout.new_empty((n_src, gout.shape[1]), dtype=torch.bfloat16)


def _spmm_setup(ctx, inputs, output):
    indptr, src, dst, w, h, n_dst, counts, mean, out_fp32, t_indptr, t_edge = inputs
    ctx.need_w = _wants_grad(w)                                 # (then h is saved too: gw = the per-edge dot of d out and h)
    ctx.save_for_backward(indptr, src, dst, w, counts, t_indptr, t_edge, *((h,) if ctx.need_w else ()))
    ctx.n_src, ctx.mean = h.shape[0], mean


def _spmm_backward(ctx, gout):
    indptr, src, dst, w, counts, t_indptr, t_edge = ctx.saved_tensors[:7]
    g = gout.contiguous()
    if g.dtype != torch.bfloat16:
        g = g.bfloat16()
    gh = gw = None
    if ctx.needs_input_grad[4] or not ctx.need_w:
        if t_indptr is None or t_edge is None:
            raise RuntimeError("bliss::spmm needs the block's by-source index (Block.transposed()) to differentiate w.r.t. h")
        gh = spmm_t(t_indptr, t_edge, src, dst, indptr, w, g, ctx.n_src, counts, ctx.mean)
    if ctx.need_w:
        gw = sddmm(src, dst, indptr, g, ctx.saved_tensors[7], None, counts, _lib.SDDMM_MEAN if ctx.mean else _lib.SDDMM_SUM, False)
    return (None, None, None, gw, gh, None, None, None, None, None, None)


spmm.register_autograd(_spmm_backward, setup_context=_spmm_setup)


def _max_partials(B, D, device):
    n = int(_lib.lib.bliss_spmm_max_partial_bytes(B, D))
    if n < 0:
        raise RuntimeError("bliss_spmm_max_partial_bytes failed")
    return torch.empty(n // 4, dtype=torch.float32, device=device) if n else None


@torch.library.custom_op("bliss::spmm_max", mutates_args=())
def spmm_max(indptr: Tensor, src: Tensor, dst: Tensor, w: Optional[Tensor], h: Tensor, n_dst: int, counts: Optional[Tensor],
             want_arg: bool, t_indptr: Optional[Tensor], t_edge: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """out[i, c] = max_{e -> i} bf16(w_e h[src_e, c]), arg[i, c] = the lowest edge that attains it (-1 and 0 for a row without
    edges) -- CSR by destination (csrc/spmm_max.hip).  ``want_arg=False`` (inference): arg is empty."""
    assert h.is_cuda and h.dtype == torch.bfloat16 and h.stride(1) == 1, "bf16 features on the GPU (load_graph.py:7)"
    B, D = int(src.numel()), h.shape[1]
    out = torch.empty(n_dst, D, dtype=torch.bfloat16, device=h.device)
    arg = torch.empty((n_dst, D) if want_arg else (0, D), dtype=torch.int32, device=h.device)
    part = _max_partials(B, D, h.device)
    _lib.check(_lib.lib.bliss_spmm_max_fwd(indptr.data_ptr(), src.data_ptr(), dst.data_ptr(), _p(w), h.data_ptr(), h.stride(0), n_dst,
                                           _nnz_ptr(counts), B, D, out.data_ptr(), out.stride(0), arg.data_ptr() if want_arg else 0,
                                           D, _p(part), _stream()), "bliss_spmm_max_fwd")
    return out, arg


@spmm_max.register_fake
def _(indptr, src, dst, w, h, n_dst, counts, want_arg, t_indptr, t_edge):
    D = h.shape[1]
    return h.new_empty((n_dst, D), dtype=torch.bfloat16), h.new_empty((n_dst, D) if want_arg else (0, D), dtype=torch.int32)


@torch.library.custom_op("bliss::spmm_max_t", mutates_args=())
def spmm_max_t(t_indptr: Tensor, t_edge: Tensor, src: Tensor, dst: Tensor, w: Optional[Tensor], gout: Tensor, arg: Tensor, n_src: int,
               counts: Optional[Tensor]) -> Tensor:
    """The routed backward: gh[j, c] = sum_{e : src_e = j, arg[dst_e, c] == e} w_e gout[dst_e, c]  (by-source index t_*)."""
    B, D = int(src.numel()), gout.shape[1]
    gh = torch.empty(n_src, D, dtype=torch.bfloat16, device=gout.device)
    part = _max_partials(B, D, gout.device)
    _lib.check(_lib.lib.bliss_spmm_max_bwd(t_indptr.data_ptr(), t_edge.data_ptr(), src.data_ptr(), dst.data_ptr(), _p(w), gout.data_ptr(),
                                           gout.stride(0), arg.data_ptr(), arg.stride(0), n_src, _nnz_ptr(counts), B, D, gh.data_ptr(),
                                           gh.stride(0), _p(part), _stream()), "bliss_spmm_max_bwd")
    return gh


@spmm_max_t.register_fake
def _(t_indptr, t_edge, src, dst, w, gout, arg, n_src, counts):
    return gout.new_empty((n_src, gout.shape[1]), dtype=torch.bfloat16)


@torch.library.custom_op("bliss::spmm_max_t_relu", mutates_args=())
def spmm_max_t_relu(t_indptr: Tensor, t_edge: Tensor, src: Tensor, dst: Tensor, w: Optional[Tensor], gout: Tensor, arg: Tensor,
                    act: Tensor, n_src: int, counts: Optional[Tensor]) -> Tensor:
    """spmm_max_t under the ReLU mask of the maximised rows ``act`` = relu(z) [n_src, dim]: where(act > 0, spmm_max_t(...), +0) in
    the same two launches (bliss_spmm_max_bwd_relu); rows without a live entry are cleared unread."""
    B, D = int(src.numel()), gout.shape[1]
    assert act.dtype == torch.bfloat16 and act.shape[0] >= n_src and act.shape[1] == D and act.stride(1) == 1
    gh = torch.empty(n_src, D, dtype=torch.bfloat16, device=gout.device)
    part = _max_partials(B, D, gout.device)
    _lib.check(_lib.lib.bliss_spmm_max_bwd_relu(t_indptr.data_ptr(), t_edge.data_ptr(), src.data_ptr(), dst.data_ptr(), _p(w),
                                                gout.data_ptr(), gout.stride(0), arg.data_ptr(), arg.stride(0), act.data_ptr(),
                                                act.stride(0), n_src, _nnz_ptr(counts), B, D, gh.data_ptr(), gh.stride(0), _p(part),
                                                _stream()), "bliss_spmm_max_bwd_relu")
    return gh


@spmm_max_t_relu.register_fake
def _(t_indptr, t_edge, src, dst, w, gout, arg, act, n_src, counts):
    return gout.new_empty((n_src, gout.shape[1]), dtype=torch.bfloat16)


def _spmm_max_setup(ctx, inputs, output):
    indptr, src, dst, w, h, n_dst, counts, want_arg, t_indptr, t_edge = inputs
    ctx.need_w = _wants_grad(w)
    ctx.save_for_backward(src, dst, w, counts, t_indptr, t_edge, output[1], *((h,) if ctx.need_w else ()))
    ctx.n_src, ctx.want_arg = h.shape[0], want_arg
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)


def _spmm_max_backward(ctx, gout, _garg):
    src, dst, w, counts, t_indptr, t_edge, arg = ctx.saved_tensors[:7]
    if gout is None:
        return (None,) * 10
    g = gout.contiguous()
    if g.dtype != torch.bfloat16:
        g = g.bfloat16()
    gh = gw = None
    if ctx.needs_input_grad[4] or not ctx.need_w:
        if t_indptr is None or t_edge is None or not ctx.want_arg:
            raise RuntimeError("bliss::spmm_max needs the block's by-source index (Block.transposed()) and want_arg=True to "
                               "differentiate w.r.t. h")
        gh = spmm_max_t(t_indptr, t_edge, src, dst, w, g, arg, ctx.n_src, counts)
    if ctx.need_w:
        if not ctx.want_arg:
            raise RuntimeError("bliss::spmm_max needs want_arg=True to differentiate w.r.t. w")
        gw = sddmm(src, dst, None, g, ctx.saved_tensors[7], arg, counts, _lib.SDDMM_MAX, False)
    return (None, None, None, gw, gh, None, None, None, None, None)


spmm_max.register_autograd(_spmm_max_backward, setup_context=_spmm_max_setup)


@torch.library.custom_op("bliss::spmm_self", mutates_args=())
def spmm_self(indptr: Tensor, src: Tensor, dst: Tensor, w: Optional[Tensor], h: Tensor, h_self: Optional[Tensor], n_dst: int,
              counts: Optional[Tensor], t_indptr: Optional[Tensor], t_edge: Optional[Tensor]) -> Tensor:
    """out[i] = (sum_{e -> i} w_e h[src_e] + h_self[i]) / (deg_i + 1), one rounding -- CSR by destination (csrc/spmm_self.hip,
    DESIGN.md section 34).  ``h_self=None``: the destinations are the leading rows of ``h`` (a block)."""
    assert h.is_cuda and h.dtype == torch.bfloat16 and h.stride(1) == 1, "bf16 features on the GPU (load_graph.py:7)"
    hs = h if h_self is None else h_self
    assert hs.is_cuda and hs.dtype == torch.bfloat16 and hs.stride(1) == 1 and hs.shape[0] >= n_dst and hs.shape[1] == h.shape[1]
    B, D = int(src.numel()), h.shape[1]
    out = torch.empty(n_dst, D, dtype=torch.bfloat16, device=h.device)
    part = spmm_partials(B, D, h.device)
    _lib.check(_lib.lib.bliss_spmm_self_fwd(indptr.data_ptr(), src.data_ptr(), dst.data_ptr(), _p(w), h.data_ptr(), h.stride(0),
                                            hs.data_ptr(), hs.stride(0), n_dst, _p(counts), _nnz_ptr(counts), B, D, out.data_ptr(),
                                            out.stride(0), _p(part), _stream()), "bliss_spmm_self_fwd")
    return out


@spmm_self.register_fake
def _(indptr, src, dst, w, h, h_self, n_dst, counts, t_indptr, t_edge):
    return h.new_empty((n_dst, h.shape[1]), dtype=torch.bfloat16)


@torch.library.custom_op("bliss::spmm_self_t", mutates_args=())
def spmm_self_t(t_indptr: Tensor, t_edge: Tensor, src: Tensor, dst: Tensor, indptr: Tensor, w: Optional[Tensor], gout: Tensor, n_src: int,
                n_dst: int, counts: Optional[Tensor], fold_self: bool) -> Tensor:
    """gh[j] = sum_{e : src_e = j} w_e / (deg_{dst_e} + 1) gout[dst_e] (+ gout[j] / (deg_j + 1) on the live destination rows when
    ``fold_self``: the destinations are the leading source rows)  -- by-source index t_*."""
    B, D = int(src.numel()), gout.shape[1]
    gh = torch.empty(n_src, D, dtype=torch.bfloat16, device=gout.device)
    part = spmm_partials(B, D, gout.device)
    # without the fold no row counts as a destination: n_dst = 0 (the degrees come from indptr either way)
    _lib.check(_lib.lib.bliss_spmm_self_bwd(t_indptr.data_ptr(), t_edge.data_ptr(), src.data_ptr(), dst.data_ptr(), indptr.data_ptr(), _p(w),
                                            gout.data_ptr(), gout.stride(0), n_src, n_dst if fold_self else 0,
                                            _p(counts) if fold_self else 0, _nnz_ptr(counts), B, D, gh.data_ptr(), gh.stride(0),
                                            _p(part), _stream()), "bliss_spmm_self_bwd")
    return gh


@spmm_self_t.register_fake
def _(t_indptr, t_edge, src, dst, indptr, w, gout, n_src, n_dst, counts, fold_self):
    return gout.new_empty((n_src, gout.shape[1]), dtype=torch.bfloat16)


def _spmm_self_setup(ctx, inputs, output):
    indptr, src, dst, w, h, h_self, n_dst, counts, t_indptr, t_edge = inputs
    ctx.need_w = _wants_grad(w)
    ctx.save_for_backward(indptr, src, dst, w, counts, t_indptr, t_edge, *((h,) if ctx.need_w else ()))
    ctx.n_src, ctx.n_dst, ctx.fold = h.shape[0], n_dst, h_self is None


def _spmm_self_backward(ctx, gout):
    indptr, src, dst, w, counts, t_indptr, t_edge = ctx.saved_tensors[:7]
    if ctx.needs_input_grad[5]:
        raise NotImplementedError("bliss::spmm_self: no gradient w.r.t. a distinct h_self (the pair form under training)")
    g = gout.contiguous()
    if g.dtype != torch.bfloat16:
        g = g.bfloat16()
    gh = gw = None
    if ctx.needs_input_grad[4] or not ctx.need_w:
        if t_indptr is None or t_edge is None:
            raise RuntimeError("bliss::spmm_self needs the block's by-source index (Block.transposed()) to differentiate w.r.t. h")
        gh = spmm_self_t(t_indptr, t_edge, src, dst, indptr, w, g, ctx.n_src, ctx.n_dst, counts, ctx.fold)
    if ctx.need_w:                                              # (a distinct h_self does not enter gw)
        gw = sddmm(src, dst, indptr, g, ctx.saved_tensors[7], None, counts, _lib.SDDMM_SELF, False)
    return (None, None, None, gw, gh, None, None, None, None, None)


spmm_self.register_autograd(_spmm_self_backward, setup_context=_spmm_self_setup)


@torch.library.custom_op("bliss::lstm_agg", mutates_args=())
def lstm_agg(indptr: Tensor, src: Tensor, w: Optional[Tensor], p: Tensor, w_hh: Tensor, b_ih: Optional[Tensor], b_hh: Optional[Tensor],
             n_dst: int, counts: Optional[Tensor], save: bool, t_indptr: Optional[Tensor],
             t_edge: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """out[i] = the last hidden state of an LSTM cell run over row i's in-edges in row order, its input projection handed over
    as ``p = bf16(h @ W_ih^T)`` [n_src, 4 D] and scaled per edge by ``w`` (csrc/lstm.hip).  Returns (out bf16
    [n_dst, D], gates fp32 [B, 4 D], cell fp32 [B, D], hprev bf16 [B, D]); the last three are the backward's state, empty unless
    ``save``.  Rows without live in-edges, and rows past a padded block's live destination count, are +0."""
    assert p.is_cuda and p.dtype == torch.bfloat16 and p.dim() == 2 and p.stride(1) == 1, "bf16 projections on the GPU"
    assert w_hh.is_cuda and w_hh.dtype == torch.bfloat16 and w_hh.dim() == 2 and w_hh.stride(1) == 1
    D, B = w_hh.shape[1], int(src.numel())
    assert w_hh.shape[0] == 4 * D and p.shape[1] == 4 * D and 1 <= D <= _lib.LSTM_MAX_DIM
    for b in (b_ih, b_hh):
        assert b is None or (b.is_cuda and b.dtype == torch.bfloat16 and b.numel() == 4 * D and b.is_contiguous())
    dev = p.device
    out = torch.empty(n_dst, D, dtype=torch.bfloat16, device=dev)
    Bs = B if save else 0
    gates = torch.empty(Bs, 4 * D, dtype=torch.float32, device=dev)
    cell = torch.empty(Bs, D, dtype=torch.float32, device=dev)
    hprev = torch.empty(Bs, D, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib.bliss_lstm_agg_fwd(indptr.data_ptr(), src.data_ptr(), _p(w), p.data_ptr(), _rs(p), w_hh.data_ptr(),
                                           _rs(w_hh), _p(b_ih), _p(b_hh), n_dst, _p(counts), _nnz_ptr(counts), B, D, out.data_ptr(),
                                           _rs(out), gates.data_ptr(), cell.data_ptr(), hprev.data_ptr(), _stream()),
               "bliss_lstm_agg_fwd")
    return out, gates, cell, hprev


@lstm_agg.register_fake
def _(indptr, src, w, p, w_hh, b_ih, b_hh, n_dst, counts, save, t_indptr, t_edge):
    D, Bs = w_hh.shape[1], (src.numel() if save else 0)
    return (p.new_empty((n_dst, D), dtype=torch.bfloat16), p.new_empty((Bs, 4 * D), dtype=torch.float32),
            p.new_empty((Bs, D), dtype=torch.float32), p.new_empty((Bs, D), dtype=torch.bfloat16))


@torch.library.custom_op("bliss::lstm_agg_t", mutates_args=())
def lstm_agg_t(indptr: Tensor, t_indptr: Optional[Tensor], t_edge: Optional[Tensor], w: Optional[Tensor], gout: Tensor, w_hh: Tensor,
               gates: Tensor, cell: Tensor, n_src: int, counts: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """The backward of lstm_agg: dgate bf16 [B, 4 D], the gradient at the gate pre-activations of every live edge (+0 past them),
    and -- with the by-source index -- dp[s] = sum_{e : src_e = s} w_e dgate[e], bf16 [n_src, 4 D] (else empty)."""
    D, B, n_dst = w_hh.shape[1], gates.shape[0], gout.shape[0]
    dev = gout.device
    dgate = torch.empty(B, 4 * D, dtype=torch.bfloat16, device=dev)
    wt = w_hh.t().contiguous()                                  # [D, 4 D]: the product's B operand, K-contiguous
    _lib.check(_lib.lib.bliss_lstm_agg_bwd(indptr.data_ptr(), gout.data_ptr(), _rs(gout), wt.data_ptr(), _rs(wt),
                                           gates.data_ptr(), cell.data_ptr(), n_dst, _p(counts), _nnz_ptr(counts), B, D,
                                           dgate.data_ptr(), _stream()), "bliss_lstm_agg_bwd")
    if t_indptr is None or t_edge is None:
        return dgate, torch.empty(0, 4 * D, dtype=torch.bfloat16, device=dev)
    dp = torch.empty(n_src, 4 * D, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib.bliss_lstm_edge_reduce(t_indptr.data_ptr(), t_edge.data_ptr(), _p(w), dgate.data_ptr(), n_src, _nnz_ptr(counts),
                                               B, D, dp.data_ptr(), _rs(dp), _stream()), "bliss_lstm_edge_reduce")
    return dgate, dp


@lstm_agg_t.register_fake
def _(indptr, t_indptr, t_edge, w, gout, w_hh, gates, cell, n_src, counts):
    D = w_hh.shape[1]
    return (gout.new_empty((gates.shape[0], 4 * D), dtype=torch.bfloat16),
            gout.new_empty((n_src if t_indptr is not None and t_edge is not None else 0, 4 * D), dtype=torch.bfloat16))


def _lstm_setup(ctx, inputs, output):
    indptr, src, w, p, w_hh, b_ih, b_hh, n_dst, counts, save, t_indptr, t_edge = inputs
    ctx.need_w = _wants_grad(w)
    ctx.save_for_backward(indptr, src, w, w_hh, counts, t_indptr, t_edge, output[1], output[2], output[3], *((p,) if ctx.need_w else ()))
    ctx.n_src, ctx.saved_state = p.shape[0], save
    ctx.mark_non_differentiable(output[1], output[2], output[3])
    ctx.set_materialize_grads(False)


def _lstm_backward(ctx, gout, _g1, _g2, _g3):
    indptr, src, w, w_hh, counts, t_indptr, t_edge, gates, cell, hprev = ctx.saved_tensors[:10]
    if gout is None:
        return (None,) * 12
    if not ctx.saved_state:
        raise RuntimeError("bliss::lstm_agg was run with save=False: the backward's state was not kept")
    need_p = ctx.needs_input_grad[3]
    if need_p and (t_indptr is None or t_edge is None):
        raise RuntimeError("bliss::lstm_agg needs the block's by-source index (Block.transposed()) to differentiate w.r.t. p")
    g = gout.contiguous()
    if g.dtype != torch.bfloat16:
        g = g.bfloat16()
    dgate, dp = lstm_agg_t(indptr, t_indptr if need_p else None, t_edge if need_p else None, w, g, w_hh, gates, cell, ctx.n_src, counts)
    gw = g_hh = gb_ih = gb_hh = None
    if ctx.need_w:                                              # gw_e = dgate[e] . p[src_e]: the per-edge dot with the edge as its own row
        rows = torch.arange(src.numel(), dtype=torch.int32, device=src.device)
        gw = sddmm(src, rows, None, dgate, ctx.saved_tensors[10], None, counts, _lib.SDDMM_SUM, False)
    if ctx.needs_input_grad[4]:
        g_hh = dgate.t() @ hprev                                # [4 D, B] x [B, D]: zeros past the live edges on both sides
    if ctx.needs_input_grad[5] or ctx.needs_input_grad[6]:
        from .nn import _bias_grad
        gb = _bias_grad(dgate)
        gb_ih = gb if ctx.needs_input_grad[5] else None
        gb_hh = gb if ctx.needs_input_grad[6] else None
    return (None, None, gw, dp if need_p else None, g_hh, gb_ih, gb_hh, None, None, None, None, None)


lstm_agg.register_autograd(_lstm_backward, setup_context=_lstm_setup)


@torch.library.custom_op("bliss::embed_norm", mutates_args=())
def embed_norm(h: Tensor) -> Tensor:
    """bf16 [K]: ||h_j||_2 per row (model.py:318-320)."""
    assert h.is_cuda and h.dtype == torch.bfloat16 and h.stride(1) == 1
    out = torch.empty(h.shape[0], dtype=torch.bfloat16, device=h.device)
    _lib.check(_lib.lib.bliss_embed_norm(h.data_ptr(), h.shape[0], h.shape[1], h.stride(0), out.data_ptr(), _stream()), "bliss_embed_norm")
    return out


@embed_norm.register_fake
def _(h):
    return h.new_empty((h.shape[0],), dtype=torch.bfloat16)
