"""Message-passing layers over bliss Blocks: the ``dglnn.SAGEConv`` the reference instantiates
(model.py:303-308) with its g-SpMM replaced by the gfx950 kernels of csrc/spmm.hip.

[DGL-recalled] dglnn.SAGEConv(in, out, 'mean'):  rst = fc_self(h[:S]) + fc_neigh o mean_w(h);
fc_neigh (bias-free) is applied BEFORE aggregation iff in > out; fc_self carries the bias; both
weights xavier-uniform with gain('relu').  The dense transforms are plain library GEMMs (hipBLASLt
through torch.nn.functional.linear); the aggregation and its backward are ours.
'pool' (max-reduce, csrc/spmm_max.hip), 'gcn' (the self-inclusive normalised sum of csrc/spmm_self.hip: no fc_self, a
plain bias) and 'lstm' (a recurrent cell over each destination's in-edges, csrc/lstm.hip) are the other aggregators built:
DESIGN.md sections 30, 34 and 37.
"""
import torch
import torch.nn as nn

from . import _lib
from ._engine import _stream, spmm_partials


def embed_norm(h):
    """``th.reshape(th.norm(h, dim=1, keepdim=True), (-1,))`` of model.py:318-320 -> bf16 [K]  (``torch.ops.bliss.embed_norm``)."""
    from . import ops
    h = h.detach()
    if h.dtype != torch.bfloat16:
        h = h.bfloat16()
    if h.stride(1) != 1:
        h = h.contiguous()
    return ops.embed_norm(h)


def _wait_block(block):
    # A block whose build was left to another stream (train.PipelinedTrainStep: the input layer's block is built beside the
    # first transform of the forward pass): its first consumer waits for the builder's flag.  Set during graph capture only.
    r = getattr(block, "_ready", None)
    if r is not None:
        _lib.check(_lib.lib.bliss_flag_wait(r[0], r[1], _stream()), "bliss_flag_wait")
        block._ready = None


def _aggregate_operands(block, h, edge_weight):
    """What weighted_aggregate and max_aggregate hand to their op: h with unit column stride, w bf16 contiguous or None (the cast
    is autograd's, so an fp32 leaf gets its gradient through it), the device-side counts of a capacity-padded block, and the
    by-source index when a gradient w.r.t. h is needed (else None, None)."""
    assert h.is_cuda and h.dtype == torch.bfloat16, "bf16 features on the GPU (load_graph.py:7)"
    _wait_block(block)
    if h.stride(1) != 1:
        h = h.contiguous()
    w = None
    if edge_weight is not None:
        w = edge_weight.reshape(-1)
        if w.dtype != torch.bfloat16:
            w = w.bfloat16()
        w = w.contiguous()
        assert w.numel() == block.num_edges()
    counts = getattr(block, "_counts_dev", None) if block._nnz_ptr else None
    need_t = h.requires_grad and torch.is_grad_enabled()
    t_indptr, t_edge = block.transposed() if need_t else (None, None)
    return h, w, counts, t_indptr, t_edge


def weighted_aggregate(block, h, edge_weight=None, mean=True, out_fp32=False):
    """out[i] = (1/deg_i if mean) * sum_{e -> i} w_e h[src_e] over a Block -- ``torch.ops.bliss.spmm`` (bliss_gnn_amd/ops.py: a
    torch.library custom op with a fake kernel and the transposed SpMM as its autograd formula).  Edge weights that require a
    gradient get gw_e = (1/deg_{dst_e} if mean) * d out[dst_e] . h[src_e] from ``torch.ops.bliss.sddmm``."""
    from . import ops
    h, w, counts, t_indptr, t_edge = _aggregate_operands(block, h, edge_weight)
    return ops.spmm(block.indptr, block.src, block.dst, w, h, block.num_dst_nodes(), counts, bool(mean), bool(out_fp32), t_indptr, t_edge)


def max_aggregate(block, h, edge_weight=None, return_arg=False):
    """out[i, c] = max_{e -> i} bf16(w_e h[src_e, c]) over a Block, 0 for a row without edges -- ``torch.ops.bliss.spmm_max``
    (csrc/spmm_max.hip, DESIGN.md section 30: DGL's ``update_all(u_mul_e | copy_u, fn.max)``, the lowest edge wins a tie);
    the gradient w.r.t. h is routed to the recorded edge of every element, and edge weights that require a gradient get the
    dot product of d out and h over the columns their edge won.  ``return_arg=True`` also returns arg
    int32 [S, dim] (the winning edge, -1 for a row without edges)."""
    from . import ops
    h, w, counts, t_indptr, t_edge = _aggregate_operands(block, h, edge_weight)
    w_grad = w is not None and w.requires_grad and torch.is_grad_enabled()
    out, arg = ops.spmm_max(block.indptr, block.src, block.dst, w, h, block.num_dst_nodes(), counts,
                            bool(return_arg or t_indptr is not None or w_grad), t_indptr, t_edge)
    return (out, arg) if return_arg else out


def gcn_aggregate(block, h, edge_weight=None, h_self=None):
    """out[i] = (sum_{e -> i} w_e h[src_e] + h_self[i]) / (deg_i + 1) over a Block, ONE rounding -- ``torch.ops.bliss.spmm_self``
    (csrc/spmm_self.hip, DESIGN.md section 34: the 'gcn' aggregator of dglnn.SAGEConv [DGL-recalled]).  ``h_self=None``: the
    destinations are the leading rows of ``h``, and the gradient w.r.t. h carries the self term on those rows.  Edge weights that
    require a gradient get gw_e = d out[dst_e] . h[src_e] / (deg_{dst_e} + 1).  A distinct
    ``h_self`` (the (feat_src, feat_dst) pair form) is forward-only: one that requires a gradient is refused."""
    from . import ops
    if h_self is h:
        h_self = None
    if h_self is not None:
        assert h_self.is_cuda and h_self.dtype == torch.bfloat16, "bf16 features on the GPU (load_graph.py:7)"
        if h_self.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("gcn_aggregate: a distinct h_self that requires a gradient (the (feat_src, feat_dst) pair form under "
                                      "training) is not built: DESIGN.md section 34")
        if h_self.stride(1) != 1:
            h_self = h_self.contiguous()
        if h_self.shape[0] < block.num_dst_nodes() or h_self.shape[1] != h.shape[1]:
            raise ValueError("gcn_aggregate: h_self is [num_dst_nodes, dim] like h")
    elif h.shape[0] < block.num_dst_nodes():
        raise ValueError("gcn_aggregate: the destinations are the leading rows of h; pass h_self for any other block")
    h, w, counts, t_indptr, t_edge = _aggregate_operands(block, h, edge_weight)
    return ops.spmm_self(block.indptr, block.src, block.dst, w, h, h_self, block.num_dst_nodes(), counts, t_indptr, t_edge)


LSTM_MAX_DIM = _lib.LSTM_MAX_DIM            # the widest hidden state of csrc/lstm.hip's tile


def lstm_refusal(lstm, h=None, what="lstm_aggregate"):
    """Why the recurrent aggregation cannot take this nn.LSTM (and these features), or None."""
    if not isinstance(lstm, nn.LSTM) or lstm.num_layers != 1 or lstm.bidirectional or lstm.proj_size != 0 or lstm.input_size != lstm.hidden_size:
        return "%s takes a one-layer, one-direction nn.LSTM(D, D) without a projection" % what
    if lstm.hidden_size > LSTM_MAX_DIM:
        return "%s: in_feats <= %d (the tile of csrc/lstm.hip, DESIGN.md section 37), not %d" % (what, LSTM_MAX_DIM, lstm.hidden_size)
    bad = [q for q in list(lstm.parameters()) + ([] if h is None else [h]) if not (q.is_cuda and q.dtype == torch.bfloat16)]
    if bad:
        return ("%s takes bf16 features and LSTM parameters on the GPU, not %s on %s: there is no other path"
                % (what, bad[0].dtype, bad[0].device))
    if h is not None and (h.dim() != 2 or h.shape[1] != lstm.hidden_size):
        return "%s: features [n_src, %d] for this LSTM, not %r" % (what, lstm.hidden_size, tuple(h.shape))
    return None


def lstm_aggregate(block, h, lstm, edge_weight=None):
    """out[i] = the last hidden state of ``lstm`` (an nn.LSTM(D, D)) run over w_e h[src_e] for the in-edges e of i in the block's row
    order from h = c = 0, +0 for a row without in-edges -- ``torch.ops.bliss.lstm_agg`` (csrc/lstm.hip, DESIGN.md section 37: the
    'lstm' aggregator of dglnn.SAGEConv [DGL-recalled]).  The input projection runs once per source row as a library GEMM,
    P = h @ W_ih^T, rounded to bf16; the recurrence takes P.  Differentiates w.r.t. h, the four LSTM parameters and, when they
    require it, the edge weights (gw_e = dgate[e] . P[src_e]).  Raises NotImplementedError, before any launch, for anything but
    bf16 on the GPU and D <= 256."""
    from . import ops
    why = lstm_refusal(lstm, h)
    if why is not None:
        raise NotImplementedError(why)
    h, w, counts, t_indptr, t_edge = _aggregate_operands(block, h, edge_weight)
    p = torch.nn.functional.linear(h, lstm.weight_ih_l0)        # [n_src, 4 D]; its autograd gives d h and d W_ih from d P
    grad = torch.is_grad_enabled()
    if grad and p.requires_grad and t_indptr is None:           # (h itself may need nothing: the input layer's W_ih still does)
        t_indptr, t_edge = block.transposed()
    b_ih, b_hh = (lstm.bias_ih_l0, lstm.bias_hh_l0) if lstm.bias else (None, None)
    save = grad and any(q is not None and q.requires_grad for q in (p, w, lstm.weight_hh_l0, b_ih, b_hh))
    return ops.lstm_agg(block.indptr, block.src, w, p, lstm.weight_hh_l0, b_ih, b_hh, block.num_dst_nodes(), counts, save,
                        t_indptr, t_edge)[0]


class _SageEpilogue(torch.autograd.Function):
    """out = dropout_p(relu(a + b)), norm = ||out||_2 per row in one kernel (csrc/spmm.hip: k_sage_epilogue)."""

    @staticmethod
    def forward(ctx, a, b, p, ctr, seed):
        ctx.set_materialize_grads(False)          # (no zero-filled gradients for the outputs nothing differentiates through)
        a, b = a.contiguous(), b.contiguous()
        n, d = a.shape
        out = torch.empty_like(a)
        norm = torch.empty(n, dtype=torch.bfloat16, device=a.device)
        _lib.check(_lib.lib.bliss_sage_epilogue_fwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), n, d, float(p), int(seed),
                                                    0 if ctr is None else ctr.data_ptr(), out.data_ptr(), out.stride(0),
                                                    norm.data_ptr(), _stream()), "bliss_sage_epilogue_fwd")
        ctx.save_for_backward(out)
        ctx.p = float(p)
        ctx.mark_non_differentiable(norm)
        return out, norm

    @staticmethod
    def backward(ctx, dout, _dnorm):
        (out,) = ctx.saved_tensors
        if dout is None:
            return None, None, None, None, None
        dout = dout.contiguous()
        if dout.dtype != torch.bfloat16:
            dout = dout.bfloat16()
        din = torch.empty_like(out)
        _lib.check(_lib.lib.bliss_sage_epilogue_bwd(dout.data_ptr(), dout.stride(0), out.data_ptr(), out.stride(0), out.shape[0],
                                                    out.shape[1], ctx.p, din.data_ptr(), din.stride(0), _stream()),
                   "bliss_sage_epilogue_bwd")
        return din, din, None, None, None


def sage_epilogue(self_out, neigh, p, ctr, seed):
    """The tail of a hidden SAGE layer (model.py:321-333) and the row norms the next layer stores (:318-320)."""
    return _SageEpilogue.apply(self_out, neigh, p, ctr, seed)


# ------------------------------------------------------------------------------------------------ loss (csrc/loss.hip)
_row_ids = {}


def _identity_ids(n, device):
    """int32 [n] = 0 .. n-1: the label ids of a live launch whose labels are gathered already (the live entry points take
    bliss_cross_entropy_sum's arguments, which name the labels through ids); built once per size and device."""
    key = (int(n), str(device))
    if key not in _row_ids:
        _row_ids[key] = torch.arange(int(n), dtype=torch.int32, device=device)
    return _row_ids[key]


def _live_word(n_rows_dev, device):
    """The live row count of a capacity-padded batch as the kernels take it: one int32 word on ``device``."""
    if not (torch.is_tensor(n_rows_dev) and n_rows_dev.dtype == torch.int32 and n_rows_dev.numel() == 1 and n_rows_dev.device == device):
        raise ValueError("n_rows_dev: one int32 word on the logits' device")
    return n_rows_dev


def _live_kw(n_rows_dev):
    """The launch helpers' keyword for a live row count; nothing without one: their calls are then the ones they were."""
    return {} if n_rows_dev is None else {"n_rows_dev": n_rows_dev}


_NO_LIVE = ("a live row count (n_rows_dev) needs the one-launch loss kernel -- bf16 logits [rows, classes] on the GPU with unit "
            "column stride and labels on the same device; there is no masked form of torch's functional loss here")


class _CrossEntropy(torch.autograd.Function):
    """nn.CrossEntropyLoss() (mean) on bf16 logits, forward and gradient in one launch (train_lightning.py:77-79, :142)."""

    @staticmethod
    def forward(ctx, logits, labels, state, n_rows_dev=None):
        x = logits if logits.stride(1) == 1 else logits.contiguous()
        if n_rows_dev is not None:
            loss, dx = _ce_launch(x, labels, state, n_rows_dev=n_rows_dev)
            ctx.save_for_backward(dx)
            return loss.to(logits.dtype)
        n, c = x.shape
        dx = torch.empty(n, c, dtype=torch.bfloat16, device=x.device)
        rows = torch.empty(n, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib.bliss_cross_entropy(x.data_ptr(), x.stride(0), labels.data_ptr(), n, c, rows.data_ptr(), dx.data_ptr(), dx.stride(0),
                                                loss.data_ptr(), state.data_ptr(), state.data_ptr() + 4, _stream()), "bliss_cross_entropy")
        ctx.save_for_backward(dx)
        return loss.to(logits.dtype)

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g.to(dx.dtype), None, None, None


def _ce_launch(x, labels, state, x2=None, label_ids=None, n_rows_dev=None):
    n, c = x.shape
    dx = torch.empty(n, c, dtype=torch.bfloat16, device=x.device)
    rows = torch.empty(n, dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    if n_rows_dev is not None:                  # n is the capacity; the divisor is the device's count (bliss_cross_entropy_live)
        if x2 is None and label_ids is None:
            label_ids = _identity_ids(n, x.device)
        _lib.check(_lib.lib.bliss_cross_entropy_live(x.data_ptr(), x.stride(0), 0 if x2 is None else x2.data_ptr(),
                                                     0 if x2 is None else x2.stride(0), labels.data_ptr(),
                                                     0 if label_ids is None else label_ids.data_ptr(), n, n_rows_dev.data_ptr(), c,
                                                     rows.data_ptr(), dx.data_ptr(), dx.stride(0), loss.data_ptr(), state.data_ptr(),
                                                     state.data_ptr() + 4, _stream()), "bliss_cross_entropy_live")
    elif x2 is None and label_ids is None:
        _lib.check(_lib.lib.bliss_cross_entropy(x.data_ptr(), x.stride(0), labels.data_ptr(), n, c, rows.data_ptr(), dx.data_ptr(),
                                                dx.stride(0), loss.data_ptr(), state.data_ptr(), state.data_ptr() + 4, _stream()),
                   "bliss_cross_entropy")
    else:
        _lib.check(_lib.lib.bliss_cross_entropy_sum(x.data_ptr(), x.stride(0), 0 if x2 is None else x2.data_ptr(),
                                                    0 if x2 is None else x2.stride(0), labels.data_ptr(),
                                                    0 if label_ids is None else label_ids.data_ptr(), n, c, rows.data_ptr(), dx.data_ptr(),
                                                    dx.stride(0), loss.data_ptr(), state.data_ptr(), state.data_ptr() + 4, _stream()),
                   "bliss_cross_entropy_sum")
    return loss, dx


def _check_loss_errors(module, name):
    """Read the loss kernel's error word, clear it, and raise if it was set (one tiny read-back: call it where the loop
    synchronises anyway)."""
    st = getattr(module, "_state", None)
    if st is None:
        return
    word = int(st[1].item())
    if word:
        st[1] = 0
        raise RuntimeError("%s: the loss kernel met labels out of range -- a class index outside [0, n_classes) or a label id "
                           "outside the label table (error 0x%x, %s); the rows concerned counted for nothing"
                           % (name, word, _lib.err_string(word)))


class CrossEntropyLoss(nn.Module):
    """``nn.CrossEntropyLoss()`` as the reference builds it (train_lightning.py:77-79): mean over the batch, class-index
    targets.  bf16 logits on the GPU take the one-launch kernel; anything else goes to torch's functional form.

    ``n_rows_dev`` (``forward``, ``backward_from``, ``backward_from_parts``): the logits are a capacity-padded batch and only the
    first ``n_rows_dev[0]`` rows (an int32 word on the device) are live -- the mean is over those, the other rows get a zero
    gradient and nothing of them is read (csrc/loss.hip: bliss_cross_entropy_live).  Kernel path only: anything else raises."""

    def forward(self, logits, target, n_rows_dev=None):
        if logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and target.dtype == torch.int64 and target.dim() == 1:
            if getattr(self, "_state", None) is None or self._state.device != logits.device:
                self._state = torch.zeros(2, dtype=torch.int32, device=logits.device)       # [0] ticket, [1] error word
            if n_rows_dev is not None:
                if target.device != logits.device or target.shape[0] != logits.shape[0]:
                    raise NotImplementedError(_NO_LIVE)
                return _CrossEntropy.apply(logits, target.contiguous(), self._state, _live_word(n_rows_dev, logits.device))
            return _CrossEntropy.apply(logits, target.contiguous(), self._state)
        if n_rows_dev is not None:
            raise NotImplementedError(_NO_LIVE)
        return torch.nn.functional.cross_entropy(logits, target)

    def _eligible(self, logits, target):
        return logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and target.dtype == torch.int64 and target.dim() == 1

    def check_errors(self):
        """torch raises a device assert on a class index outside [0, n_classes); the kernel sets a word instead (the row gets no
        loss and no one-hot).  This reads the word, clears it and raises."""
        _check_loss_errors(self, "CrossEntropyLoss")

    def backward_from(self, logits, target, n_rows_dev=None):
        """loss.backward() without the loss node: the kernel produces d loss / d logits with the loss, so the train loops call
        ``logits.backward(that)`` directly (saves the ones-fill, the scalar cast and the elementwise product of the generic
        route).  Returns the loss (fp32 scalar, detached)."""
        if not self._eligible(logits, target):
            if n_rows_dev is not None:
                raise NotImplementedError(_NO_LIVE)
            loss = self.forward(logits, target)
            loss.backward()
            return loss.detach()
        if getattr(self, "_state", None) is None or self._state.device != logits.device:
            self._state = torch.zeros(2, dtype=torch.int32, device=logits.device)
        x = logits.detach()
        if n_rows_dev is not None:
            if target.device != logits.device or target.shape[0] != logits.shape[0]:
                raise NotImplementedError(_NO_LIVE)
            n_rows_dev = _live_word(n_rows_dev, logits.device)
        loss, dx = _ce_launch(x if x.stride(1) == 1 else x.contiguous(), target.contiguous(), self._state, **_live_kw(n_rows_dev))
        logits.backward(dx)
        return loss

    def backward_from_parts(self, a, b, label_table, label_ids, n_rows_dev=None):
        """backward_from for logits = a + b that are never formed (the output layer's fc_self + h_neigh) and labels
        = label_table[label_ids] that are never gathered: one launch, then the same gradient into both addends."""
        ok = (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape and a.dim() == 2
              and a.stride(1) == 1 and b.stride(1) == 1 and label_table.dtype == torch.int64 and label_table.dim() == 1
              and label_table.is_contiguous() and label_ids.dtype == torch.int32 and label_ids.is_contiguous()
              and label_ids.numel() == a.shape[0])
        if not ok:
            return self.backward_from(a + b, torch.index_select(label_table, 0, label_ids.long()), n_rows_dev)
        if getattr(self, "_state", None) is None or self._state.device != a.device:
            self._state = torch.zeros(2, dtype=torch.int32, device=a.device)
        if n_rows_dev is not None:
            n_rows_dev = _live_word(n_rows_dev, a.device)
        loss, dx = _ce_launch(a.detach(), label_table, self._state, x2=b.detach(), label_ids=label_ids, **_live_kw(n_rows_dev))
        torch.autograd.backward([a, b], [dx, dx])
        return loss


class _BCEWithLogits(torch.autograd.Function):
    """nn.BCEWithLogitsLoss() (mean) on bf16 logits and fp32 targets, forward and gradient in one launch (train_lightning.py:77-79)."""

    @staticmethod
    def forward(ctx, logits, target, state, n_rows_dev=None):
        loss, dx = _bce_launch(logits, target, state, **_live_kw(n_rows_dev))
        ctx.save_for_backward(dx)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g.to(dx.dtype), None, None, None


def _bce_launch(x, targets, state, x2=None, label_ids=None, n_rows_dev=None):
    n, c = x.shape
    dx = torch.empty(n, c, dtype=torch.bfloat16, device=x.device)
    rows = torch.empty(n, dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    if n_rows_dev is not None:                  # n is the capacity; the divisor is the device's count (bliss_bce_logits_live)
        if x2 is None and label_ids is None:
            label_ids = _identity_ids(n, x.device)
        _lib.check(_lib.lib.bliss_bce_logits_live(x.data_ptr(), x.stride(0), 0 if x2 is None else x2.data_ptr(),
                                                  0 if x2 is None else x2.stride(0), targets.data_ptr(),
                                                  0 if label_ids is None else label_ids.data_ptr(), n, n_rows_dev.data_ptr(), c,
                                                  rows.data_ptr(), dx.data_ptr(), dx.stride(0), loss.data_ptr(), state.data_ptr(),
                                                  state.data_ptr() + 4, _stream()), "bliss_bce_logits_live")
    elif x2 is None and label_ids is None:
        _lib.check(_lib.lib.bliss_bce_logits(x.data_ptr(), x.stride(0), targets.data_ptr(), n, c, rows.data_ptr(), dx.data_ptr(),
                                             dx.stride(0), loss.data_ptr(), state.data_ptr(), state.data_ptr() + 4, _stream()),
                   "bliss_bce_logits")
    else:
        _lib.check(_lib.lib.bliss_bce_logits_sum(x.data_ptr(), x.stride(0), 0 if x2 is None else x2.data_ptr(),
                                                 0 if x2 is None else x2.stride(0), targets.data_ptr(),
                                                 0 if label_ids is None else label_ids.data_ptr(), n, c, rows.data_ptr(), dx.data_ptr(),
                                                 dx.stride(0), loss.data_ptr(), state.data_ptr(), state.data_ptr() + 4, _stream()),
                   "bliss_bce_logits_sum")
    return loss, dx


class BCEWithLogitsLoss(nn.Module):
    """``nn.BCEWithLogitsLoss()`` as the reference builds it for the multi-label dataset (train_lightning.py:77-79): mean over
    all (row, class) pairs, no ``weight``, no ``pos_weight``.  bf16 logits on the GPU with fp32 targets take the one-launch
    kernel (csrc/loss.hip: k_bce_logits; the loss is an fp32 scalar, as torch's is for these dtypes); anything else goes to
    torch's functional form.  ``n_rows_dev``: a live row count, as ``CrossEntropyLoss`` takes it (bliss_bce_logits_live: the mean
    is over the live rows x classes); kernel path only."""

    def _eligible(self, logits, target):
        return (logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.stride(1) == 1 and logits.numel() > 0
                and target.dtype == torch.float32 and target.shape == logits.shape and target.is_contiguous()
                and target.device == logits.device and not target.requires_grad)

    def _state_on(self, device):
        if getattr(self, "_state", None) is None or self._state.device != device:
            self._state = torch.zeros(2, dtype=torch.int32, device=device)                 # [0] ticket, [1] error word
        return self._state

    def check_errors(self):
        """A label id outside the target table (backward_from_parts) sets a word; this reads it, clears it and raises."""
        _check_loss_errors(self, "BCEWithLogitsLoss")

    def forward(self, logits, target, n_rows_dev=None):
        if self._eligible(logits, target):
            if n_rows_dev is not None:
                return _BCEWithLogits.apply(logits, target, self._state_on(logits.device), _live_word(n_rows_dev, logits.device))
            return _BCEWithLogits.apply(logits, target, self._state_on(logits.device))
        if n_rows_dev is not None:
            raise NotImplementedError(_NO_LIVE)
        return torch.nn.functional.binary_cross_entropy_with_logits(logits, target)

    def backward_from(self, logits, target, n_rows_dev=None):
        """loss.backward() without the loss node (see CrossEntropyLoss.backward_from).  Returns the loss (fp32 scalar, detached)."""
        if not self._eligible(logits, target):
            if n_rows_dev is not None:
                raise NotImplementedError(_NO_LIVE)
            loss = self.forward(logits, target)
            loss.backward()
            return loss.detach()
        if n_rows_dev is not None:
            n_rows_dev = _live_word(n_rows_dev, logits.device)
        loss, dx = _bce_launch(logits.detach(), target, self._state_on(logits.device), **_live_kw(n_rows_dev))
        logits.backward(dx)
        return loss

    def backward_from_parts(self, a, b, label_table, label_ids, n_rows_dev=None):
        """backward_from for logits = a + b that are never formed (the output layer's fc_self + h_neigh) and targets
        = label_table[label_ids] ([V, n_cls] fp32) that are never gathered: one launch, then the same gradient into both addends."""
        ok = (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape and a.dim() == 2
              and a.numel() > 0 and a.stride(1) == 1 and b.stride(1) == 1 and b.device == a.device
              and label_table.dtype == torch.float32 and label_table.dim() == 2 and label_table.shape[1] == a.shape[1]
              and label_table.is_contiguous() and label_table.device == a.device and not label_table.requires_grad
              and label_ids.dtype == torch.int32 and label_ids.is_contiguous() and label_ids.numel() == a.shape[0]
              and label_ids.device == a.device)
        if not ok:
            return self.backward_from(a + b, torch.index_select(label_table, 0, label_ids.long()), n_rows_dev)
        if n_rows_dev is not None:
            n_rows_dev = _live_word(n_rows_dev, a.device)
        loss, dx = _bce_launch(a.detach(), label_table, self._state_on(a.device), x2=b.detach(), label_ids=label_ids, **_live_kw(n_rows_dev))
        torch.autograd.backward([a, b], [dx, dx])
        return loss


# ------------------------------------------------------------------------------------------------ MFMA tile GEMM (csrc/sage.hip)
TILE_GEMM_MAX_K, TILE_GEMM_MAX_N = 1024, 256
# transforms="wide" (DESIGN.md section 29): a product whose reduction passes TILE_GEMM_MAX_K walks it in panels of that many
# columns (bliss_tile_gemm_wide, bliss_dgrad_wide); a product within it keeps the entry point, launches and bits it always had
TILE_WIDE_MAX_K = _lib.WIDE_MAX_K


class LazyRows:
    """``table[ids]`` not gathered yet: ``block.srcdata.lazy('features')``.  SAGE.forward hands it to the fused transform,
    whose A-operand load IS the gather (train_lightning.py:138 + model.py:318-329 in one launch)."""

    def __init__(self, table, ids, frame=None, key=None):
        self.table, self.ids, self._frame, self._key = table, ids, frame, key
        self.shape, self.dtype, self.device = (ids.numel(), table.shape[1]), table.dtype, table.device
        self.is_cuda = table.is_cuda

    def materialize(self):
        """The rows as a tensor: through the owning frame when there is one (its gather kernel also leaves the row norms the
        model asks for next, graph._LazyFrame), else a plain index_select."""
        if self._frame is not None:
            return self._frame[self._key]
        return torch.index_select(self.table, 0, self.ids)


def _tg_args(a1, w1, out, m_bound, ids=None, a2=None, w2=None, bias=None, m_dev=0, a_copy=None, in_norm=None, out_norm=None,
             relu=False, p=0.0, seed=0, ctr=None):
    import ctypes as C
    t = _lib.TileGemm()
    t.a1, t.a1_stride, t.ids = a1.data_ptr(), a1.stride(0), 0 if ids is None else ids.data_ptr()
    t.w1, t.w1_stride, t.k1 = w1.data_ptr(), w1.stride(0), w1.shape[1]
    if a2 is not None:
        t.a2, t.a2_stride, t.w2, t.w2_stride, t.k2 = a2.data_ptr(), a2.stride(0), w2.data_ptr(), w2.stride(0), w2.shape[1]
    t.bias = 0 if bias is None else bias.data_ptr()
    t.m_bound, t.m_dev, t.n = int(m_bound), int(m_dev), w1.shape[0]
    t.out, t.out_stride = out.data_ptr(), out.stride(0)
    if a_copy is not None:
        t.a_copy, t.copy_stride = a_copy.data_ptr(), a_copy.stride(0)
    t.in_norm = 0 if in_norm is None else in_norm.data_ptr()
    t.out_norm = 0 if out_norm is None else out_norm.data_ptr()
    t.relu, t.drop_p, t.drop_seed, t.drop_ctr = int(relu), float(p), int(seed) & 0xFFFFFFFF, 0 if ctr is None else ctr.data_ptr()
    return t


def _tile_gemm(first, second=None, wide=False):
    """One launch for one or two argument sets.  ``wide``: a launch with a reduction past TILE_GEMM_MAX_K goes to the K-panelled
    entry point; every other launch is bliss_tile_gemm's, wide or not."""
    import ctypes as C
    sets = [first] + ([] if second is None else [second])
    if wide and any(max(t.k1, t.k2) > TILE_GEMM_MAX_K for t in sets):
        _lib.check(_lib.lib.bliss_tile_gemm_wide(C.byref(first), None if second is None else C.byref(second), _stream()), "bliss_tile_gemm_wide")
        return
    _lib.check(_lib.lib.bliss_tile_gemm(C.byref(first), None if second is None else C.byref(second), _stream()), "bliss_tile_gemm")


def _bf16c(t):
    t = t if t.dtype == torch.bfloat16 else t.bfloat16()
    return t if t.stride(-1) == 1 else t.contiguous()



# ------------------------------------------------------------------------------------------------ backward products (csrc/sage_bwd.hip)
def _mfma_bwd_on():
    """The hand-written MFMA backward (round 3).  BLISS_SAGE_MFMA_BWD=0 restores the library GEMMs of round 2."""
    import os
    return os.environ.get("BLISS_SAGE_MFMA_BWD", "1") != "0"


def _bwd_ok(*mats):
    return all(m is None or (m.is_cuda and m.dtype == torch.bfloat16 and m.dim() == 2 and m.stride(1) == 1) for m in mats)


def sage_dgrad(a1, w1, m_bound, m_dev=0, a2=None, w2=None, m2_bound=0, m2_dev=0):
    """out[r] = a1[r] @ w1 (+ a2[r] @ w2 for r < m2): the gradient w.r.t. a layer's input rows; w = nn.Linear weights [out, in]."""
    import ctypes as C
    out = torch.empty(m_bound, w1.shape[1], dtype=torch.bfloat16, device=a1.device)
    t = _lib.DGrad()
    t.a1, t.a1_stride, t.w1, t.w1_stride, t.k1 = a1.data_ptr(), a1.stride(0), w1.data_ptr(), w1.stride(0), w1.shape[0]
    if a2 is not None:
        t.a2, t.a2_stride, t.w2, t.w2_stride, t.k2 = a2.data_ptr(), a2.stride(0), w2.data_ptr(), w2.stride(0), w2.shape[0]
        t.m2_bound, t.m2_dev = int(m2_bound), int(m2_dev)
    t.m_bound, t.m_dev, t.n = int(m_bound), int(m_dev), w1.shape[1]
    t.out, t.out_stride = out.data_ptr(), out.stride(0)
    _lib.check(_lib.lib.bliss_sage_dgrad(C.byref(t), _stream()), "bliss_sage_dgrad")
    return out


def sage_wgrad(problems):
    """[(d [R, n_out], x [R, k_in], rows_bound, rows_dev, want_bias)] (one or two) -> [(dW [n_out, k_in], db or None)]: the weight
    (and bias) gradients of Linear layers, dW = d^T x over the block's rows, one launch pair for all of them."""
    import ctypes as C
    n = len(problems)
    arr = (_lib.WGrad * n)()
    outs = []
    for i, (d, x, rb, rdev, want_b) in enumerate(problems):
        dw = torch.empty(d.shape[1], x.shape[1], dtype=torch.bfloat16, device=d.device)
        db = torch.empty(d.shape[1], dtype=torch.bfloat16, device=d.device) if want_b else None
        a = arr[i]
        a.d, a.d_stride, a.n_out = d.data_ptr(), d.stride(0), d.shape[1]
        a.x, a.x_stride, a.k_in = x.data_ptr(), x.stride(0), x.shape[1]
        a.rows_bound, a.rows_dev = int(rb), int(rdev)
        a.dw, a.dw_stride, a.db = dw.data_ptr(), dw.stride(0), 0 if db is None else db.data_ptr()
        outs.append((dw, db))
    need = int(_lib.lib.bliss_sage_wgrad_workspace(arr, n))
    if need < 0:
        raise RuntimeError("bliss_sage_wgrad: invalid problem description")
    # fp32 partial tiles: a scratch tensor of the caching allocator (inside a captured graph: of the graph's pool); the
    # reduce kernel behind the product reads what the product wrote, in stream order, so nothing outlives the call
    ws = torch.empty(max(need, 4), dtype=torch.float32, device=problems[0][0].device)
    _lib.check(_lib.lib.bliss_sage_wgrad(arr, n, ws.data_ptr(), ws.numel(), _stream()), "bliss_sage_wgrad")
    return outs


class _SageLinearPair(torch.autograd.Function):
    """fc_neigh over all source rows and fc_self (+bias) over the destination rows of a W-first SAGEConv layer (in > out,
    [DGL-recalled] SURVEY.md m2/m4) in ONE launch; with ``ids`` the rows are gathered from ``x`` (a node-feature table) on
    the fly.  Returns (Z [K, out], Y [S, out], the input rows [K, in], their bf16 norms [K])."""

    @staticmethod
    def forward(ctx, x, ids, w_neigh, w_self, b_self, n_src, n_dst, src_dev, dst_dev, wide=False):
        ctx.set_materialize_grads(False)          # (else autograd zero-fills a gradient for `rows`: 13 MB on the input layer)
        x, wn, ws = _bf16c(x), _bf16c(w_neigh), _bf16c(w_self)
        dev, n_out = x.device, wn.shape[0]
        z = torch.empty(n_src, n_out, dtype=torch.bfloat16, device=dev)
        y = torch.empty(n_dst, n_out, dtype=torch.bfloat16, device=dev)
        norm = torch.empty(n_src, dtype=torch.bfloat16, device=dev)
        rows = torch.empty(n_src, x.shape[1], dtype=torch.bfloat16, device=dev) if ids is not None else x
        _tile_gemm(_tg_args(x, wn, z, n_src, ids=ids, m_dev=src_dev, a_copy=rows if ids is not None else None, in_norm=norm),
                   _tg_args(x, ws, y, n_dst, ids=ids, bias=b_self, m_dev=dst_dev), wide=wide)
        ctx.save_for_backward(rows, wn, ws)
        ctx.gathered, ctx.n_dst, ctx.has_bias = ids is not None, n_dst, b_self is not None
        ctx.n_src, ctx.src_dev, ctx.dst_dev = n_src, src_dev, dst_dev
        ctx.mark_non_differentiable(rows, norm) if ids is not None else ctx.mark_non_differentiable(norm)
        return z, y, rows, norm

    @staticmethod
    def backward(ctx, dz, dy, _drows, _dnorm):
        rows, wn, ws = ctx.saved_tensors
        want_dx = not ctx.gathered and ctx.needs_input_grad[0]
        d_wn = d_ws = d_b = dx = None
        if (_mfma_bwd_on() and dz is not None and dy is not None and wn.shape[0] <= 256 and _bwd_ok(rows, wn, ws)
                and dz.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16):
            # csrc/sage_bwd.hip: both weight gradients and the bias gradient in one launch pair, the input gradient
            # (both Linears into one accumulator) in one launch
            dz, dy = _bf16c(dz), _bf16c(dy)
            (d_wn, _), (d_ws, d_b) = sage_wgrad([(dz, rows, ctx.n_src, ctx.src_dev, False), (dy, rows, ctx.n_dst, ctx.dst_dev, ctx.has_bias)])
            if want_dx:
                dx = sage_dgrad(dz, wn, ctx.n_src, ctx.src_dev, a2=dy, w2=ws, m2_bound=ctx.n_dst, m2_dev=ctx.dst_dev)
                if _drows is not None:
                    dx = dx + _drows
            return dx, None, d_wn, d_ws, d_b, None, None, None, None, None
        if dz is not None:
            dz = _bf16c(dz)
            d_wn = _weight_grad(dz, rows)
            if want_dx:
                dx = dz @ wn
        if dy is not None:
            dy = _bf16c(dy)
            d_ws = _weight_grad(dy, rows[: ctx.n_dst])
            d_b = _bias_grad(dy) if ctx.has_bias else None
            if want_dx:
                if dx is None:
                    dx = torch.zeros_like(rows)
                dx[: ctx.n_dst].addmm_(dy, ws)                                   # (the GEMM accumulates: no separate add)
        if _drows is not None and want_dx:
            dx = _drows if dx is None else dx + _drows
        return dx, None, d_wn, d_ws, d_b, None, None, None, None, None


class _SageLinearSplit(torch.autograd.Function):
    """_SageLinearPair for a block whose destinations are NOT its leading source rows (a shard's block: the destinations are
    this rank's seeds, anywhere in the global source list): fc_neigh over the source rows and fc_self (+bias) over the
    destination rows -- handed in beside them, or gathered from the source rows through ``dst_ids`` by the launch itself --,
    ONE launch; the input rows' bf16 norms come with it.  Backward on csrc/sage_bwd.hip: both weight gradients and the bias
    gradient in one launch pair, an input gradient per operand."""

    @staticmethod
    def forward(ctx, x_src, x_dst, w_neigh, w_self, b_self, src_dev, dst_dev, dst_ids=None):
        ctx.set_materialize_grads(False)
        xs, wn, ws = _bf16c(x_src), _bf16c(w_neigh), _bf16c(w_self)
        dev, n_out = xs.device, wn.shape[0]
        gathered = x_dst is None
        n_dst = dst_ids.numel() if gathered else x_dst.shape[0]
        xd = torch.empty(n_dst, xs.shape[1], dtype=torch.bfloat16, device=dev) if gathered else _bf16c(x_dst)
        z = torch.empty(xs.shape[0], n_out, dtype=torch.bfloat16, device=dev)
        y = torch.empty(n_dst, n_out, dtype=torch.bfloat16, device=dev)
        norm = torch.empty(xs.shape[0], dtype=torch.bfloat16, device=dev)
        second = (_tg_args(xs, ws, y, n_dst, ids=dst_ids, bias=b_self, m_dev=dst_dev, a_copy=xd) if gathered
                  else _tg_args(xd, ws, y, n_dst, bias=b_self, m_dev=dst_dev))
        _tile_gemm(_tg_args(xs, wn, z, xs.shape[0], m_dev=src_dev, in_norm=norm), second)
        ctx.save_for_backward(xs, xd, wn, ws, dst_ids if gathered else None)
        ctx.has_bias, ctx.src_dev, ctx.dst_dev, ctx.gathered = b_self is not None, src_dev, dst_dev, gathered
        ctx.mark_non_differentiable(norm)
        return z, y, norm

    @staticmethod
    def backward(ctx, dz, dy, _dnorm):
        xs, xd, wn, ws, ids = ctx.saved_tensors
        d_wn = d_ws = d_b = dxs = dxd = None
        probs = []
        if dz is not None:
            dz = _bf16c(dz)
            probs.append((dz, xs, xs.shape[0], ctx.src_dev, False))
        if dy is not None:
            dy = _bf16c(dy)
            probs.append((dy, xd, xd.shape[0], ctx.dst_dev, ctx.has_bias))
        if probs:
            outs = sage_wgrad(probs)
            if dz is not None:
                d_wn = outs[0][0]
            if dy is not None:
                d_ws, d_b = outs[-1]
        if dz is not None and ctx.needs_input_grad[0]:
            dxs = sage_dgrad(dz, wn, xs.shape[0], ctx.src_dev)
        if dy is not None and ctx.needs_input_grad[0 if ctx.gathered else 1]:
            dxd = sage_dgrad(dy, ws, xd.shape[0], ctx.dst_dev)           # (rows at or beyond the true count: zeros)
            if ctx.gathered:                                             # the destination rows came out of x_src: back into its gradient
                dxs = torch.empty_like(xs).fill_(0) if dxs is None else dxs
                dxs.index_add_(0, ids, dxd)                              # (the padding ids repeat row 0 and carry zero rows)
                dxd = None
        return dxs, dxd, d_wn, d_ws, d_b, None, None, None


_ones_rows = {}


def _bias_grad(d):
    """d.sum(0) (the bias gradient of a Linear layer) as a [1, rows] x [rows, out] product with a row of ones: fp32 accumulation,
    one rounding, like aten::sum -- which runs this tall reduction as a memset plus an atomic kernel (15.7 vs 9.8 us for
    5 K x 256, 11.7 vs 6.5 for 2 K x 256; scratch/biasbench.py)."""
    if not (d.is_cuda and d.dim() == 2 and d.shape[0] >= 1024):
        return d.sum(0)
    key = (d.device.index, d.dtype)
    buf = _ones_rows.get(key)
    if buf is None or buf.shape[1] < d.shape[0]:
        buf = _ones_rows[key] = torch.ones(1, max(d.shape[0], 16384), dtype=d.dtype, device=d.device)
    return (buf[:, : d.shape[0]] @ d)[0]


def _weight_grad(d, x, split=4):
    """d.t() @ x for a long reduction (thousands of block rows) and a small result (out x in features): the library runs it on
    out/64 x in/64 = 40 workgroups, a sixth of the chip.  Split the rows into ``split`` batches (fp32 partial products, one
    rounding at the end: the bits of the plain call): 44 -> 32 us for 11 K x 256 x 602, 22.5 -> 19.6 for 5 K rows
    (scratch/dwbench.py, graph replay)."""
    R = d.shape[0]
    if R < 8192 or x.shape[1] < 512 or R % split or not d.is_cuda:       # (in the loop the 5 K-row product is no faster split)
        return d.t() @ x
    p = torch.bmm(d.view(split, R // split, d.shape[1]).transpose(1, 2), x.reshape(split, R // split, x.shape[1]), out_dtype=torch.float32)
    return p.sum(0).to(d.dtype)


def _dropout_needs_relu(relu, p):
    """bliss_sage_epilogue_bwd takes the dropout mask AND the ReLU mask from ``out > 0`` (include/bliss_gnn.h): without the ReLU
    a kept negative element would lose its gradient.  Refused before any launch."""
    if p > 0 and not relu:
        raise ValueError("dropout (p = %g) without ReLU: the backward reads its mask from out > 0, which is the dropout mask "
                         "only behind a ReLU" % p)


class _SageDualLinear(torch.autograd.Function):
    """An aggregate-first SAGEConv layer's tail (in <= out): fc_neigh(h_neigh) + fc_self(h_dst) + bias, ReLU, dropout and the
    row norms of the result (model.py:321-333, :318-320 of the next layer) in ONE launch: both products accumulate in the
    same fp32 registers, one rounding to bf16."""

    @staticmethod
    def forward(ctx, a_neigh, a_self, w_neigh, w_self, bias, relu, p, ctr, seed, n_rows, rows_dev):
        ctx.set_materialize_grads(False)
        _dropout_needs_relu(relu, p)
        a1, a2, w1, w2 = _bf16c(a_neigh), _bf16c(a_self), _bf16c(w_neigh), _bf16c(w_self)
        out = torch.empty(n_rows, w1.shape[0], dtype=torch.bfloat16, device=a1.device)
        norm = torch.empty(n_rows, dtype=torch.bfloat16, device=a1.device)
        _tile_gemm(_tg_args(a1, w1, out, n_rows, a2=a2, w2=w2, bias=bias, m_dev=rows_dev, out_norm=norm, relu=relu, p=p, seed=seed, ctr=ctr))
        ctx.save_for_backward(a1, a2, w1, w2, out)
        ctx.relu, ctx.p, ctx.has_bias, ctx.rows_dev = relu, float(p), bias is not None, rows_dev
        ctx.mark_non_differentiable(norm)
        return out, norm

    @staticmethod
    def backward(ctx, dout, _dnorm):
        a1, a2, w1, w2, out = ctx.saved_tensors
        if dout is None:
            return (None,) * 11
        d = _bf16c(dout)
        if ctx.relu or ctx.p > 0:
            din = torch.empty_like(out)
            _lib.check(_lib.lib.bliss_sage_epilogue_bwd(d.data_ptr(), d.stride(0), out.data_ptr(), out.stride(0), out.shape[0],
                                                        out.shape[1], ctx.p, din.data_ptr(), din.stride(0), _stream()),
                       "bliss_sage_epilogue_bwd")
            d = din
        if _mfma_bwd_on() and w1.shape[0] <= 256 and _bwd_ok(d, a1, a2, w1, w2) and a1.shape[0] == d.shape[0] and a2.shape[0] >= d.shape[0]:
            rd = ctx.rows_dev
            (dw1, _), (dw2, db) = sage_wgrad([(d, a1, d.shape[0], rd, False), (d, a2, d.shape[0], rd, ctx.has_bias)])
            da1 = sage_dgrad(d, w1, d.shape[0], rd) if ctx.needs_input_grad[0] else None
            da2 = None
            if ctx.needs_input_grad[1]:
                da2 = sage_dgrad(d, w2, d.shape[0], rd)
                if a2.shape[0] > d.shape[0]:
                    da2 = torch.cat([da2, torch.zeros(a2.shape[0] - d.shape[0], da2.shape[1], dtype=da2.dtype, device=da2.device)])
            return (da1, da2, dw1, dw2, db, None, None, None, None, None, None)
        return (d @ w1, d @ w2, d.t() @ a1, d.t() @ a2, _bias_grad(d) if ctx.has_bias else None, None, None, None, None, None, None)


class _SageAggDual(torch.autograd.Function):
    """Aggregation + _SageDualLinear as ONE autograd node: the layer input h feeds both the SpMM and (its first rows) fc_self, and
    two nodes made autograd zero-pad the slice's gradient and add the two (fill + copy + add kernels, 5 K x 256 each); here the
    fc_self product accumulates straight into the transposed SpMM's result.  Edge weights that require a gradient get
    gw_e = (d W_neigh)[dst_e] . h[src_e] / deg_{dst_e} (bliss::sddmm): one more dense launch for d W_neigh on
    the destination rows, issued in that case only."""

    @staticmethod
    def forward(ctx, h, indptr, src, dst, w, counts, t_indptr, t_edge, n_dst, w_neigh, w_self, bias, relu, p, ctr, seed, rows_dev):
        from . import ops
        ctx.set_materialize_grads(False)
        _dropout_needs_relu(relu, p)
        h, w1, w2 = _bf16c(h), _bf16c(w_neigh), _bf16c(w_self)
        agg = ops.spmm(indptr, src, dst, w, h, n_dst, counts, True, False, None, None)
        out = torch.empty(n_dst, w1.shape[0], dtype=torch.bfloat16, device=h.device)
        norm = torch.empty(n_dst, dtype=torch.bfloat16, device=h.device)
        _tile_gemm(_tg_args(agg, w1, out, n_dst, a2=h, w2=w2, bias=bias, m_dev=rows_dev, out_norm=norm, relu=relu, p=p, seed=seed, ctr=ctr))
        ctx.save_for_backward(agg, h, w1, w2, out, indptr, src, dst, w, counts, t_indptr, t_edge)
        ctx.relu, ctx.p, ctx.has_bias, ctx.n_dst, ctx.rows_dev = relu, float(p), bias is not None, n_dst, rows_dev
        ctx.mark_non_differentiable(norm)
        return out, norm

    @staticmethod
    def backward(ctx, dout, _dnorm):
        from . import ops
        agg, h, w1, w2, out, indptr, src, dst, w, counts, t_indptr, t_edge = ctx.saved_tensors
        if dout is None:
            return (None,) * 17
        d = _bf16c(dout)
        if ctx.relu or ctx.p > 0:
            din = torch.empty_like(out)
            _lib.check(_lib.lib.bliss_sage_epilogue_bwd(d.data_ptr(), d.stride(0), out.data_ptr(), out.stride(0), out.shape[0],
                                                        out.shape[1], ctx.p, din.data_ptr(), din.stride(0), _stream()),
                       "bliss_sage_epilogue_bwd")
            d = din
        gh = gw = None
        mfma = _mfma_bwd_on() and w1.shape[0] <= 256 and _bwd_ok(d, agg, h, w1, w2)
        if w is not None and ctx.needs_input_grad[4]:
            dn = sage_dgrad(d, w1, ctx.n_dst, ctx.rows_dev) if mfma else d @ w1
            gw = ops.sddmm(src, dst, indptr, dn, h, None, counts, _lib.SDDMM_MEAN, False)
        if ctx.needs_input_grad[0]:
            if t_indptr is None or t_edge is None:
                raise RuntimeError("the block's by-source index (Block.transposed()) is needed to differentiate w.r.t. h")
            if mfma:
                # A^T (d W_neigh) = (A^T d) W_neigh: the transposed aggregation first, then ONE launch for both Linears' input
                # gradients -- gh = T W_neigh + (d W_self on the destination rows), fp32 accumulation, one rounding
                t = ops.spmm_t(t_indptr, t_edge, src, dst, indptr, w, d, h.shape[0], counts, True)
                src_dev = counts.data_ptr() + 12 if counts is not None else 0
                gh = sage_dgrad(t, w1, h.shape[0], src_dev, a2=d, w2=w2, m2_bound=ctx.n_dst, m2_dev=ctx.rows_dev)
            else:
                gh = ops.spmm_t(t_indptr, t_edge, src, dst, indptr, w, d @ w1 if gw is None else dn, h.shape[0], counts, True)
                gh[: ctx.n_dst].addmm_(d, w2)
        if mfma:
            (dw1, _), (dw2, db) = sage_wgrad([(d, agg, ctx.n_dst, ctx.rows_dev, False), (d, h, ctx.n_dst, ctx.rows_dev, ctx.has_bias)])
            return (gh, None, None, None, gw, None, None, None, None, dw1, dw2, db, None, None, None, None, None)
        return (gh, None, None, None, gw, None, None, None, None, d.t() @ agg, d.t() @ h[: ctx.n_dst],
                _bias_grad(d) if ctx.has_bias else None, None, None, None, None, None)


def sage_agg_dual(block, h, edge_weight, w_neigh, w_self, bias, relu, p, ctr, seed, rows_dev):
    """mean-aggregate ``h`` over ``block`` and apply fc_neigh(h_neigh) + fc_self(h_dst) + bias (+ ReLU, dropout, row norms)."""
    assert h.is_cuda and h.dtype == torch.bfloat16
    _wait_block(block)
    w = None
    if edge_weight is not None:
        w = edge_weight.reshape(-1)
        w = (w if w.dtype == torch.bfloat16 else w.bfloat16()).contiguous()
    counts = getattr(block, "_counts_dev", None) if block._nnz_ptr else None
    need_t = h.requires_grad and torch.is_grad_enabled()
    t_indptr, t_edge = block.transposed() if need_t else (None, None)
    return _SageAggDual.apply(h, block.indptr, block.src, block.dst, w, counts, t_indptr, t_edge, block.num_dst_nodes(), w_neigh, w_self,
                              bias, relu, p, ctr, seed, rows_dev)


def tile_gemm_ok(in_feats, out_feats, wide=False):
    return in_feats <= (TILE_WIDE_MAX_K if wide else TILE_GEMM_MAX_K) and out_feats <= TILE_GEMM_MAX_N


class SAGEConv(nn.Module):
    """dglnn.SAGEConv(in_feats, out_feats, 'mean') as used at model.py:303-308, 321-329, and [DGL-recalled] the 'pool'
    aggregator: neigh = max over the in-edges of relu(fc_pool(feat_src))[src_e] * w_e, then fc_neigh --
    never fc_neigh before the aggregation, which DGL has for 'mean' and 'gcn' only; and [DGL-recalled] the 'gcn' aggregator, which SAGEGCNConv below constructs (DESIGN.md
    section 34): rst = fc_neigh o agg + bias, agg[i] = (sum_e w_e z[src_e] + z_dst[i]) / (deg_i + 1), fc_neigh first iff in > out, no
    fc_self, a plain ``bias`` parameter."""

    _AGGREGATORS = ("mean", "pool")              # what this class's constructor takes; SAGEGCNConv below: ("gcn",), SAGELSTMConv: ("lstm",)

    def __init__(self, in_feats, out_feats, aggregator_type="mean", feat_drop=0.0, bias=True, norm=None, activation=None):
        super().__init__()
        if aggregator_type not in self._AGGREGATORS:
            raise NotImplementedError("SAGEConv: aggregator_type 'mean' (model.py:303-308) and 'pool' are built here, 'gcn' as "
                                      "nn.SAGEGCNConv(in_feats, out_feats, ...) and 'lstm' as nn.SAGELSTMConv(in_feats, out_feats, ...) "
                                      "(DESIGN.md sections 34 and 37), not %r" % (aggregator_type,))
        if aggregator_type == "lstm" and in_feats > LSTM_MAX_DIM:
            raise NotImplementedError("SAGELSTMConv: in_feats <= %d (the tile of csrc/lstm.hip, DESIGN.md section 37), not %d"
                                      % (LSTM_MAX_DIM, in_feats))
        self._aggre_type = aggregator_type
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self.feat_drop = nn.Dropout(feat_drop)
        self.norm, self.activation = norm, activation
        if aggregator_type == "pool":
            self.fc_pool = nn.Linear(in_feats, in_feats)
        if aggregator_type == "lstm":
            self.lstm = nn.LSTM(in_feats, in_feats, batch_first=True)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        if aggregator_type == "gcn":                 # no fc_self: the destination's own row rides in the aggregation; a plain bias
            if bias:
                self.bias = nn.Parameter(torch.zeros(out_feats))
            else:
                self.register_parameter("bias", None)
        else:
            self.fc_self = nn.Linear(in_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        if self._aggre_type == "pool":
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)
        if self._aggre_type == "lstm":
            self.lstm.reset_parameters()             # uniform +-1 / sqrt(in_feats), as DGL leaves it
        if self._aggre_type == "gcn":
            if self.bias is not None:
                nn.init.zeros_(self.bias)
        else:
            nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def _forward_gcn(self, graph, feat_src, feat_dst, edge_weight):
        """rst = fc_neigh o agg, agg[i] = (sum_e w_e z[src_e] + z_dst[i]) / (deg_i + 1); ``feat_dst`` None: the
        destinations are the leading source rows."""
        lin_first = self._in_src_feats > self._out_feats
        z = self.fc_neigh(feat_src) if lin_first else feat_src
        z_dst = None
        if feat_dst is not None:
            z_dst = self.fc_neigh(feat_dst) if lin_first else feat_dst
        agg = gcn_aggregate(graph, z, edge_weight, z_dst)
        rst = agg if lin_first else self.fc_neigh(agg)
        return rst if self.bias is None else rst + self.bias

    def forward(self, graph, feat, edge_weight=None, parts=False):
        """``parts=True`` returns (fc_self(h_dst), h_neigh) un-added, for a caller that fuses the sum with what follows ('gcn' has no
        two parts: the finished tensor)."""
        if isinstance(feat, tuple):                  # (feat_src, feat_dst) like dglnn.SAGEConv: destinations that are not the
            feat_src, feat_dst = self.feat_drop(feat[0]), self.feat_drop(feat[1])      # leading source rows (shard blocks)
        else:
            feat_src = self.feat_drop(feat)
            feat_dst = feat_src[: graph.num_dst_nodes()]
        if self._aggre_type == "gcn":
            rst = self._forward_gcn(graph, feat_src, feat_dst if isinstance(feat, tuple) else None, edge_weight)
            if self.activation is not None:
                rst = self.activation(rst)
            if self.norm is not None:
                rst = self.norm(rst)
            return rst
        if self._aggre_type == "pool":
            h_neigh = self.fc_neigh(max_aggregate(graph, torch.relu(self.fc_pool(feat_src)), edge_weight))
        elif self._aggre_type == "lstm":             # never fc_neigh before the recurrence
            h_neigh = self.fc_neigh(lstm_aggregate(graph, feat_src, self.lstm, edge_weight))
        elif self._in_src_feats > self._out_feats:   # fc_neigh before the aggregation
            h_neigh = weighted_aggregate(graph, self.fc_neigh(feat_src), edge_weight, mean=True)
        else:
            h_neigh = self.fc_neigh(weighted_aggregate(graph, feat_src, edge_weight, mean=True))
        if parts and self.activation is None and self.norm is None:
            return self.fc_self(feat_dst), h_neigh
        rst = self.fc_self(feat_dst) + h_neigh
        if self.activation is not None:
            rst = self.activation(rst)
        if self.norm is not None:
            rst = self.norm(rst)
        return rst


class SAGEGCNConv(SAGEConv):
    """[DGL-recalled] dglnn.SAGEConv(in_feats, out_feats, 'gcn'), a class of its own because
    ``SAGEConv(in, out, "gcn")`` keeps refusing, as it always has: rst = fc_neigh o agg + bias, agg[i] = (sum_e w_e z[src_e] +
    z_dst[i]) / (deg_i + 1), fc_neigh first iff in > out; parameters ``fc_neigh.weight`` and a plain ``bias``, no ``fc_self``.
    ``forward(graph, feat, edge_weight=None)`` is SAGEConv's, both orders of fc_neigh and the (feat_src, feat_dst) pair form."""
    _AGGREGATORS = ("gcn",)

    def __init__(self, in_feats, out_feats, feat_drop=0.0, bias=True, norm=None, activation=None):
        super().__init__(in_feats, out_feats, "gcn", feat_drop=feat_drop, bias=bias, norm=norm, activation=activation)


class SAGELSTMConv(SAGEConv):
    """[DGL-recalled] dglnn.SAGEConv(in_feats, out_feats, 'lstm'), a class of its own for SAGEGCNConv's
    reason (``SAGEConv(in, out, "lstm")`` keeps refusing): rst = fc_self(h_dst) + fc_neigh(neigh), neigh[d] = the last hidden state
    of ``lstm = nn.LSTM(in, in, batch_first=True)`` run over w_e h[src_e] for d's in-edges in row order (nn.lstm_aggregate).
    Parameters ``lstm.weight_ih_l0``, ``lstm.weight_hh_l0`` (4 in, in), ``lstm.bias_ih_l0``, ``lstm.bias_hh_l0`` (4 in,),
    ``fc_neigh.weight``, ``fc_self.weight``, ``fc_self.bias``.  ``forward(graph, feat, edge_weight=None, parts=False)`` is
    SAGEConv's.  in_feats <= 256; bf16 on the GPU or NotImplementedError."""
    _AGGREGATORS = ("lstm",)

    def __init__(self, in_feats, out_feats, feat_drop=0.0, bias=True, norm=None, activation=None):
        super().__init__(in_feats, out_feats, "lstm", feat_drop=feat_drop, bias=bias, norm=norm, activation=activation)


# transforms="tile" (DESIGN.md section 26): GraphConv(norm='both') on bounded kernels -- the degree-normalised SpMM of csrc/gcn.hip,
# the dense products on the MFMA entry points with the operand roles swapped (weight stays [in, out]) and one row-wise epilogue
# launch per direction; every loop that crosses rows or edges is bounded by the block's device-side counts.
# transforms="wide" (DESIGN.md section 29): everything "tile" is, with in_feats up to TILE_WIDE_MAX_K -- the one product whose
# reduction is in_feats walks it in panels when it passes TILE_GEMM_MAX_K; a layer within 1024 has the launches and bits of "tile".
GCN_TRANSFORMS = ("library", "tile", "wide")
TILE_KINDS = ("tile", "wide")            # the values of ``transforms`` that take the bounded-kernel branch


def _is_relu(act):
    return act in (torch.relu, torch.nn.functional.relu) or isinstance(act, nn.ReLU)


def _gcn_spmm(backward, idx, w, ns, nd, h, n_rows, nnz_dev):
    """bliss_gcn_spmm_fwd (out [n_dst, dim] from h [n_src, dim]) or _bwd (gh [n_src, dim] from gout [n_dst, dim]) over
    ``idx`` = (indptr, src, dst, t_indptr, t_edge)."""
    indptr, src, dst, t_indptr, t_edge = idx
    B, D = int(src.numel()), h.shape[1]
    out = torch.empty(n_rows, D, dtype=torch.bfloat16, device=h.device)
    part = spmm_partials(B, D, h.device, floor=4)
    wp = 0 if w is None else w.data_ptr()
    if backward:
        _lib.check(_lib.lib.bliss_gcn_spmm_bwd(t_indptr.data_ptr(), t_edge.data_ptr(), src.data_ptr(), dst.data_ptr(), wp, ns.data_ptr(),
                                               nd.data_ptr(), h.data_ptr(), h.stride(0), n_rows, nnz_dev, B, D, out.data_ptr(), out.stride(0),
                                               part.data_ptr(), _stream()), "bliss_gcn_spmm_bwd")
    else:
        _lib.check(_lib.lib.bliss_gcn_spmm_fwd(indptr.data_ptr(), src.data_ptr(), dst.data_ptr(), wp, ns.data_ptr(), nd.data_ptr(),
                                               h.data_ptr(), h.stride(0), n_rows, nnz_dev, B, D, out.data_ptr(), out.stride(0),
                                               part.data_ptr(), _stream()), "bliss_gcn_spmm_fwd")
    return out


def _gcn_xwt(d, w, m_bound, m_dev):
    """d[m, out] . W^T -> [m, in] for W = [in, out]: bliss_tile_gemm reads W as an nn.Linear weight [n = in, k = out]; output-column
    blocks of at most 256, two per launch; zero rows at or past the count."""
    out = torch.empty(m_bound, w.shape[0], dtype=torch.bfloat16, device=d.device)
    sets = [_tg_args(d, w[c0:c1], out[:, c0:c1], m_bound, m_dev=m_dev) for c0, c1 in _col_blocks(w.shape[0])]
    for i in range(0, len(sets), 2):
        _tile_gemm(sets[i], sets[i + 1] if i + 1 < len(sets) else None)
    return out


def _gcn_epilogue_args(n_rows, rows_dev, width, relu, p, state, ctr_used):
    t = _lib.GcnEpilogue()
    t.n_rows, t.rows_dev, t.width, t.relu = int(n_rows), int(rows_dev), int(width), int(bool(relu))
    if p > 0:
        t.drop_p, t.drop_seed, t.drop_ctr, t.drop_ctr_used = float(p), int(state["seed"]) & 0xFFFFFFFF, state["ctr"].data_ptr(), ctr_used.data_ptr()
    return t


class _GcnLayer(torch.autograd.Function):
    """One GraphConv(norm='both') layer on the bounded kernels: the norms (bliss_gcn_norms), the product with ``weight`` [in, out]
    before (in > out) or behind the degree-normalised SpMM (bliss_gat_dgrad: A[m, k] . W[k, n]) and the epilogue (bias, ReLU,
    keyed dropout, the row norms of the stored rows).  Backward: the epilogue's mirror with the bias gradient, the transposed
    SpMM, dX on bliss_tile_gemm, dW = X^T dY on bliss_sage_wgrad -- all bound by the block's device-side counts."""

    @staticmethod
    def forward(ctx, x, weight, bias, idx, ew, n_src, n_dst, words, relu, p, state, want_norm, wide=False):
        import ctypes as C
        ctx.set_materialize_grads(False)
        x, w = _bf16c(x), _bf16c(weight)
        dev = x.device
        dst_dev, src_dev, nnz_dev = words
        indptr, t_indptr = idx[0], idx[3]
        ns = torch.empty(n_src, dtype=torch.float32, device=dev)
        nd = torch.empty(n_dst, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib.bliss_gcn_norms(indptr.data_ptr(), n_dst, t_indptr.data_ptr(), n_src, nd.data_ptr(), ns.data_ptr(), _stream()),
                   "bliss_gcn_norms")
        w_first = w.shape[0] > w.shape[1]
        if w_first:
            kept = x
            a = _gcn_spmm(False, idx, ew, ns, nd, gat_dgrad(x, w, n_src, src_dev, wide=wide), n_dst, nnz_dev)    # (k = in_feats)
        else:
            kept = _gcn_spmm(False, idx, ew, ns, nd, x, n_dst, nnz_dev)
            a = gat_dgrad(kept, w, n_dst, dst_dev)
        width = w.shape[1]
        out = torch.empty(n_dst, width, dtype=torch.bfloat16, device=dev)
        norm = torch.empty(n_dst, dtype=torch.bfloat16, device=dev) if want_norm else None
        ctr_used = torch.empty(1, dtype=torch.int32, device=dev) if p > 0 else None
        t = _gcn_epilogue_args(n_dst, dst_dev, width, relu, p, state, ctr_used)
        t.a, t.a_stride, t.bias = a.data_ptr(), a.stride(0), 0 if bias is None else bias.data_ptr()
        t.out, t.out_stride, t.norm_out = out.data_ptr(), out.stride(0), 0 if norm is None else norm.data_ptr()
        _lib.check(_lib.lib.bliss_gcn_epilogue_fwd(C.byref(t), _stream()), "bliss_gcn_epilogue_fwd")
        ctx.save_for_backward(kept, w, out if relu else None, ew, ns, nd, ctr_used, *idx)
        ctx.cfg = (w_first, n_src, n_dst, words, bool(relu), float(p), state, bias is not None, x.shape[0])
        if norm is not None:
            ctx.mark_non_differentiable(norm)
        return out, norm

    @staticmethod
    def backward(ctx, dout, _dnorm):
        import ctypes as C
        kept, w, out, ew, ns, nd, ctr_used = ctx.saved_tensors[:7]
        idx = tuple(ctx.saved_tensors[7:])
        w_first, n_src, n_dst, words, relu, p, state, has_bias, x_rows = ctx.cfg
        if dout is None:
            return (None,) * 13
        dst_dev, src_dev, nnz_dev = words
        dout = _bf16c(dout)
        dev, width = dout.device, w.shape[1]
        g = torch.empty(n_dst, width, dtype=torch.bfloat16, device=dev)
        db = torch.empty(width, dtype=torch.bfloat16, device=dev) if has_bias else None
        t = _gcn_epilogue_args(n_dst, dst_dev, width, relu, p, state, ctr_used)
        t.dout, t.dout_stride, t.din, t.din_stride = dout.data_ptr(), dout.stride(0), g.data_ptr(), g.stride(0)
        if relu:
            t.out, t.out_stride = out.data_ptr(), out.stride(0)
        if has_bias:
            rows = int(_lib.lib.bliss_gcn_db_chunk_rows())
            part = torch.empty(max(((n_dst + rows - 1) // rows) * width, 4), dtype=torch.float32, device=dev)
            t.db, t.db_partials = db.data_ptr(), part.data_ptr()
        _lib.check(_lib.lib.bliss_gcn_epilogue_bwd(C.byref(t), _stream()), "bliss_gcn_epilogue_bwd")
        dx = None
        if w_first:
            dz = _gcn_spmm(True, idx, ew, ns, nd, g, n_src, nnz_dev)                       # [n_src, out]
            dw = _wgrad_blocks([(kept, dz, n_src, src_dev, False)])[0][0]
            if ctx.needs_input_grad[0]:
                dx = _gcn_xwt(dz, w, n_src, src_dev)
        else:
            dw = _wgrad_blocks([(kept, g, n_dst, dst_dev, False)])[0][0]
            if ctx.needs_input_grad[0]:
                dx = _gcn_spmm(True, idx, ew, ns, nd, _gcn_xwt(g, w, n_dst, dst_dev), n_src, nnz_dev)
        if dx is not None and x_rows > n_src:
            dx = torch.cat([dx, _zero_rows(x_rows - n_src, dx)])
        return (dx, dw, db) + (None,) * 10


# transforms="tile" for SAGEConv 'gcn' (DESIGN.md section 34): fc_neigh on bliss_tile_gemm, the self-inclusive normalised sum of
# csrc/spmm_self.hip and GraphConv's row-wise epilogue; every loop that crosses rows or edges is bounded by the block's device-side counts.
def _spmm_self_launch(backward, idx, w, h, n_src, n_dst, words):
    """bliss_spmm_self_fwd (out [n_dst, dim] from h [n_src, dim], the self rows = h's leading rows) or _bwd (gh [n_src, dim] from
    gout [n_dst, dim], the self term folded in) over ``idx`` = (indptr, src, dst, t_indptr, t_edge)."""
    indptr, src, dst, t_indptr, t_edge = idx
    dst_dev, _src_dev, nnz_dev = words
    B, D = int(src.numel()), h.shape[1]
    out = torch.empty(n_src if backward else n_dst, D, dtype=torch.bfloat16, device=h.device)
    part = spmm_partials(B, D, h.device, floor=4)
    wp = 0 if w is None else w.data_ptr()
    if backward:
        _lib.check(_lib.lib.bliss_spmm_self_bwd(t_indptr.data_ptr(), t_edge.data_ptr(), src.data_ptr(), dst.data_ptr(), indptr.data_ptr(), wp,
                                                h.data_ptr(), h.stride(0), n_src, n_dst, dst_dev, nnz_dev, B, D, out.data_ptr(), out.stride(0),
                                                part.data_ptr(), _stream()), "bliss_spmm_self_bwd")
    else:
        _lib.check(_lib.lib.bliss_spmm_self_fwd(indptr.data_ptr(), src.data_ptr(), dst.data_ptr(), wp, h.data_ptr(), h.stride(0), h.data_ptr(),
                                                h.stride(0), n_dst, dst_dev, nnz_dev, B, D, out.data_ptr(), out.stride(0), part.data_ptr(),
                                                _stream()), "bliss_spmm_self_fwd")
    return out


def _linear_tile(x, w, m_bound, m_dev):
    """x[m, in] . W^T -> [m, out] for an nn.Linear weight W = [out, in] on bliss_tile_gemm: output-column blocks of at most 256, two
    per launch; zero rows at or past the count."""
    out = torch.empty(m_bound, w.shape[0], dtype=torch.bfloat16, device=x.device)
    sets = [_tg_args(x, w[c0:c1], out[:, c0:c1], m_bound, m_dev=m_dev) for c0, c1 in _col_blocks(w.shape[0])]
    for i in range(0, len(sets), 2):
        _tile_gemm(sets[i], sets[i + 1] if i + 1 < len(sets) else None)
    return out


class _SageGcnTile(torch.autograd.Function):
    """One SAGEGCNConv layer (SAGEConv 'gcn') on the bounded kernels, ONE autograd node: fc_neigh (``weight`` [out, in], an
    nn.Linear weight) on bliss_tile_gemm before (in > out) or behind the self-inclusive normalised sum (bliss_spmm_self_fwd), and
    GraphConv's epilogue (bias, ReLU, keyed dropout, the row norms of the stored rows).  Backward: the epilogue's mirror with the bias
    gradient, bliss_spmm_self_bwd, dX on bliss_gat_dgrad, dW = dY^T X on bliss_sage_wgrad -- all bound by the block's device-side
    counts."""

    @staticmethod
    def forward(ctx, x, weight, bias, idx, ew, n_src, n_dst, words, relu, p, state, want_norm):
        import ctypes as C
        ctx.set_materialize_grads(False)
        x, w = _bf16c(x), _bf16c(weight)
        dev = x.device
        dst_dev, src_dev, _nnz_dev = words
        lin_first = w.shape[1] > w.shape[0]
        if lin_first:
            kept = x
            a = _spmm_self_launch(False, idx, ew, _linear_tile(x, w, n_src, src_dev), n_src, n_dst, words)
        else:
            kept = _spmm_self_launch(False, idx, ew, x, n_src, n_dst, words)
            a = _linear_tile(kept, w, n_dst, dst_dev)
        width = w.shape[0]
        out = torch.empty(n_dst, width, dtype=torch.bfloat16, device=dev)
        norm = torch.empty(n_dst, dtype=torch.bfloat16, device=dev) if want_norm else None
        ctr_used = torch.empty(1, dtype=torch.int32, device=dev) if p > 0 else None
        t = _gcn_epilogue_args(n_dst, dst_dev, width, relu, p, state, ctr_used)
        t.a, t.a_stride, t.bias = a.data_ptr(), a.stride(0), 0 if bias is None else bias.data_ptr()
        t.out, t.out_stride, t.norm_out = out.data_ptr(), out.stride(0), 0 if norm is None else norm.data_ptr()
        _lib.check(_lib.lib.bliss_gcn_epilogue_fwd(C.byref(t), _stream()), "bliss_gcn_epilogue_fwd")
        ctx.save_for_backward(kept, w, out if relu else None, ew, ctr_used, *idx)
        ctx.cfg = (lin_first, n_src, n_dst, words, bool(relu), float(p), state, bias is not None, x.shape[0])
        if norm is not None:
            ctx.mark_non_differentiable(norm)
        return out, norm

    @staticmethod
    def backward(ctx, dout, _dnorm):
        import ctypes as C
        kept, w, out, ew, ctr_used = ctx.saved_tensors[:5]
        idx = tuple(ctx.saved_tensors[5:])
        lin_first, n_src, n_dst, words, relu, p, state, has_bias, x_rows = ctx.cfg
        if dout is None:
            return (None,) * 12
        dst_dev, src_dev, _nnz_dev = words
        dout = _bf16c(dout)
        dev, width = dout.device, w.shape[0]
        g = torch.empty(n_dst, width, dtype=torch.bfloat16, device=dev)
        db = torch.empty(width, dtype=torch.bfloat16, device=dev) if has_bias else None
        t = _gcn_epilogue_args(n_dst, dst_dev, width, relu, p, state, ctr_used)
        t.dout, t.dout_stride, t.din, t.din_stride = dout.data_ptr(), dout.stride(0), g.data_ptr(), g.stride(0)
        if relu:
            t.out, t.out_stride = out.data_ptr(), out.stride(0)
        if has_bias:
            rows = int(_lib.lib.bliss_gcn_db_chunk_rows())
            part = torch.empty(max(((n_dst + rows - 1) // rows) * width, 4), dtype=torch.float32, device=dev)
            t.db, t.db_partials = db.data_ptr(), part.data_ptr()
        _lib.check(_lib.lib.bliss_gcn_epilogue_bwd(C.byref(t), _stream()), "bliss_gcn_epilogue_bwd")
        dx = None
        if lin_first:
            dz = _spmm_self_launch(True, idx, ew, g, n_src, n_dst, words)                  # [n_src, out]
            dw = _wgrad_blocks([(dz, kept, n_src, src_dev, False)])[0][0]
            if ctx.needs_input_grad[0]:
                dx = gat_dgrad(dz, w, n_src, src_dev)
        else:
            dw = _wgrad_blocks([(g, kept, n_dst, dst_dev, False)])[0][0]
            if ctx.needs_input_grad[0]:
                dx = _spmm_self_launch(True, idx, ew, gat_dgrad(g, w, n_dst, dst_dev), n_src, n_dst, words)
        if dx is not None and x_rows > n_src:
            dx = torch.cat([dx, _zero_rows(x_rows - n_src, dx)])
        return (dx, dw, db) + (None,) * 9


def sage_gcn_tile(block, h, edge_weight, layer, relu, p, state, want_norm):
    """``layer`` = SAGEGCNConv(in, out) on ``block`` through _SageGcnTile: (out [n_dst, out_feats], its bf16 row norms or None).
    ``h``: bf16 [>= num_src_nodes, in_feats] on the GPU.  Rows at or past the block's live destination count come out as zeros."""
    K, S = block.num_src_nodes(), block.num_dst_nodes()
    if not (torch.is_tensor(h) and h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 2):
        raise NotImplementedError('SAGEConv "gcn": transforms="tile" takes bf16 features [rows, in_feats] on the GPU')
    if h.shape[0] < K or h.shape[1] != layer._in_src_feats or S > K:
        raise ValueError('SAGEConv "gcn": %d x %d input rows for a block of %d sources, %d destinations and in_feats %d'
                         % (h.shape[0], h.shape[1], K, S, layer._in_src_feats))
    _wait_block(block)
    ew = None
    if edge_weight is not None:
        ew = _bf16c(edge_weight.detach().reshape(-1))
        if ew.numel() != block.num_edges():
            raise ValueError('SAGEConv "gcn": %d edge weights for %d edges' % (ew.numel(), block.num_edges()))
    need_t = torch.is_grad_enabled() and (h.requires_grad or any(q.requires_grad for q in layer.parameters()))
    t_indptr, t_edge = block.transposed() if need_t else (None, None)      # (the backward's index; evaluation builds none)
    return _SageGcnTile.apply(h, layer.fc_neigh.weight, layer.bias, (block.indptr, block.src, block.dst, t_indptr, t_edge), ew, K, S,
                              _block_words(block), bool(relu), float(p), state if p > 0 else None, bool(want_norm))


# Full-neighbour inference of GraphConv(norm='both') straight off the graph's CSC (csrc/gcn_infer.hip): the
# batch-by-batch walk of GCN.inference without a block -- per-edge source norms of the batch structure, then a wave per row.
def _gcn_infer_args(indptr, indices, batch_size, row0, row1, edge0, n_edges, ns, what):
    V = indptr.numel() - 1
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or not (indptr.is_contiguous() and indices.is_contiguous()):
        raise ValueError("%s: the graph's CSC is int64 indptr / int32 indices, contiguous" % what)
    if not (indptr.is_cuda and indices.is_cuda):
        raise NotImplementedError("%s: the CSC inference path runs on the GPU" % what)
    if not (0 <= row0 <= row1 <= V) or batch_size < 1:
        raise ValueError("%s: rows %d .. %d of %d nodes, batch_size %d" % (what, row0, row1, V, batch_size))
    if n_edges >= 2 ** 31:
        raise NotImplementedError("%s: a range of 2^31 or more edges is beyond the CSC path" % what)
    if ns.dtype != torch.float32 or ns.numel() < n_edges or not ns.is_contiguous() or ns.device != indptr.device:
        raise ValueError("%s: ns is fp32 [%d] on %s" % (what, n_edges, indptr.device))
    t = _lib.GcnInfer()
    t.indptr, t.indices, t.n_nodes, t.batch_size = indptr.data_ptr(), indices.data_ptr(), V, int(batch_size)
    t.row0, t.n_rows, t.edge0, t.n_edges, t.ns = int(row0), int(row1) - int(row0), int(edge0), int(n_edges), ns.data_ptr()
    return t


def gcn_infer_state():
    """Scratch of ``gcn_infer_src_norms`` (the by-source sort of a range's edges); it grows with the largest range seen."""
    return dict(t_indptr=None, t_edge=None, temp=None)


def gcn_infer_src_norms(indptr, indices, batch_size, row0, row1, edge0, n_edges, ns, state=None):
    """``ns[e - edge0] = 1 / sqrt(max(cnt, 1))`` for the CSC positions of the destination rows ``row0 .. row1 - 1`` (whole
    batches of ``batch_size`` rows), ``cnt`` = the positions of e's batch that share e's source: the source norm GraphConv takes
    from the batch's full-neighbour block (bliss_gcn_infer_src_norms).  ``edge0`` / ``n_edges`` = indptr[row0] and the range's
    edge count as the host read them; ``ns`` fp32 [n_edges].  No host read."""
    import ctypes as C
    t = _gcn_infer_args(indptr, indices, batch_size, row0, row1, edge0, n_edges, ns, "gcn_infer_src_norms")
    if t.n_rows == 0 or t.n_edges == 0:
        return ns
    st = gcn_infer_state() if state is None else state
    dev, V = indptr.device, t.n_nodes
    nbytes = int(_lib.lib.bliss_block_transpose_temp_bytes(t.n_edges, V))
    if nbytes < 0:
        raise RuntimeError("bliss_block_transpose_temp_bytes failed")
    if st["t_indptr"] is None or st["t_indptr"].numel() < V + 1:
        st["t_indptr"] = torch.empty(V + 1, dtype=torch.int32, device=dev)
    if st["t_edge"] is None or st["t_edge"].numel() < t.n_edges:
        st["t_edge"] = torch.empty(t.n_edges, dtype=torch.int32, device=dev)
    if st["temp"] is None or st["temp"].numel() < nbytes:
        st["temp"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    t.t_indptr, t.t_edge, t.temp, t.temp_bytes = st["t_indptr"].data_ptr(), st["t_edge"].data_ptr(), st["temp"].data_ptr(), st["temp"].numel()
    _lib.check(_lib.lib.bliss_gcn_infer_src_norms(C.byref(t), _stream()), "bliss_gcn_infer_src_norms")
    return ns


def gcn_infer_spmm(indptr, indices, batch_size, row0, row1, edge0, n_edges, ns, h, out):
    """``out[r - row0] = bf16(nd_r * sum_e ns_e * h[indices[e]])`` for the rows ``row0 .. row1 - 1`` with the bits
    bliss_gcn_spmm_fwd gives on the full-neighbour block of every batch (bliss_gcn_infer_spmm).  ``h`` bf16 [V, dim] of ALL
    nodes; ``out`` bf16 [row1 - row0, dim] (a view of the layer's rows); ``ns`` from ``gcn_infer_src_norms`` on the same range."""
    import ctypes as C
    t = _gcn_infer_args(indptr, indices, batch_size, row0, row1, edge0, n_edges, ns, "gcn_infer_spmm")
    dev, dim = indptr.device, h.shape[1]
    if h.dtype != torch.bfloat16 or h.dim() != 2 or h.shape[0] < t.n_nodes or h.stride(1) != 1 or h.device != dev:
        raise ValueError("gcn_infer_spmm: h is bf16 [%d, dim] on %s" % (t.n_nodes, dev))
    if out.dtype != torch.bfloat16 or out.shape != (t.n_rows, dim) or (dim > 1 and out.stride(1) != 1) or out.device != dev:
        raise ValueError("gcn_infer_spmm: out is bf16 [%d, %d] on %s" % (t.n_rows, dim, dev))
    if t.n_rows == 0:
        return out
    t.h, t.h_stride, t.dim, t.out, t.out_stride = h.data_ptr(), h.stride(0), dim, out.data_ptr(), out.stride(0)
    _lib.check(_lib.lib.bliss_gcn_infer_spmm(C.byref(t), _stream()), "bliss_gcn_infer_spmm")
    return out


SAGE_INFER_REDUCE = {"mean": _lib.SAGE_INFER_MEAN, "max": _lib.SAGE_INFER_MAX}


def sage_infer_spmm(indptr, indices, batch_size, row0, row1, edge0, n_edges, h, out, reduce="mean"):
    """SAGEConv's full-neighbour message passing for the rows ``row0 .. row1 - 1`` (whole batches of ``batch_size`` rows) straight
    off the graph's CSC (bliss_sage_infer_spmm, csrc/sage_infer.hip), one launch:
    ``reduce="mean"``: ``out[r - row0] = bf16(1 / max(deg_r, 1) * sum_e h[indices[e]])`` with the bits ``weighted_aggregate(blk, x,
    None, mean=True)`` gives on the full-neighbour block of every batch; ``reduce="max"``: the column-wise maximum with the bits of
    ``max_aggregate(blk, x, None)``.  ``h`` bf16 [V, dim] of ALL nodes; ``out`` bf16 [row1 - row0, dim] (a view of the layer's
    rows); ``edge0`` / ``n_edges`` = indptr[row0] and the range's edge count as the host read them.  No host read."""
    import ctypes as C
    what = "sage_infer_spmm"
    if reduce not in SAGE_INFER_REDUCE:
        raise ValueError("%s: reduce must be one of %r, not %r" % (what, tuple(SAGE_INFER_REDUCE), reduce))
    V = indptr.numel() - 1
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or not (indptr.is_contiguous() and indices.is_contiguous()):
        raise ValueError("%s: the graph's CSC is int64 indptr / int32 indices, contiguous" % what)
    if not (indptr.is_cuda and indices.is_cuda):
        raise NotImplementedError("%s: the CSC inference path runs on the GPU" % what)
    if not (0 <= row0 <= row1 <= V) or batch_size < 1:
        raise ValueError("%s: rows %d .. %d of %d nodes, batch_size %d" % (what, row0, row1, V, batch_size))
    if n_edges >= 2 ** 31:
        raise NotImplementedError("%s: a range of 2^31 or more edges is beyond the CSC path" % what)
    dev, n_rows = indptr.device, int(row1) - int(row0)
    if h.dtype != torch.bfloat16 or h.dim() != 2 or h.shape[0] < V or h.stride(1) != 1 or h.device != dev:
        raise ValueError("%s: h is bf16 [%d, dim] on %s" % (what, V, dev))
    dim = h.shape[1]
    if out.dtype != torch.bfloat16 or out.shape != (n_rows, dim) or (dim > 1 and out.stride(1) != 1) or out.device != dev:
        raise ValueError("%s: out is bf16 [%d, %d] on %s" % (what, n_rows, dim, dev))
    if n_rows == 0:
        return out
    t = _lib.SageInfer()
    t.indptr, t.indices, t.n_nodes, t.batch_size = indptr.data_ptr(), indices.data_ptr(), V, int(batch_size)
    t.row0, t.n_rows, t.edge0, t.n_edges, t.reduce = int(row0), n_rows, int(edge0), int(n_edges), SAGE_INFER_REDUCE[reduce]
    t.h, t.h_stride, t.dim, t.out, t.out_stride = h.data_ptr(), h.stride(0), dim, out.data_ptr(), out.stride(0)
    _lib.check(_lib.lib.bliss_sage_infer_spmm(C.byref(t), _stream()), "bliss_sage_infer_spmm")
    return out


class GraphConv(nn.Module):
    """dglnn.GraphConv(in, out, norm='both', weight=True, bias=True) as built at model.py:397-417.

    [DGL-recalled] forward(graph, feat, edge_weight): feat_src * out_deg^-1/2 (degrees clamped to >= 1); weight first
    iff in > out; aggregate = update_all(u_mul_e('h','_edge_weight'), sum); then weight; * in_deg^-1/2; + bias;
    activation.  Degrees are the block's structural degrees (edge weights do not enter the normalisation).

    ``transforms="tile"`` runs the layer on the bounded kernels of csrc/gcn.hip and the MFMA entry
    points -- the path that runs under a batch capacity; ``"library"`` (the default) is the torch-op path with the launches and
    bits of before."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True, activation=None, allow_zero_in_degree=False,
                 transforms="library"):
        super().__init__()
        if norm != "both" or not weight:
            raise NotImplementedError("the reference only builds GraphConv(norm='both', weight=True)")
        if transforms not in GCN_TRANSFORMS:
            raise ValueError("transforms must be one of %r, not %r" % (GCN_TRANSFORMS, transforms))
        self.transforms = transforms
        self._in_feats, self._out_feats, self._activation = in_feats, out_feats, activation
        self._allow_zero_in_degree = allow_zero_in_degree
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats)) if bias else None
        nn.init.xavier_uniform_(self.weight)

    # -- transforms="tile"  -------------------------------------------------------------------------
    def _drop_state(self, device):
        st = getattr(self, "_dstate", None)
        if st is None or st["ctr"].device != device:
            st = self._dstate = gat_drop_state(getattr(self, "_drop_salt", 0), device)
        return st

    def tile_refusal(self, what="GraphConv"):
        """Why this layer cannot take the tile path, or None: the limits that do not depend on the input tensor."""
        wide = self.transforms == "wide"
        for name, n in (("in_feats", self._in_feats), ("out_feats", self._out_feats)):
            if wide and name == "in_feats":                # (out_feats is the k of _gcn_xwt and of the aggregate-first product)
                if n > TILE_WIDE_MAX_K:
                    return ('%s: transforms="wide" takes in_feats <= %d (the K-panelled MFMA kernels), this layer has %d; build it '
                            'with transforms="library"' % (what, TILE_WIDE_MAX_K, n))
            elif n > TILE_GEMM_MAX_K:
                return ('%s: transforms="%s" takes %s <= %d (the MFMA kernels keep a row tile\'s k columns in LDS), this layer has '
                        '%d; build it with transforms="library"' % (what, self.transforms, name, TILE_GEMM_MAX_K, n))
        if not (self._activation is None or _is_relu(self._activation)):
            return '%s: transforms="%s" covers the activations ReLU and None, not %r' % (what, self.transforms, self._activation)
        if not _mfma_bwd_on():
            return "%s: transforms=\"%s\" needs the MFMA backward (BLISS_SAGE_MFMA_BWD=0 is set)" % (what, self.transforms)
        ps = [self.weight] + ([self.bias] if self.bias is not None else [])
        if not all(q.is_cuda and q.dtype == torch.bfloat16 for q in ps):
            return '%s: transforms="%s" takes bf16 parameters on the GPU' % (what, self.transforms)
        return None

    def tile_forward(self, graph, feat, edge_weight=None, p=0.0, want_norm=False, what="GraphConv"):
        """The layer on the bounded kernels -> (out [n_dst, out_feats], its bf16 row norms or None).  ``p`` > 0: the keyed dropout
        of the model behind the layer's activation (the stream of this layer, ``_drop_state``).  Rows at or past the block's
        live destination count come out as zeros."""
        why = self.tile_refusal(what)
        if why is None and not (torch.is_tensor(feat) and feat.is_cuda and feat.dtype == torch.bfloat16 and feat.dim() == 2):
            why = '%s: transforms="%s" takes bf16 features [rows, in_feats] on the GPU' % (what, self.transforms)
        if why is not None:
            raise NotImplementedError(why)
        K, S = graph.num_src_nodes(), graph.num_dst_nodes()
        if feat.shape[0] < K or feat.shape[1] != self._in_feats:
            raise ValueError("%s: %d x %d input rows for a block of %d sources and in_feats %d" % (what, feat.shape[0], feat.shape[1], K, self._in_feats))
        _wait_block(graph)
        ew = None
        if edge_weight is not None:
            ew = _bf16c(edge_weight.detach().reshape(-1))
            if ew.numel() != graph.num_edges():
                raise ValueError("%s: %d edge weights for %d edges" % (what, ew.numel(), graph.num_edges()))
        t_indptr, t_edge = graph.transposed()                   # the norms need the by-source index, also in evaluation
        p = float(p)
        return _GcnLayer.apply(feat, self.weight, self.bias, (graph.indptr, graph.src, graph.dst, t_indptr, t_edge), ew, K, S,
                               _block_words(graph), self._activation is not None, p, self._drop_state(feat.device) if p > 0 else None,
                               bool(want_norm), self.transforms == "wide")

    # -- full-neighbour inference off the graph's CSC -------------------------------------------------
    def infer_refusal(self, h_all, what="GraphConv"):
        """Why ``infer_transform`` / ``infer_rows`` / ``infer_finish`` cannot run on these input rows, or None."""
        if not (torch.is_tensor(h_all) and h_all.is_cuda and h_all.dtype == torch.bfloat16 and h_all.dim() == 2):
            return "%s: the CSC inference path takes bf16 rows on the GPU, not %s on %s" % (what, h_all.dtype, h_all.device)
        if self.transforms not in TILE_KINDS:
            return ('%s: the CSC inference path has the bits of the bounded kernels; build the layer with transforms="tile" '
                    "(this one is %r)" % (what, self.transforms))
        return self.tile_refusal(what)

    def infer_transform(self, h_all):
        """The [V, dim] table the range SpMM gathers from: ``h W`` over ALL rows in one launch for a weight-first layer
        (bliss_gat_dgrad: a row's bits do not depend on how many rows the launch has), the input itself otherwise."""
        if self._in_feats > self._out_feats:
            return gat_dgrad(_bf16c(h_all), _bf16c(self.weight.detach()), h_all.shape[0], wide=self.transforms == "wide")
        return _bf16c(h_all)

    def infer_rows(self, g, batch_size, row0, row1, edge0, n_edges, ns, table, out):
        """The degree-normalised sums of the rows ``row0 .. row1 - 1`` (whole batches) into ``out`` (see ``gcn_infer_spmm``)."""
        return gcn_infer_spmm(g.indptr, g.indices, batch_size, row0, row1, edge0, n_edges, ns, table, out)

    def infer_finish(self, agg):
        """The finished rows of the layer in evaluation mode from the aggregated rows: the product with the weight for an
        aggregate-first layer, then the epilogue (bias, ReLU; no dropout, no row norms)."""
        import ctypes as C
        w = _bf16c(self.weight.detach())
        a = agg if self._in_feats > self._out_feats else gat_dgrad(agg, w, agg.shape[0])
        out = torch.empty(a.shape[0], w.shape[1], dtype=torch.bfloat16, device=a.device)
        t = _gcn_epilogue_args(a.shape[0], 0, w.shape[1], self._activation is not None, 0.0, None, None)
        t.a, t.a_stride, t.bias = a.data_ptr(), a.stride(0), 0 if self.bias is None else self.bias.data_ptr()
        t.out, t.out_stride = out.data_ptr(), out.stride(0)
        _lib.check(_lib.lib.bliss_gcn_epilogue_fwd(C.byref(t), _stream()), "bliss_gcn_epilogue_fwd")
        return out

    def forward(self, graph, feat, weight=None, edge_weight=None):
        if self.transforms in TILE_KINDS:
            if weight is not None:
                raise NotImplementedError('GraphConv: transforms="%s" multiplies by the layer\'s own weight' % self.transforms)
            return self.tile_forward(graph, feat, edge_weight)[0]
        n_dst = graph.num_dst_nodes()
        src, ones = graph.src, None
        if getattr(graph, "_nnz_ptr", 0) and getattr(graph, "_counts_dev", None) is not None:
            # capacity-padded (static-shape) block, round 3: only the first B edges exist (B on the device: LayerCounts::B); the
            # entries behind them are stale and must neither count nor index.  Padding rows have no edges: degree 0 -> clamp 1.
            valid = torch.arange(src.numel(), device=feat.device) < graph._counts_dev[4]
            src, ones = torch.where(valid, src, 0), valid.to(torch.int32)
        # (a fill kernel, not torch.zeros: memset nodes of a captured HIP graph were seen stale on replay)
        out_deg = torch.empty(graph.num_src_nodes(), dtype=torch.int32, device=feat.device).fill_(0)
        out_deg.index_add_(0, src, torch.ones_like(src) if ones is None else ones)
        norm_src = out_deg.clamp(min=1).to(feat.dtype).pow(-0.5)
        feat_src = feat * norm_src[:, None]
        w = self.weight
        if self._in_feats > self._out_feats:
            rst = weighted_aggregate(graph, feat_src @ w, edge_weight, mean=False)
        else:
            rst = weighted_aggregate(graph, feat_src, edge_weight, mean=False) @ w
        in_deg = (graph.indptr[1:n_dst + 1] - graph.indptr[:n_dst]).clamp(min=1).to(feat.dtype).pow(-0.5)
        rst = rst * in_deg[:, None]
        if self.bias is not None:
            rst = rst + self.bias
        if self._activation is not None:
            rst = self._activation(rst)
        return rst


# ------------------------------------------------------------------------------------------------ GATv2
def _nnz(block):
    return block._nnz_ptr, int(block.src.numel())


def _gat_partials(B, HD, device, floor):
    """The fp32 head / tail partials of the GAT kernels' balanced walk: two rows of HD per chunk of B edges, at least ``floor``
    floats (4 where a kernel reads the buffer in 16-byte pieces)."""
    n = 2 * (-(-B // _lib.lib.bliss_gat_chunk_edges())) * HD
    return torch.empty(max(n, floor), dtype=torch.float32, device=device)


class _GatLogits(torch.autograd.Function):
    """e[e,h] = attn[h,:] . leaky_relu(feat[src_e,h,:] + feat[dst_e,h,:])   (model.py:82-86)."""

    @staticmethod
    def forward(ctx, feat, attn, block, H, D, slope):
        feat, attn = feat.contiguous(), attn.reshape(-1).contiguous()
        nnz_ptr, B = _nnz(block)
        e = torch.empty(B, H, dtype=torch.bfloat16, device=feat.device)
        _lib.check(_lib.lib.bliss_gat_logits(block.src.data_ptr(), block.dst.data_ptr(), nnz_ptr, B, feat.data_ptr(), feat.stride(0),
                                             attn.data_ptr(), H, D, float(slope), e.data_ptr(), _stream()), "bliss_gat_logits")
        ctx.save_for_backward(feat, attn)
        ctx.block, ctx.H, ctx.D, ctx.slope = block, H, D, slope
        return e

    @staticmethod
    def backward(ctx, de):
        feat, attn = ctx.saved_tensors
        block, H, D, slope = ctx.block, ctx.H, ctx.D, ctx.slope
        de = de.contiguous().bfloat16()
        nnz_ptr, B = _nnz(block)
        K, S, HD = feat.shape[0], block.num_dst_nodes(), H * D
        part = _gat_partials(B, HD, feat.device, 1)
        d_attn = torch.zeros(HD, dtype=torch.float32, device=feat.device)
        d_el = torch.empty(K, HD, dtype=torch.bfloat16, device=feat.device)
        d_er = torch.empty(S, HD, dtype=torch.bfloat16, device=feat.device)
        t_indptr, t_edge = block.transposed()
        for which, rp, n_rows, out, da in ((3, t_indptr, K, d_el, 0), (2, block.indptr, S, d_er, d_attn.data_ptr())):
            _lib.check(_lib.lib.bliss_gat_rows(which, rp.data_ptr(), n_rows, t_edge.data_ptr(), block.src.data_ptr(),
                                               block.dst.data_ptr(), nnz_ptr, B, de.data_ptr(), feat.data_ptr(), feat.stride(0),
                                               attn.data_ptr(), H, D, float(slope), out.data_ptr(), out.stride(0),
                                               part.data_ptr(), da, _stream()), "bliss_gat_rows")
        d_feat = d_el
        d_feat[:S] += d_er                                  # shared weights: the destinations are the first S source rows
        return d_feat, d_attn.to(attn.dtype).view(1, H, D), None, None, None, None


class _EdgeSoftmax(torch.autograd.Function):
    """dglnn.functional.edge_softmax over the in-edges of every destination (model.py:88-90)."""

    @staticmethod
    def forward(ctx, e, block, H):
        e = e.contiguous()
        a = torch.empty_like(e)
        _lib.check(_lib.lib.bliss_gat_edge_softmax(block.indptr.data_ptr(), block.num_dst_nodes(), e.data_ptr(), 0, H, 0,
                                                   a.data_ptr(), _stream()), "bliss_gat_edge_softmax")
        ctx.save_for_backward(a)
        ctx.block, ctx.H = block, H
        return a

    @staticmethod
    def backward(ctx, da):
        (a,) = ctx.saved_tensors
        da = da.contiguous().bfloat16()
        de = torch.empty_like(a)
        _lib.check(_lib.lib.bliss_gat_edge_softmax(ctx.block.indptr.data_ptr(), ctx.block.num_dst_nodes(), da.data_ptr(),
                                                   a.data_ptr(), ctx.H, 1, de.data_ptr(), _stream()), "bliss_gat_edge_softmax")
        return de, None, None


class _GatAggregate(torch.autograd.Function):
    """out[i,h,:] = sum_{e -> i} a[e,h] * feat[src_e,h,:]   (update_all(u_mul_e('el','a'), sum), model.py:98)."""

    @staticmethod
    def forward(ctx, a, feat, block, H, D):
        a, feat = a.contiguous(), feat.contiguous()
        nnz_ptr, B = _nnz(block)
        S, HD = block.num_dst_nodes(), H * D
        out = torch.empty(S, HD, dtype=torch.bfloat16, device=feat.device)
        part = _gat_partials(B, HD, feat.device, 1)
        _lib.check(_lib.lib.bliss_gat_rows(0, block.indptr.data_ptr(), S, 0, block.src.data_ptr(), block.dst.data_ptr(), nnz_ptr, B,
                                           a.data_ptr(), feat.data_ptr(), feat.stride(0), 0, H, D, 0.0, out.data_ptr(),
                                           out.stride(0), part.data_ptr(), 0, _stream()), "bliss_gat_rows")
        ctx.save_for_backward(a, feat)
        ctx.block, ctx.H, ctx.D = block, H, D
        return out

    @staticmethod
    def backward(ctx, dout):
        a, feat = ctx.saved_tensors
        block, H, D = ctx.block, ctx.H, ctx.D
        dout = dout.contiguous().bfloat16()
        nnz_ptr, B = _nnz(block)
        K, HD = feat.shape[0], H * D
        da = torch.empty(B, H, dtype=torch.bfloat16, device=feat.device)
        _lib.check(_lib.lib.bliss_gat_edge_dot(block.src.data_ptr(), block.dst.data_ptr(), nnz_ptr, B, feat.data_ptr(), feat.stride(0),
                                               dout.data_ptr(), dout.stride(0), H, D, da.data_ptr(), _stream()), "bliss_gat_edge_dot")
        t_indptr, t_edge = block.transposed()
        d_feat = torch.empty(K, HD, dtype=torch.bfloat16, device=feat.device)
        part = _gat_partials(B, HD, feat.device, 1)
        _lib.check(_lib.lib.bliss_gat_rows(1, t_indptr.data_ptr(), K, t_edge.data_ptr(), block.src.data_ptr(), block.dst.data_ptr(),
                                           nnz_ptr, B, a.data_ptr(), dout.data_ptr(), dout.stride(0), 0, H, D, 0.0,
                                           d_feat.data_ptr(), d_feat.stride(0), part.data_ptr(), 0, _stream()), "bliss_gat_rows")
        return da, d_feat, None, None, None


def _gat_segments(block, S, B, state):
    """wg_row int32 [cap_wg, 4] (one descriptor per virtual workgroup), n_wg int32 [1] for ``block`` (bliss_gat_segments) and the per-row words the sharing workgroups
    meet on (zero-initialised once per layer and size; the kernels return them to zero)."""
    import ctypes as C
    dev = block.indptr.device
    cap_wg = S + B // int(_lib.lib.bliss_gat_segment_edges()) + 1
    if state["row_ws"] is None or state["row_ws"].numel() < S * 32:
        state["row_ws"] = torch.zeros(max(S, 1) * 32, dtype=torch.int32, device=dev)
    wg_row = torch.empty(cap_wg, 4, dtype=torch.int32, device=dev)
    n_wg = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.bliss_gat_segments(block.indptr.data_ptr(), S, cap_wg, wg_row.data_ptr(), n_wg.data_ptr(), state["err"].data_ptr(),
                                           _stream()), "bliss_gat_segments")
    return dict(wg_row=wg_row, n_wg=n_wg, cap_wg=cap_wg)


def _gat_fused_on(H, D):
    import os
    return os.environ.get("BLISS_GAT_FUSED", "1") != "0" and bool(_lib.lib.bliss_gat_fused_supported(int(H), int(D)))


class _GatFusedMP(torch.autograd.Function):
    """model.py:82-99 in ONE launch per direction and destination row (csrc/gat_fused.hip): (rst [S, H*D], e [B, H]) from
    feat = fc_src(h) and attn, attention dropout inside (model.py:88; counter-hash stream like the SAGE epilogue's -- the same
    Bernoulli(1-p)/scale law as nn.Dropout, not torch's Philox stream).  Backward: by destination in one launch pair (d a,
    softmax backward, d er, d attn), by source in one merge-style pass (logits + aggregation backward together)."""

    @staticmethod
    def forward(ctx, feat, attn, block, H, D, slope, p_drop, state):
        import ctypes as C
        ctx.set_materialize_grads(False)
        feat, attn_f = feat.contiguous(), attn.reshape(-1).contiguous()
        nnz_ptr, B = _nnz(block)
        S, HD, dev = block.num_dst_nodes(), H * D, feat.device
        e = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
        a = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
        ad = torch.empty(B, H, dtype=torch.bfloat16, device=dev) if p_drop > 0 else a
        rst = torch.empty(S, HD, dtype=torch.bfloat16, device=dev)
        t = _lib.GatFused()
        t.indptr, t.src, t.n_dst = block.indptr.data_ptr(), block.src.data_ptr(), S
        t.n_dst_dev = block._counts_dev.data_ptr() if (block._nnz_ptr and getattr(block, "_counts_dev", None) is not None) else 0
        t.feat, t.feat_stride, t.attn, t.heads, t.head_dim, t.negative_slope = feat.data_ptr(), feat.stride(0), attn_f.data_ptr(), H, D, float(slope)
        t.e, t.a, t.a_drop, t.rst, t.rst_stride = e.data_ptr(), a.data_ptr(), ad.data_ptr(), rst.data_ptr(), rst.stride(0)
        if p_drop > 0:
            t.drop_p, t.drop_seed, t.drop_ctr = float(p_drop), int(state["seed"]) & 0xFFFFFFFF, state["ctr"].data_ptr()
        # hub destinations are shared by several workgroups: virtual workgroup -> row map of THIS block (one small launch)
        seg = _gat_segments(block, S, B, state)
        seg_part = torch.empty(seg["cap_wg"] * (HD + 8), dtype=torch.float32, device=dev)
        t.wg_row, t.n_wg_dev, t.cap_wg = seg["wg_row"].data_ptr(), seg["n_wg"].data_ptr(), seg["cap_wg"]
        t.row_ws, t.seg_part, t.err = state["row_ws"].data_ptr(), seg_part.data_ptr(), state["err"].data_ptr()
        _lib.check(_lib.lib.bliss_gat_fused_fwd(C.byref(t), _stream()), "bliss_gat_fused_fwd")
        ctx.save_for_backward(feat, attn_f, a, ad, seg["wg_row"], seg["n_wg"])
        ctx.cap_wg = seg["cap_wg"]
        ctx.block, ctx.H, ctx.D, ctx.slope, ctx.p, ctx.state, ctx.n_dst_dev = block, H, D, float(slope), float(p_drop), state, t.n_dst_dev
        ctx.attn_shape, ctx.attn_dtype = attn.shape, attn.dtype
        return rst, e

    @staticmethod
    def backward(ctx, d_rst, _d_e):
        import ctypes as C
        feat, attn_f, a, ad, wg_row, n_wg = ctx.saved_tensors
        if _d_e is not None:
            raise NotImplementedError("the returned logits are the bandit's a_ij (model.py:224-227): nothing differentiates through them")
        if d_rst is None:
            return (None,) * 8
        block, H, D = ctx.block, ctx.H, ctx.D
        nnz_ptr, B = _nnz(block)
        K, S, HD, dev = feat.shape[0], block.num_dst_nodes(), H * D, feat.device
        g = d_rst.reshape(S, HD)
        g = (g if g.dtype == torch.bfloat16 else g.bfloat16()).contiguous()
        de = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
        d_er = torch.empty(S, HD, dtype=torch.bfloat16, device=dev)
        cap_wg = ctx.cap_wg
        dpart = torch.empty(cap_wg, HD, dtype=torch.float32, device=dev)
        bsum = torch.empty(-(-cap_wg // 32), HD, dtype=torch.float32, device=dev)
        seg_part = torch.empty(cap_wg * (HD + 8), dtype=torch.float32, device=dev)
        d_attn = torch.empty(HD, dtype=torch.float32, device=dev)
        t = _lib.GatFused()
        t.indptr, t.src, t.n_dst, t.n_dst_dev = block.indptr.data_ptr(), block.src.data_ptr(), S, ctx.n_dst_dev
        t.feat, t.feat_stride, t.attn, t.heads, t.head_dim, t.negative_slope = feat.data_ptr(), feat.stride(0), attn_f.data_ptr(), H, D, ctx.slope
        t.a, t.a_drop = a.data_ptr(), ad.data_ptr()
        t.drop_p = ctx.p
        t.g, t.g_stride, t.de, t.d_er, t.d_er_stride, t.dattn_part = g.data_ptr(), g.stride(0), de.data_ptr(), d_er.data_ptr(), d_er.stride(0), dpart.data_ptr()
        t.wg_row, t.n_wg_dev, t.cap_wg = wg_row.data_ptr(), n_wg.data_ptr(), cap_wg
        t.row_ws, t.seg_part, t.err = ctx.state["row_ws"].data_ptr(), seg_part.data_ptr(), ctx.state["err"].data_ptr()
        _lib.check(_lib.lib.bliss_gat_fused_bwd_dst(C.byref(t), bsum.data_ptr(), d_attn.data_ptr(), ctx.state["ticket"].data_ptr(), _stream()),
                   "bliss_gat_fused_bwd_dst")
        t_indptr, t_edge = block.transposed()
        d_feat = torch.empty(K, HD, dtype=torch.bfloat16, device=dev)
        part = _gat_partials(B, HD, dev, 4)
        _lib.check(_lib.lib.bliss_gat_rows_src_fused(t_indptr.data_ptr(), K, t_edge.data_ptr(), block.src.data_ptr(), block.dst.data_ptr(), nnz_ptr, B,
                                                     de.data_ptr(), ad.data_ptr(), feat.data_ptr(), feat.stride(0), g.data_ptr(), g.stride(0),
                                                     attn_f.data_ptr(), H, D, ctx.slope, d_feat.data_ptr(), d_feat.stride(0), part.data_ptr(),
                                                     _stream()), "bliss_gat_rows_src_fused")
        d_feat[:S] += d_er                                  # shared weights: the destinations are the first S source rows
        return d_feat, d_attn.to(ctx.attn_dtype).view(ctx.attn_shape), None, None, None, None, None, None


def gat_infer_state(device):
    """Scratch of ``gat_infer_layer``: the error word and the buffers that grow with the largest range seen."""
    return dict(err=torch.zeros(1, dtype=torch.int32, device=device), n_wg=torch.empty(1, dtype=torch.int32, device=device),
                wg_row=None, row_ws=None, seg_part=None)


def _gat_infer_refusal(feat, H, D, what="gat_infer_layer"):
    """Why the CSC inference kernel cannot take these rows, or None."""
    if not (feat.is_cuda and feat.dtype == torch.bfloat16):
        return "%s: the CSC inference path takes bf16 rows on the GPU, not %s on %s" % (what, feat.dtype, feat.device)
    if not _gat_fused_on(H, D):
        return ("%s: the CSC inference path runs on the fused message-passing kernel (bliss_gat_fused_supported(%d, %d) is false "
                "or BLISS_GAT_FUSED=0)" % (what, H, D))
    return None


def gat_infer_layer(indptr, indices, row0, row1, n_edges, feat, attn, H, D, slope, out, res=None, act=0, state=None):
    """model.py:82-106 for the destinations ``row0 .. row1 - 1`` of the WHOLE graph in one launch pair (bliss_gat_infer_fwd,
    DESIGN.md section 23): ``out[r - row0] = act(rst_r + res[r - row0])`` with ``rst`` the fused kernel's bits on the range's
    full-neighbour block, read straight off the graph's int64 ``indptr`` / int32 ``indices``.  ``feat`` = fc_src(h) of ALL nodes
    [V, H*D]; ``res`` the range's residual rows or None; ``out`` [row1 - row0, H*D] bf16 (a view of the layer's rows);
    ``n_edges`` = indptr[row1] - indptr[row0] as the host read it (below 2^31).  ``state`` (``gat_infer_state``) owns the
    scratch and regrows it by range; no host read, nothing of edge size allocated."""
    import ctypes as C
    why = _gat_infer_refusal(feat, H, D)
    if why is not None:
        raise NotImplementedError(why)
    n_rows, HD, dev = int(row1) - int(row0), H * D, feat.device
    V = indptr.numel() - 1
    if not (0 <= row0 <= row1 <= V) or feat.shape[0] < V or feat.shape[1] != HD or feat.stride(1) != 1:
        raise ValueError("gat_infer_layer: rows %d .. %d of %d nodes, feat %r for H*D = %d" % (row0, row1, V, tuple(feat.shape), HD))
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or not (indptr.is_contiguous() and indices.is_contiguous()):
        raise ValueError("gat_infer_layer: the graph's CSC is int64 indptr / int32 indices, contiguous")
    if out.dtype != torch.bfloat16 or out.shape != (n_rows, HD) or out.stride(1) != 1 or out.device != dev:
        raise ValueError("gat_infer_layer: out is bf16 [%d, %d] on %s" % (n_rows, HD, dev))
    if res is not None and (res.dtype != torch.bfloat16 or res.shape != (n_rows, HD) or res.stride(1) != 1 or res.device != dev):
        raise ValueError("gat_infer_layer: res is bf16 [%d, %d] on %s" % (n_rows, HD, dev))
    if n_rows == 0:
        return out
    st = gat_infer_state(dev) if state is None else state
    cap_wg = n_rows + int(n_edges) // int(_lib.lib.bliss_gat_segment_edges())
    if st["wg_row"] is None or st["wg_row"].shape[0] < cap_wg:
        st["wg_row"] = torch.empty(cap_wg, 4, dtype=torch.int32, device=dev)
    if st["seg_part"] is None or st["seg_part"].numel() < cap_wg * HD:
        st["seg_part"] = torch.empty(cap_wg * HD, dtype=torch.float32, device=dev)
    if st["row_ws"] is None or st["row_ws"].numel() < n_rows * 32:
        st["row_ws"] = torch.zeros(n_rows * 32, dtype=torch.int32, device=dev)        # (zero once: the kernel returns it to zero)
    attn_f = attn.detach().reshape(-1).contiguous()
    t = _lib.GatInfer()
    t.indptr, t.indices, t.row0, t.n_rows, t.n_edges = indptr.data_ptr(), indices.data_ptr(), int(row0), n_rows, int(n_edges)
    t.feat, t.feat_stride, t.attn, t.heads, t.head_dim, t.negative_slope = feat.data_ptr(), feat.stride(0), attn_f.data_ptr(), H, D, float(slope)
    if res is not None:
        t.res, t.res_stride = res.data_ptr(), res.stride(0)
    t.act, t.out, t.out_stride = int(act), out.data_ptr(), out.stride(0)
    t.wg_row, t.n_wg_dev, t.cap_wg = st["wg_row"].data_ptr(), st["n_wg"].data_ptr(), cap_wg
    t.row_ws, t.seg_part, t.err = st["row_ws"].data_ptr(), st["seg_part"].data_ptr(), st["err"].data_ptr()
    _lib.check(_lib.lib.bliss_gat_infer_fwd(C.byref(t), _stream()), "bliss_gat_infer_fwd")
    return out


# ------------------------------------------------------------------------------------------------ GATv2 on bounded kernels
# transforms="tile" (DESIGN.md section 22): fc_src / res_fc on the MFMA tile kernels, the glue around the message passing in one
# launch per direction (csrc/gat_glue.hip) -- every loop that crosses rows is bounded by the block's device-side counts, so the
# layers run on a capacity-padded output block (train.GraphedTrainStep(batch_capacity=...)).
# transforms="wide" (DESIGN.md section 29): "tile" with in_feats up to TILE_WIDE_MAX_K (fc_src / res_fc of a wide input layer on
# bliss_tile_gemm_wide); a layer within 1024 has the launches and bits of "tile".
GAT_TRANSFORMS = ("library", "tile", "wide")


def _block_words(block):
    """Addresses of the block's live (S, K, B) words for the kernels' ``*_dev`` arguments; (0, 0, 0) for an exact-size block."""
    if block._nnz_ptr and getattr(block, "_counts_dev", None) is not None:
        cd = block._counts_dev.data_ptr()
        return cd, cd + 12, cd + 16
    return 0, 0, 0


def _col_blocks(n):
    return [(c, min(n, c + TILE_GEMM_MAX_N)) for c in range(0, n, TILE_GEMM_MAX_N)]


def _dgrad_fits(k1, k2):
    """Do both staged operands and a W slab of bliss_gat_dgrad fit a workgroup's 160 KiB of LDS (csrc/sage_bwd.hip)?"""
    st = lambda k: (((k + 15) & ~15) + 8) if k else 0
    return 2 * (32 * (st(k1) + st(k2)) + 64 * (256 + 32)) <= 160 * 1024


def gat_dgrad(a1, w1, m_bound, m_dev=0, a2=None, w2=None, m2_bound=0, m2_dev=0, wide=False):
    """sage_dgrad for gradient rows of up to 1024 columns (bliss_gat_dgrad): out[r] = a1[r] @ w1 (+ a2[r] @ w2 for r < m2), fp32
    accumulation over all of it, one rounding; zero rows at or past the counts.  ``wide``: rows of more than 1024 columns (up
    to TILE_WIDE_MAX_K) go to bliss_dgrad_wide; a product within 1024 stays on bliss_gat_dgrad, wide or not."""
    import ctypes as C
    out = torch.empty(m_bound, w1.shape[1], dtype=torch.bfloat16, device=a1.device)
    t = _lib.DGrad()
    t.a1, t.a1_stride, t.w1, t.w1_stride, t.k1 = a1.data_ptr(), a1.stride(0), w1.data_ptr(), w1.stride(0), w1.shape[0]
    if a2 is not None:
        t.a2, t.a2_stride, t.w2, t.w2_stride, t.k2 = a2.data_ptr(), a2.stride(0), w2.data_ptr(), w2.stride(0), w2.shape[0]
        t.m2_bound, t.m2_dev = int(m2_bound), int(m2_dev)
    t.m_bound, t.m_dev, t.n = int(m_bound), int(m_dev), w1.shape[1]
    t.out, t.out_stride = out.data_ptr(), out.stride(0)
    if wide and max(t.k1, t.k2) > TILE_GEMM_MAX_K:
        _lib.check(_lib.lib.bliss_dgrad_wide(C.byref(t), _stream()), "bliss_dgrad_wide")
        return out
    _lib.check(_lib.lib.bliss_gat_dgrad(C.byref(t), _stream()), "bliss_gat_dgrad")
    return out


def _zero_rows(n, like):
    # (a fill kernel, not torch.zeros: memset nodes of a captured HIP graph were seen stale on replay)
    return torch.empty(n, like.shape[1], dtype=like.dtype, device=like.device).fill_(0)


def _wgrad_blocks(problems):
    """[(d [R, N], x [R, k_in], rows_bound, rows_dev, want_bias)] -> [(dW [N, k_in], db or None)] for N of any size: one
    bliss_sage_wgrad problem per block of 256 output rows (a column slice of d, a row slice of dW), two problems per launch."""
    import ctypes as C
    outs, recs = [], []
    for d, x, rb, rdev, want_b in problems:
        dw = torch.empty(d.shape[1], x.shape[1], dtype=torch.bfloat16, device=d.device)
        db = torch.empty(d.shape[1], dtype=torch.bfloat16, device=d.device) if want_b else None
        outs.append((dw, db))
        for c0, c1 in _col_blocks(d.shape[1]):
            recs.append((d[:, c0:c1], x, rb, rdev, dw[c0:c1], None if db is None else db[c0:c1]))
    for i in range(0, len(recs), 2):
        pair = recs[i:i + 2]
        arr = (_lib.WGrad * len(pair))()
        for a, (d, x, rb, rdev, dw, db) in zip(arr, pair):
            a.d, a.d_stride, a.n_out = d.data_ptr(), d.stride(0), d.shape[1]
            a.x, a.x_stride, a.k_in = x.data_ptr(), x.stride(0), x.shape[1]
            a.rows_bound, a.rows_dev = int(rb), int(rdev)
            a.dw, a.dw_stride, a.db = dw.data_ptr(), dw.stride(0), 0 if db is None else db.data_ptr()
        need = int(_lib.lib.bliss_sage_wgrad_workspace(arr, len(pair)))
        if need < 0:
            raise RuntimeError("bliss_sage_wgrad: invalid problem description")
        ws = torch.empty(max(need, 4), dtype=torch.float32, device=pair[0][0].device)
        _lib.check(_lib.lib.bliss_sage_wgrad(arr, len(pair), ws.data_ptr(), ws.numel(), _stream()), "bliss_sage_wgrad")
    return outs


class _GatLinear(torch.autograd.Function):
    """y1 = x[:n1] @ w1^T (+ b1) and, with a second weight, y2 = x[:n2] @ w2^T (+ b2), n2 <= n1 -- fc_src over a block's source
    rows and res_fc over its destination rows (model.py:66-72, :101-103) -- on bliss_tile_gemm in output-column blocks of at most
    256 (a row slice of W, an offset ``out`` pointer with the full row stride), two blocks per launch.  ``dev1`` / ``dev2``: the
    block's live row words (0: the bounds are exact); rows at or past them come out as zeros.  Backward: the weight (and bias)
    gradients on bliss_sage_wgrad, one problem per column block; the input gradient on bliss_gat_dgrad (both Linears into one
    fp32 accumulator when they fit)."""

    @staticmethod
    def forward(ctx, x, w1, b1, n1, dev1, w2, b2, n2, dev2, wide=False):
        ctx.set_materialize_grads(False)
        x, w1 = _bf16c(x), _bf16c(w1)
        w2 = None if w2 is None else _bf16c(w2)
        k_max = TILE_WIDE_MAX_K if wide else TILE_GEMM_MAX_K
        if x.shape[1] > k_max or x.shape[0] < n1 or (w2 is not None and n2 > n1):
            raise ValueError("_GatLinear: in_feats <= %d, n2 <= n1 <= rows" % k_max)
        y1 = torch.empty(n1, w1.shape[0], dtype=torch.bfloat16, device=x.device)
        y2 = None if w2 is None else torch.empty(n2, w2.shape[0], dtype=torch.bfloat16, device=x.device)
        sets = [_tg_args(x, w1[c0:c1], y1[:, c0:c1], n1, bias=None if b1 is None else b1[c0:c1], m_dev=dev1) for c0, c1 in _col_blocks(w1.shape[0])]
        if w2 is not None:
            sets += [_tg_args(x, w2[c0:c1], y2[:, c0:c1], n2, bias=None if b2 is None else b2[c0:c1], m_dev=dev2) for c0, c1 in _col_blocks(w2.shape[0])]
        for i in range(0, len(sets), 2):
            _tile_gemm(sets[i], sets[i + 1] if i + 1 < len(sets) else None, wide=wide)
        ctx.save_for_backward(x, w1, w2)
        ctx.n1, ctx.dev1, ctx.n2, ctx.dev2, ctx.has_b1, ctx.has_b2 = n1, dev1, n2, dev2, b1 is not None, b2 is not None
        return y1, y2

    @staticmethod
    def backward(ctx, d1, d2):
        x, w1, w2 = ctx.saved_tensors
        d1 = None if d1 is None else _bf16c(d1)
        d2 = None if (d2 is None or w2 is None) else _bf16c(d2)
        probs = []
        if d1 is not None:
            probs.append((d1, x, ctx.n1, ctx.dev1, ctx.has_b1))
        if d2 is not None:
            probs.append((d2, x, ctx.n2, ctx.dev2, ctx.has_b2))
        outs = _wgrad_blocks(probs) if probs else []
        dw1, db1 = outs[0] if d1 is not None else (None, None)
        dw2, db2 = outs[-1] if d2 is not None else (None, None)
        dx = None
        if ctx.needs_input_grad[0] and probs:
            if d1 is not None and d2 is not None and _dgrad_fits(w1.shape[0], w2.shape[0]):
                dx = gat_dgrad(d1, w1, ctx.n1, ctx.dev1, a2=d2, w2=w2, m2_bound=ctx.n2, m2_dev=ctx.dev2)
            else:
                dx = gat_dgrad(d1, w1, ctx.n1, ctx.dev1) if d1 is not None else None
                if d2 is not None:
                    dx2 = gat_dgrad(d2, w2, ctx.n2, ctx.dev2)                # (zero rows at or past the count)
                    if dx is None:
                        dx = torch.cat([dx2, _zero_rows(ctx.n1 - ctx.n2, dx2)])
                    else:
                        dx[: ctx.n2] += dx2
            if x.shape[0] > ctx.n1:
                dx = torch.cat([dx, _zero_rows(x.shape[0] - ctx.n1, dx)])
        return dx, dw1, db1, None, None, dw2, db2, None, None, None


def gat_linear(x, w, b, n_rows, rows_dev=0, w2=None, b2=None, n2_rows=0, rows2_dev=0, wide=False):
    """``_GatLinear``: (x[:n_rows] @ w^T + b, x[:n2_rows] @ w2^T + b2 or None).  ``wide``: in_feats up to TILE_WIDE_MAX_K."""
    return _GatLinear.apply(x, w, b, int(n_rows), int(rows_dev), w2, b2, int(n2_rows), int(rows2_dev), bool(wide))


# ------------------------------------------------------------------------------------------------ SAGEConv 'pool' on the tile kernels
# transforms="tile" (DESIGN.md section 32): relu(fc_pool(h)) on bliss_tile_gemm, the max-reduce of csrc/spmm_max.hip, the layer's
# tail (fc_neigh + fc_self + bias, ReLU, dropout, row norms) in one launch; the backward's ReLU mask of fc_pool inside the routed
# max backward (bliss_spmm_max_bwd_relu).  Every row and edge loop is bounded by the block's device-side counts.
def _tile_gemm_fits(k1, k2=0, n=TILE_GEMM_MAX_N):
    """Does one argument set of bliss_tile_gemm fit a workgroup's 160 KiB of LDS?  The size formula of csrc/sage.hip (convert):
    32 staged rows of each operand at stride round16(k) + 8, a 256 x 72 slab of W, or the output tile, whichever is larger."""
    st = lambda k: (((k + 15) & ~15) + 8) if k else 0
    stage = 2 * (32 * (st(k1) + st(k2)) + 256 * (64 + 8))
    outt = 2 * 32 * (((n + 63) & ~63) + 8)
    return max(stage, outt) <= 160 * 1024


def _tile_gemm_by_size(first, second=None):
    """One launch on bliss_tile_gemm, or -- where a set's operands pass its LDS -- on bliss_tile_gemm_wide, which stages one operand
    panel at a time and returns bliss_tile_gemm's bits at k <= 1024.  Decided from the size formula, never by trying the call."""
    import ctypes as C
    sets = [first] + ([] if second is None else [second])
    wide = not all(_tile_gemm_fits(t.k1, t.k2, t.n) for t in sets)
    name = "bliss_tile_gemm_wide" if wide else "bliss_tile_gemm"
    _lib.check(getattr(_lib.lib, name)(C.byref(first), None if second is None else C.byref(second), _stream()), name)
    return name


class _SagePoolTile(torch.autograd.Function):
    """A SAGEConv('pool') layer with its tail on a block, ONE autograd node:

        pooled = relu(fc_pool(h))                      bliss_tile_gemm, output-column blocks of <= 256, two per launch, rows < K
        neigh, arg = max_{e -> i} bf16(w_e pooled[src_e])   bliss_spmm_max_fwd, edges < B
        out = dropout_p(relu(fc_neigh(neigh) + fc_self(h[:S]) + bias))   one launch, rows < S (the last layer: no ReLU, p = 0)

    K, S, B the block's live counts (its device words when it is capacity-padded).  With ``ids`` the rows of ``x`` are gathered by
    the first launch, which also writes them out for the later launches and the backward.  Returns (out, out_norm, in_norm); the
    norms have the bits of ops.embed_norm.  Backward: the epilogue's mask, dW_neigh / dW_self / db_self in one launch pair,
    d_neigh = d W_neigh, d_z = the routed max backward under the mask pooled > 0 (no element-wise torch op), dW_pool / db_pool in
    column blocks, dh = d_z W_pool + d W_self on the first S rows in one accumulator.  ``dbg``: a dict that receives pooled, neigh,
    arg, out, the entry point of the tail and (backward) d, d_neigh, d_z -- the stage-by-stage tests read it; None in use."""

    @staticmethod
    def forward(ctx, x, ids, w_pool, b_pool, w_neigh, w_self, b_self, blk, relu, p, ctr, seed, dbg):
        from . import ops
        ctx.set_materialize_grads(False)
        _dropout_needs_relu(relu, p)
        indptr, src, dst, w, counts, t_indptr, t_edge, K, S, src_dev, dst_dev = blk
        x, wp, wn, ws = _bf16c(x), _bf16c(w_pool), _bf16c(w_neigh), _bf16c(w_self)
        fin, fout, dev = wp.shape[1], wn.shape[0], x.device
        gathered = ids is not None
        if x.shape[1] != fin or (not gathered and x.shape[0] < K) or S > K:
            raise ValueError("_SagePoolTile: x [>= K, in_feats], S <= K")
        rows = torch.empty(K, fin, dtype=torch.bfloat16, device=dev) if gathered else x
        pooled = torch.empty(K, fin, dtype=torch.bfloat16, device=dev)
        in_norm = torch.empty(K, dtype=torch.bfloat16, device=dev)
        sets = []
        for i, (c0, c1) in enumerate(_col_blocks(fin)):
            # the first launch reads the table itself (its second block gathers again: the copy is still being written beside it)
            a, a_ids = (x, ids) if i < 2 else (rows, None)
            sets.append(_tg_args(a, wp[c0:c1], pooled[:, c0:c1], K, ids=a_ids, bias=None if b_pool is None else b_pool[c0:c1], m_dev=src_dev,
                                 a_copy=rows if (gathered and i == 0) else None, in_norm=in_norm if i == 0 else None, relu=True))
        for i in range(0, len(sets), 2):
            _tile_gemm(sets[i], sets[i + 1] if i + 1 < len(sets) else None)
        neigh, arg = ops.spmm_max(indptr, src, dst, w, pooled, S, counts, True, None, None)
        out = torch.empty(S, fout, dtype=torch.bfloat16, device=dev)
        out_norm = torch.empty(S, dtype=torch.bfloat16, device=dev)
        entry = _tile_gemm_by_size(_tg_args(neigh, wn, out, S, a2=rows, w2=ws, bias=b_self, m_dev=dst_dev, out_norm=out_norm, relu=relu, p=p,
                                            seed=seed, ctr=ctr))
        ctx.save_for_backward(rows, pooled, neigh, arg, out, wp, wn, ws, indptr, src, dst, w, counts, t_indptr, t_edge)
        ctx.relu, ctx.p, ctx.has_bp, ctx.has_bs, ctx.gathered, ctx.x_rows = bool(relu), float(p), b_pool is not None, b_self is not None, gathered, x.shape[0]
        ctx.K, ctx.S, ctx.src_dev, ctx.dst_dev, ctx.dbg = K, S, src_dev, dst_dev, dbg
        if dbg is not None:
            dbg.update(pooled=pooled, neigh=neigh, arg=arg, out=out, rows=rows, tail_entry=entry)
        ctx.mark_non_differentiable(out_norm, in_norm)
        return out, out_norm, in_norm

    @staticmethod
    def backward(ctx, dout, _dn1, _dn2):
        from . import ops
        rows, pooled, neigh, arg, out, wp, wn, ws, indptr, src, dst, w, counts, t_indptr, t_edge = ctx.saved_tensors
        if dout is None:
            return (None,) * 13
        K, S, src_dev, dst_dev = ctx.K, ctx.S, ctx.src_dev, ctx.dst_dev
        d = _bf16c(dout)
        if ctx.relu or ctx.p > 0:
            din = torch.empty_like(out)
            _lib.check(_lib.lib.bliss_sage_epilogue_bwd(d.data_ptr(), d.stride(0), out.data_ptr(), out.stride(0), out.shape[0],
                                                        out.shape[1], ctx.p, din.data_ptr(), din.stride(0), _stream()),
                       "bliss_sage_epilogue_bwd")
            d = din
        (d_wn, _), (d_ws, d_bs) = sage_wgrad([(d, neigh, S, dst_dev, False), (d, rows, S, dst_dev, ctx.has_bs)])
        want_dx = ctx.needs_input_grad[0] and not ctx.gathered
        d_wp = d_bp = dx = d_neigh = d_z = None
        if want_dx or ctx.needs_input_grad[2] or (ctx.has_bp and ctx.needs_input_grad[3]):
            if t_indptr is None or t_edge is None:
                raise RuntimeError("the block's by-source index (Block.transposed()) is needed to differentiate through fc_pool")
            d_neigh = sage_dgrad(d, wn, S, dst_dev)
            d_z = ops.spmm_max_t_relu(t_indptr, t_edge, src, dst, w, d_neigh, arg, pooled, K, counts)
            ((d_wp, d_bp),) = _wgrad_blocks([(d_z, rows, K, src_dev, ctx.has_bp)])
            if want_dx:
                fin, fout = wp.shape[0], ws.shape[0]
                if _dgrad_fits(fin, fout):
                    dx = gat_dgrad(d_z, wp, K, src_dev, a2=d, w2=ws, m2_bound=S, m2_dev=dst_dev)
                else:
                    dx = gat_dgrad(d_z, wp, K, src_dev)
                    dx[:S] += gat_dgrad(d, ws, S, dst_dev)                  # (zero rows at or past the count)
                if ctx.x_rows > K:
                    dx = torch.cat([dx, _zero_rows(ctx.x_rows - K, dx)])
        if ctx.dbg is not None:
            ctx.dbg.update(d=d, d_neigh=d_neigh, d_z=d_z)
        return dx, None, d_wp, d_bp, d_wn, d_ws, d_bs, None, None, None, None, None, None


def sage_pool_tile(block, h, edge_weight, layer, relu, p, ctr, seed, dbg=None):
    """``layer`` = SAGEConv(in, out, 'pool') on ``block`` through _SagePoolTile: (out, out_norm, in_norm).  ``h``: the layer's input
    rows, a bf16 tensor on the GPU or a LazyRows (gathered by the first launch)."""
    assert h.is_cuda and h.dtype == torch.bfloat16, "bf16 features on the GPU (load_graph.py:7)"
    _wait_block(block)
    w = None
    if edge_weight is not None:
        w = edge_weight.reshape(-1)
        w = (w if w.dtype == torch.bfloat16 else w.bfloat16()).contiguous()
    dst_dev, src_dev, _ = _block_words(block)
    counts = block._counts_dev if dst_dev else None
    table, ids = (h.table, h.ids) if isinstance(h, LazyRows) else (h, None)
    fp = layer.fc_pool
    need_t = torch.is_grad_enabled() and ((ids is None and h.requires_grad) or fp.weight.requires_grad or fp.bias.requires_grad)
    t_indptr, t_edge = block.transposed() if need_t else (None, None)
    blk = (block.indptr, block.src, block.dst, w, counts, t_indptr, t_edge, block.num_src_nodes(), block.num_dst_nodes(), src_dev, dst_dev)
    return _SagePoolTile.apply(table, ids, fp.weight, fp.bias, layer.fc_neigh.weight, layer.fc_self.weight, layer.fc_self.bias, blk,
                               bool(relu), float(p), ctr, int(seed), dbg)


def gat_drop_state(salt, device):
    """The feat_drop stream of one GATv2 layer: its launch counter (device uint64[2]) and seed -- a function of torch's CUDA seed
    and of the layer's ordinal, like the attention dropout's (GATv2Conv._fused_state)."""
    return dict(ctr=torch.zeros(2, dtype=torch.int64, device=device),
                seed=(torch.cuda.initial_seed() ^ (0x85EBCA77 * (int(salt) + 1))) & 0xFFFFFFFF)


def _glue_args(H, D, act, head_mean, p, n_rows, rows_dev, state, ctr_used):
    t = _lib.GatGlue()
    t.n_rows, t.n_rows_dev, t.heads, t.head_dim, t.act, t.head_mean = int(n_rows), int(rows_dev), int(H), int(D), int(act), int(bool(head_mean))
    if p > 0:
        t.drop_p, t.drop_seed, t.drop_ctr, t.drop_ctr_used = float(p), int(state["seed"]) & 0xFFFFFFFF, state["ctr"].data_ptr(), ctr_used.data_ptr()
    return t


class _GatGlue(torch.autograd.Function):
    """csrc/gat_glue.hip: out = dropout_p(flatten-or-head-mean(act(rst (+ res)))) over the rows below the live count, zeros past
    it; ``pre`` (with ``want_pre``) is the value before the dropout, for the row norms the next layer stores."""

    @staticmethod
    def forward(ctx, rst, res, H, D, act, head_mean, p, state, n_rows, rows_dev, want_pre):
        import ctypes as C
        ctx.set_materialize_grads(False)
        rst = _bf16c(rst)
        res = None if res is None else _bf16c(res)
        HD, dev = H * D, rst.device
        if rst.dim() != 2 or rst.shape[1] != HD or rst.shape[0] < n_rows or (res is not None and (res.shape[1] != HD or res.shape[0] < n_rows)):
            raise ValueError("gat_glue: rst (and res) are [rows >= n_rows, heads * head_dim]")
        width = D if head_mean else HD
        out = torch.empty(n_rows, width, dtype=torch.bfloat16, device=dev)
        pre = torch.empty(n_rows, width, dtype=torch.bfloat16, device=dev) if (want_pre and p > 0) else None
        ctr_used = torch.empty(1, dtype=torch.int32, device=dev) if p > 0 else None
        t = _glue_args(H, D, act, head_mean, p, n_rows, rows_dev, state, ctr_used)
        t.rst, t.rst_stride = rst.data_ptr(), rst.stride(0)
        if res is not None:
            t.res, t.res_stride = res.data_ptr(), res.stride(0)
        t.out, t.out_stride = out.data_ptr(), out.stride(0)
        if pre is not None:
            t.pre, t.pre_stride = pre.data_ptr(), pre.stride(0)
        _lib.check(_lib.lib.bliss_gat_glue_fwd(C.byref(t), _stream()), "bliss_gat_glue_fwd")
        ctx.save_for_backward(rst if act else None, res if act else None, ctr_used)
        ctx.cfg = (H, D, act, head_mean, float(p), state, n_rows, rows_dev, res is not None)
        if pre is not None:
            ctx.mark_non_differentiable(pre)
        return out, pre

    @staticmethod
    def backward(ctx, dout, _dpre):
        import ctypes as C
        rst, res, ctr_used = ctx.saved_tensors
        H, D, act, head_mean, p, state, n_rows, rows_dev, has_res = ctx.cfg
        if dout is None:
            return (None,) * 11
        dout = _bf16c(dout)
        din = torch.empty(n_rows, H * D, dtype=torch.bfloat16, device=dout.device)
        t = _glue_args(H, D, act, head_mean, p, n_rows, rows_dev, state, ctr_used)
        if act:
            t.rst, t.rst_stride = rst.data_ptr(), rst.stride(0)
            if res is not None:
                t.res, t.res_stride = res.data_ptr(), res.stride(0)
        t.dout, t.dout_stride, t.din, t.din_stride = dout.data_ptr(), dout.stride(0), din.data_ptr(), din.stride(0)
        _lib.check(_lib.lib.bliss_gat_glue_bwd(C.byref(t), _stream()), "bliss_gat_glue_bwd")
        return (din, din if has_res else None) + (None,) * 9


GLUE_ACT_NONE, GLUE_ACT_ELU = 0, 1


def gat_glue(rst, res, heads, head_dim, act=GLUE_ACT_NONE, head_mean=False, p=0.0, state=None, n_rows=None, rows_dev=0, want_pre=False):
    """The glue behind a GATv2 layer's message passing (see ``_GatGlue``) -> (out, pre or None)."""
    n_rows = rst.shape[0] if n_rows is None else int(n_rows)
    if p > 0 and state is None:
        raise ValueError("gat_glue: dropout needs the stream's state (gat_drop_state)")
    out, pre = _GatGlue.apply(rst, res, int(heads), int(head_dim), int(act), bool(head_mean), float(p), state, n_rows, int(rows_dev), bool(want_pre))
    return out, (out.detach() if (want_pre and pre is None) else pre)


def gat_feat_drop(x, p, state, n_rows=None, rows_dev=0):
    """feat_drop (model.py:66) on the rows below the live count with the keyed mask; zeros past it."""
    return gat_glue(x, None, 1, x.shape[1], p=p, state=state, n_rows=n_rows, rows_dev=rows_dev)[0]


def gat_head_mean(e, n_edges=None, edges_dev=0):
    """a_ij = e.mean(1) (model.py:224-227) over the live edges: bf16 [B]; entries past the count are left as allocated."""
    e = _bf16c(e.detach())
    B, H = (e.shape[0] if n_edges is None else int(n_edges)), e.shape[1]
    out = torch.empty(B, dtype=torch.bfloat16, device=e.device)
    _lib.check(_lib.lib.bliss_gat_head_mean(e.data_ptr(), H, B, int(edges_dev), out.data_ptr(), _stream()), "bliss_gat_head_mean")
    return out


def _glue_act(act, what):
    if act is None:
        return GLUE_ACT_NONE
    if act is torch.nn.functional.elu or (isinstance(act, nn.ELU) and float(act.alpha) == 1.0):
        return GLUE_ACT_ELU
    raise NotImplementedError('%s: transforms="tile" covers the activations ELU (alpha 1) and None, not %r' % (what, act))


def edge_softmax(graph, logits):
    """``dglnn.functional.edge_softmax(graph, e)`` (model.py:88-90): softmax over the in-edges of every destination,
    per head; ``logits`` [B, H, 1] (or [B, H])."""
    shape = logits.shape
    H = shape[1] if logits.dim() > 1 else 1
    return _EdgeSoftmax.apply(logits.reshape(shape[0], H), graph, H).view(shape)


def gat_forward_f32(graph, feat, attn, H, D, slope):
    """The message-passing part of custom_GATv2Conv.forward (model.py:82-99) WITHOUT the intermediate bf16 roundings of the
    default kernels and with float results: (e [B, H], a [B, H], out [S, H*D]) from the bf16 operands ``feat`` = fc_src(h)
    [K, H*D] and ``attn``.  Forward only -- the check of the north star's 1e-4 bound against fp32 math (tests/); the model
    path rounds where the reference's bf16 tensor ops round."""
    feat, attn = feat.detach().contiguous(), attn.detach().reshape(-1).contiguous()
    assert feat.dtype == torch.bfloat16 and attn.dtype == torch.bfloat16 and feat.is_cuda
    nnz_ptr, B = _nnz(graph)
    S, HD, dev = graph.num_dst_nodes(), H * D, feat.device
    e = torch.empty(B, H, dtype=torch.float32, device=dev)
    a = torch.empty(B, H, dtype=torch.float32, device=dev)
    out = torch.empty(S, HD, dtype=torch.float32, device=dev)
    part = _gat_partials(B, HD, dev, 1)
    _lib.check(_lib.lib.bliss_gat_logits_f32(graph.src.data_ptr(), graph.dst.data_ptr(), nnz_ptr, B, feat.data_ptr(), feat.stride(0),
                                             attn.data_ptr(), H, D, float(slope), e.data_ptr(), _stream()), "bliss_gat_logits_f32")
    _lib.check(_lib.lib.bliss_gat_edge_softmax(graph.indptr.data_ptr(), S, e.data_ptr(), 0, H, 2, a.data_ptr(), _stream()),
               "bliss_gat_edge_softmax")
    _lib.check(_lib.lib.bliss_gat_rows(4, graph.indptr.data_ptr(), S, 0, graph.src.data_ptr(), graph.dst.data_ptr(), nnz_ptr, B,
                                       a.data_ptr(), feat.data_ptr(), feat.stride(0), 0, H, D, 0.0, out.data_ptr(), out.stride(0),
                                       part.data_ptr(), 0, _stream()), "bliss_gat_rows")
    return e, a, out


class GATv2Conv(nn.Module):
    """The reference's ``custom_GATv2Conv`` (model.py:13-112): dglnn.GATv2Conv with the forward that returns the
    PRE-softmax logits as "attention" (:108-110) and ignores ``edge_weight`` (:91-96 are commented out).

    [DGL-recalled] parameters: fc_src Linear(in, H*D, bias), shared with fc_dst when share_weights; attn (1,H,D);
    res_fc Linear(in, H*D, bias) when residual and in != H*D, identity when equal; xavier_normal(gain('relu'))."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False,
                 activation=None, allow_zero_in_degree=False, bias=True, share_weights=False, transforms="library"):
        super().__init__()
        if not share_weights:
            raise NotImplementedError("the reference always builds share_weights=True (model.py:152,170,186,202)")
        if transforms not in GAT_TRANSFORMS:
            raise ValueError("transforms must be one of %r, not %r" % (GAT_TRANSFORMS, transforms))
        self.transforms = transforms
        self._num_heads, self._out_feats, self._in = num_heads, out_feats, in_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self.fc_src = nn.Linear(in_feats, out_feats * num_heads, bias=bias)
        self.fc_dst = self.fc_src
        self.attn = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop, self.attn_drop = nn.Dropout(feat_drop), nn.Dropout(attn_drop)
        self.negative_slope = negative_slope
        if residual:
            self.res_fc = nn.Linear(in_feats, num_heads * out_feats, bias=bias) if in_feats != out_feats * num_heads else nn.Identity()
        else:
            self.res_fc = None
        self.activation = activation
        self.share_weights = share_weights
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc_src.weight, gain=gain)
        nn.init.xavier_normal_(self.attn, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)
        if bias:
            nn.init.constant_(self.fc_src.bias, 0)

    def _fused_state(self, device):
        """Device state of the fused kernels: the attention-dropout launch counter (uint64[2]: counter, ticket), its seed, and
        the ticket of the d attn reduction.  The seed is a function of torch's CUDA seed and of the layer's ordinal in its model
        (``_drop_salt``, set by model.GATv2): the same seeds give the same masks run after run (round 3: it used to mix in
        ``id(self)``, so two runs of one script trained differently)."""
        st = getattr(self, "_fstate", None)
        if st is None or st["ctr"].device != device:
            st = self._fstate = dict(ctr=torch.zeros(2, dtype=torch.int64, device=device), ticket=torch.zeros(1, dtype=torch.int32, device=device),
                                     seed=(torch.cuda.initial_seed() ^ (0x9E3779B1 * (int(getattr(self, "_drop_salt", 0)) + 1))) & 0xFFFFFFFF,
                                     err=torch.zeros(1, dtype=torch.int32, device=device), row_ws=None)
        return st

    def check_errors(self):
        """A row shared by several workgroups whose partners failed to meet within the spin bound (never seen; the grid drains
        and the word says so)."""
        st = getattr(self, "_fstate", None)
        if st is not None and int(st["err"].item()):
            raise RuntimeError("GATv2 fused kernels: error 0x%x (%s)" % (int(st["err"].item()), _lib.err_string(int(st["err"].item()))))

    # -- transforms="tile"  -------------------------------------------------------------------------
    def _feat_state(self, device):
        st = getattr(self, "_dstate", None)
        if st is None or st["ctr"].device != device:
            st = self._dstate = gat_drop_state(getattr(self, "_drop_salt", 0), device)
        return st

    def tile_refusal(self, what="GATv2Conv"):
        """Why this layer cannot take the tile path, or None: the limits that do not depend on the input tensor."""
        H, D, kind = self._num_heads, self._out_feats, self.transforms
        if kind == "wide":
            if self._in > TILE_WIDE_MAX_K:
                return ('%s: transforms="wide" takes in_feats <= %d (the K-panelled tile kernel), this layer has %d; build it with '
                        'transforms="library"' % (what, TILE_WIDE_MAX_K, self._in))
        elif self._in > TILE_GEMM_MAX_K:
            return ('%s: transforms="tile" takes in_feats <= %d (the tile kernel keeps a row tile\'s K columns in LDS), this layer '
                    'has %d; build it with transforms="library"' % (what, TILE_GEMM_MAX_K, self._in))
        if not _gat_fused_on(H, D):
            return ('%s: transforms="%s" runs on the fused message-passing kernels (bliss_gat_fused_supported(%d, %d) is false or '
                    'BLISS_GAT_FUSED=0)' % (what, kind, H, D))
        if not _mfma_bwd_on():
            return "%s: transforms=\"%s\" needs the MFMA backward (BLISS_SAGE_MFMA_BWD=0 is set)" % (what, kind)
        try:
            _glue_act(self.activation, what)
        except NotImplementedError as e:
            return str(e)
        return None

    def _tile_check(self, feat, what):
        why = self.tile_refusal(what)
        if why is None and not (feat.is_cuda and feat.dtype == torch.bfloat16 and self.fc_src.weight.dtype == torch.bfloat16):
            why = '%s: transforms="%s" takes bf16 features and parameters on the GPU' % (what, self.transforms)
        if why is not None:
            raise NotImplementedError(why)

    def tile_feat_drop(self, graph, feat):
        """feat_drop over the block's live source rows (identity in evaluation or with p = 0)."""
        p = float(self.feat_drop.p) if self.training else 0.0
        if p <= 0:
            return feat
        return gat_feat_drop(feat, p, self._feat_state(feat.device), graph.num_src_nodes(), _block_words(graph)[1])

    def tile_parts(self, graph, h_src, what="GATv2Conv"):
        """(rst [S, H*D], res [S, H*D] or None, e [B, H]) from the feat-dropped input rows: fc_src / res_fc on the tile kernels,
        model.py:82-99 on the fused kernels; every row past the block's live counts is zero."""
        H, D, S, K = self._num_heads, self._out_feats, graph.num_dst_nodes(), graph.num_src_nodes()
        self._tile_check(h_src, what)
        if h_src.shape[0] < K or h_src.shape[1] != self._in:
            raise ValueError("%s: %d x %d input rows for a block of %d sources and in_feats %d" % (what, h_src.shape[0], h_src.shape[1], K, self._in))
        if not self._allow_zero_in_degree and not torch.cuda.is_current_stream_capturing() and bool((graph.in_degrees() == 0).any()):
            raise RuntimeError("There are 0-in-degree nodes in the graph (model.py:49-61); build the layer with "
                               "allow_zero_in_degree=True or add self loops")      # (a host read: not taken inside a captured step)
        dst_dev, src_dev, _ = _block_words(graph)
        lin = isinstance(self.res_fc, nn.Linear)
        feat_src, res = gat_linear(h_src, self.fc_src.weight, self.fc_src.bias, K, src_dev,
                                   self.res_fc.weight if lin else None, self.res_fc.bias if lin else None, S if lin else 0, dst_dev if lin else 0,
                                   wide=self.transforms == "wide")
        if self.res_fc is not None and not lin:
            res = h_src[:S]                                                      # nn.Identity (in_feats == H * D)
        p_drop = float(self.attn_drop.p) if self.training else 0.0
        rst, e = _GatFusedMP.apply(feat_src, self.attn, graph, H, D, self.negative_slope, p_drop, self._fused_state(feat_src.device))
        return rst, res, e

    # -- full-neighbour inference off the graph's CSC -------------------------------------------------
    def infer_refusal(self, h_all, what="GATv2Conv"):
        """Why ``infer_transform`` / ``infer_rows`` cannot run on these input rows, or None."""
        why = _gat_infer_refusal(h_all, self._num_heads, self._out_feats, what)
        if why is None and self.fc_src.weight.dtype != torch.bfloat16:
            why = "%s: the CSC inference path takes bf16 parameters" % what
        if why is None and self.transforms in TILE_KINDS and self._in > TILE_GEMM_MAX_K:
            why = self.tile_refusal(what)                  # ("wide": None up to TILE_WIDE_MAX_K)
        if why is None:
            try:
                _glue_act(self.activation, what)
            except NotImplementedError:
                why = "%s: the CSC inference kernel's epilogue has the activations ELU (alpha 1) and None, not %r" % (what, self.activation)
        return why

    def infer_transform(self, h_all):
        """(fc_src(h) [V, H*D], res [V, H*D] or None) over ALL rows, once per layer: on the tile kernels for a
        ``transforms="tile"`` layer (a row's bits do not depend on how many rows the launch has), on nn.Linear otherwise.
        An identity residual is the input itself."""
        lin = isinstance(self.res_fc, nn.Linear)
        if self.transforms in TILE_KINDS:
            V = h_all.shape[0]
            feat_src, res = gat_linear(h_all, self.fc_src.weight, self.fc_src.bias, V, 0, self.res_fc.weight if lin else None,
                                       self.res_fc.bias if lin else None, V if lin else 0, 0, wide=self.transforms == "wide")
        else:
            feat_src, res = self.fc_src(h_all), (self.res_fc(h_all) if lin else None)
        if self.res_fc is not None and not lin:
            res = h_all                                                          # nn.Identity (in_feats == H * D)
        return feat_src, res

    def infer_rows(self, g, row0, row1, n_edges, feat_src_all, res_all, out, state):
        """The finished rows ``row0 .. row1 - 1`` of this layer in evaluation mode, flattened [rows, H*D], into ``out`` (see
        ``gat_infer_layer``): message passing over all in-edges, residual and activation in one launch pair."""
        return gat_infer_layer(g.indptr, g.indices, row0, row1, n_edges, feat_src_all, self.attn, self._num_heads, self._out_feats,
                               self.negative_slope, out, None if res_all is None else res_all[row0:row1],
                               _glue_act(self.activation, "GATv2Conv"), state)

    def _forward_tile(self, graph, feat, get_attention):
        H, D, S = self._num_heads, self._out_feats, graph.num_dst_nodes()
        self._tile_check(feat, "GATv2Conv")
        rst, res, e = self.tile_parts(graph, self.tile_feat_drop(graph, feat))
        out = gat_glue(rst, res, H, D, act=_glue_act(self.activation, "GATv2Conv"), n_rows=S, rows_dev=_block_words(graph)[0])[0].view(S, H, D)
        return (out, e.view(-1, H, 1)) if get_attention else out

    def forward(self, graph, feat, edge_weight=None, get_attention=False):
        H, D, S = self._num_heads, self._out_feats, graph.num_dst_nodes()
        if self.transforms in TILE_KINDS:
            return self._forward_tile(graph, feat, get_attention)
        if not self._allow_zero_in_degree and bool((graph.in_degrees() == 0).any()):
            raise RuntimeError("There are 0-in-degree nodes in the graph (model.py:49-61); build the layer with "
                               "allow_zero_in_degree=True or add self loops")
        h_src = self.feat_drop(feat)
        feat_src = self.fc_src(h_src)                                            # :66-72, [K, H*D]; feat_dst = feat_src[:S]
        if feat_src.is_cuda and feat_src.dtype == torch.bfloat16 and _gat_fused_on(H, D):
            p_drop = float(self.attn_drop.p) if self.training else 0.0
            rst, e = _GatFusedMP.apply(feat_src, self.attn, graph, H, D, self.negative_slope, p_drop, self._fused_state(feat_src.device))
            rst = rst.view(S, H, D)                                              # :82-99 in one launch
        else:
            e = _GatLogits.apply(feat_src, self.attn, graph, H, D, self.negative_slope)           # :82-86
            a = self.attn_drop(_EdgeSoftmax.apply(e, graph, H))                  # :88-90
            rst = _GatAggregate.apply(a, feat_src, graph, H, D).view(S, H, D)    # :98-99
        if self.res_fc is not None:
            rst = rst + self.res_fc(h_src[:S]).view(S, -1, D)                    # :101-103
        if self.activation:
            rst = self.activation(rst)
        return (rst, e.view(-1, H, 1)) if get_attention else rst                 # :108-112
