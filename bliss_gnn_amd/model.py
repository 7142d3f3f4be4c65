"""Models over bliss Blocks with the reference's constructor and forward signatures (model.py).

``SAGE(in_feats, n_hidden, n_classes, n_layers, activation, dropout).forward(blocks, x)`` stores the
source-row norms the bandit reward needs on ``block.srcdata['embed_norm']`` (model.py:318-320) and
runs the SAGEConv layers with the sampler's edge weights (model.py:321-329).
"""
import torch
import torch.nn as nn

from .nn import TILE_KINDS, SAGEConv, SAGEGCNConv, SAGELSTMConv, embed_norm, sage_epilogue


def _gathered_norm(blocks, x):
    """The row norms of ``x`` if it is blocks[0]'s feature slice as gathered by the fused gather + norm kernel
    (graph._LazyFrame), else None (the caller then runs embed_norm: same bits either way)."""
    fn = getattr(blocks[0].srcdata, "row_norm_of", None) if len(blocks) else None
    return fn(x) if fn is not None else None


class SAGE(nn.Module):
    """model.py:292-383."""

    # "auto": the fused MFMA path when every layer is within the tile kernel's limits (in <= 1024, out <= 256), else -- silently --
    # library GEMMs.  "wide" (DESIGN.md section 29): in_feats up to nn.TILE_WIDE_MAX_K on the K-panelled tile kernel, and
    # NotImplementedError naming the reason where the MFMA path cannot be taken: no silent fall-back.  "tile" (DESIGN.md section
    # 32): only kernels whose every row and edge loop is bounded by the block's device-side counts, or NotImplementedError --
    # for "mean" the MFMA path of "auto" (same launches and bits, in_feats <= 1024), for "pool" nn.sage_pool_tile per layer.
    SAGE_TRANSFORMS = ("auto", "wide", "tile")
    # "pool" (DESIGN.md section 30): SAGEConv(..., "pool") layers on library GEMMs and the max-reduce kernels of csrc/spmm_max.hip
    # under "auto"; on the tile kernels under "tile" (section 32).  "gcn" (section 34): nn.SAGEGCNConv layers -- library GEMMs
    # and the self-inclusive normalised sum of csrc/spmm_self.hip under "auto", nn.sage_gcn_tile per layer under "tile".
    SAGE_AGGREGATORS = ("mean", "pool", "gcn")

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout, transforms="auto", aggregator_type="mean"):
        super().__init__()
        if transforms not in self.SAGE_TRANSFORMS:
            raise ValueError("transforms must be one of %r, not %r" % (self.SAGE_TRANSFORMS, transforms))
        if aggregator_type not in self.SAGE_AGGREGATORS:
            raise NotImplementedError("SAGE: aggregator_type must be one of %r, not %r%s" % (
                self.SAGE_AGGREGATORS, aggregator_type,
                " (the 'lstm' aggregator is the model SAGELSTM: DESIGN.md section 37)" if aggregator_type == "lstm" else ""))
        if aggregator_type != "mean" and transforms == "wide":
            raise NotImplementedError('SAGE: transforms="wide" runs the MFMA tile path, which covers aggregator_type="mean", not %r'
                                      % (aggregator_type,))
        self.transforms, self.aggregator_type = transforms, aggregator_type
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.layers = nn.ModuleList()
        mk = {"gcn": SAGEGCNConv, "lstm": SAGELSTMConv}.get(aggregator_type) or (lambda i, o: SAGEConv(i, o, aggregator_type))
        if n_layers > 1:
            self.layers.append(mk(in_feats, n_hidden))
            for _ in range(1, n_layers - 1):
                self.layers.append(mk(n_hidden, n_hidden))
            self.layers.append(mk(n_hidden, n_classes))
        else:
            self.layers.append(mk(in_feats, n_classes))
        self.dropout = nn.Dropout(dropout)
        self.activation = activation

    def _fusable(self, h):
        act = self.activation
        relu = act in (torch.relu, torch.nn.functional.relu) or isinstance(act, nn.ReLU)
        return relu and h.is_cuda and h.dtype == torch.bfloat16 and isinstance(self.dropout, nn.Dropout)

    def _dropout_state(self, l, device):
        """Launch counter of the fused epilogue's dropout stream for layer l (device uint64[2]) and its seed."""
        if not hasattr(self, "_drop_ctr"):
            self._drop_ctr = {}
        key = (l, str(device))
        if key not in self._drop_ctr:
            self._drop_ctr[key] = torch.zeros(2 + 64, dtype=torch.int64, device=device)      # launch counter, ticket, 64 sub-tickets
        return self._drop_ctr[key], (torch.cuda.initial_seed() ^ (0x9E3779B1 * (l + 1))) & 0xFFFFFFFF

    accepts_lazy_rows = True        # forward() takes blocks[0].srcdata.lazy('features'): the gather becomes an operand load

    def _mfma_ok(self, x):
        """The fused matrix-core path (csrc/sage.hip) covers the reference's configuration: bf16 on the GPU, ReLU, every
        layer within the tile kernel's limits (in <= 1024, out <= 256)."""
        import os
        from .nn import tile_gemm_ok
        # BLISS_SAGE_MFMA=0 falls back to library GEMMs + separate gather / epilogue kernels (the round-1 path).  Device time per
        # launch on the Reddit-like step (scratch/tgbench.py, graph replay): 602 -> 256 pair with the gather 32-37 us (gather +
        # two tuned library GEMMs: 46), 256 + 256 dual with epilogue 20 (23), 256 -> 41 pair 13 (18), and five launches fewer
        if os.environ.get("BLISS_SAGE_MFMA", "1") == "0" or self.aggregator_type != "mean":
            return False
        act = self.activation
        relu = act in (torch.relu, torch.nn.functional.relu) or isinstance(act, nn.ReLU)
        wide = self.transforms == "wide"
        dims = all(tile_gemm_ok(l._in_src_feats, l._out_feats, wide) and l.fc_self.bias is not None and l.norm is None and l.activation is None
                   and l.feat_drop.p == 0 for l in self.layers)
        if self.transforms != "auto" and not all(q.is_cuda and q.dtype == torch.bfloat16 for q in self.parameters()):
            return False                                   # ("auto" rounds other parameters to bf16 per launch, as it always has)
        return relu and dims and x.is_cuda and x.dtype == torch.bfloat16 and isinstance(self.dropout, nn.Dropout)

    def mfma_refusal(self, x):
        """Why the MFMA path cannot take ``x`` (a tensor or LazyRows of the input rows, or a parameter), or None."""
        import os
        from .nn import TILE_GEMM_MAX_N, TILE_WIDE_MAX_K, tile_gemm_ok
        if self._mfma_ok(x):
            return None
        what = 'SAGE: transforms="%s"' % self.transforms
        if os.environ.get("BLISS_SAGE_MFMA", "1") == "0":
            return "%s runs on the MFMA kernels (BLISS_SAGE_MFMA=0 is set)" % what
        bad = [q for q in [x] + list(self.parameters()) if not (q.is_cuda and q.dtype == torch.bfloat16)]
        if bad:
            return "%s takes bf16 features and parameters on the GPU, not %s on %s" % (what, bad[0].dtype, bad[0].device)
        wide = self.transforms == "wide"
        for l, layer in enumerate(self.layers):
            if not tile_gemm_ok(layer._in_src_feats, layer._out_feats, wide):
                return ("SAGE layer %d: transforms=\"%s\" takes in_feats <= %d and out_feats <= %d, this layer has %d -> %d"
                        % (l, self.transforms, TILE_WIDE_MAX_K if wide else 1024, TILE_GEMM_MAX_N, layer._in_src_feats, layer._out_feats))
        return "%s covers ReLU, nn.Dropout and plain SAGEConv layers with a bias (no norm, activation or feat_drop of their own)" % what

    @property
    def _pool_tile(self):
        return self.transforms == "tile" and self.aggregator_type == "pool"

    @property
    def _gcn_tile(self):
        return self.transforms == "tile" and self.aggregator_type == "gcn"

    def tile_refusal(self, x):
        """Why transforms="tile" cannot take ``x`` (a tensor or LazyRows of the input rows, or a parameter), or None."""
        import os
        from .nn import TILE_GEMM_MAX_K, TILE_GEMM_MAX_N, tile_gemm_ok
        if not (self._pool_tile or self._gcn_tile):
            return self.mfma_refusal(x)
        what = 'SAGE: transforms="tile"'
        for env in ("BLISS_SAGE_MFMA", "BLISS_SAGE_MFMA_BWD"):
            if os.environ.get(env, "1") == "0":
                return "%s runs on the MFMA kernels, forward and backward (%s=0 is set)" % (what, env)
        bad = [q for q in [x] + list(self.parameters()) if not (q.is_cuda and q.dtype == torch.bfloat16)]
        if bad:
            return "%s takes bf16 features and parameters on the GPU, not %s on %s" % (what, bad[0].dtype, bad[0].device)
        act = self.activation
        if not (act in (torch.relu, torch.nn.functional.relu) or isinstance(act, nn.ReLU)):
            return "%s covers the activation ReLU (the tail's and the backward's mask), not %r" % (what, act)
        if not isinstance(self.dropout, nn.Dropout):
            return "%s covers nn.Dropout (the tail's own counter-based stream), not %s" % (what, type(self.dropout).__name__)
        for l, layer in enumerate(self.layers):
            if self._gcn_tile:                                                   # ('gcn' has no fc_self; its bias is optional)
                if layer.norm is not None or layer.activation is not None or layer.feat_drop.p != 0:
                    return ("SAGE layer %d: transforms=\"tile\" covers plain SAGEConv layers (no norm, activation or feat_drop of "
                            "their own)" % l)
            elif layer.norm is not None or layer.activation is not None or layer.feat_drop.p != 0 or layer.fc_self.bias is None:
                return ("SAGE layer %d: transforms=\"tile\" covers plain SAGEConv layers with a bias (no norm, activation or feat_drop "
                        "of their own)" % l)
            if not tile_gemm_ok(layer._in_src_feats, layer._out_feats):
                return ("SAGE layer %d: transforms=\"tile\" takes in_feats <= %d and out_feats <= %d, this layer has %d -> %d"
                        % (l, TILE_GEMM_MAX_K, TILE_GEMM_MAX_N, layer._in_src_feats, layer._out_feats))
        return None

    def _mfma_path(self, x):
        """Does this forward run on the MFMA kernels?  Under "wide" and "tile" the answer is yes or an error, never the library
        path; "pool" for the tile pool model (its own layer chain, _layers_pool_tile)."""
        if self._pool_tile:
            why = self.tile_refusal(x)
            if why is not None:
                raise NotImplementedError(why)
            return "pool"
        if self._gcn_tile:
            why = self.tile_refusal(x)
            if why is not None:
                raise NotImplementedError(why)
            return "gcn"
        if self._mfma_ok(x):
            return True
        if self.transforms != "auto":
            raise NotImplementedError(self.mfma_refusal(x))
        return False

    def _layers_pool_tile(self, blocks, h, norm, lo, hi):
        """model.py:312-333, layers lo..hi-1, for 'pool' on bounded kernels: per layer one autograd node,
        nn.sage_pool_tile -- fc_pool + ReLU, the max-reduce, and both Linears with the bias, ReLU, dropout and the next layer's
        norms.  The layer's input norms come out of its first launch."""
        from .nn import sage_pool_tile
        n_layers = len(self.layers)
        for l in range(lo, hi):
            layer, block = self.layers[l], blocks[l]
            last = l == n_layers - 1
            ew = block.edata["edge_weights"] if "edge_weights" in block.edata else None
            p = self.dropout.p if (self.training and not last) else 0.0
            ctr, seed = self._dropout_state(l, h.device) if p > 0 else (None, 0)
            h, out_norm, in_norm = sage_pool_tile(block, h, ew, layer, not last, p, ctr, seed)
            block.srcdata["embed_norm"] = in_norm if norm is None else norm      # model.py:318-320 (same bits either way)
            norm = None if last else out_norm
        return h, norm

    def _gcn_drop_state(self, l, device):
        """The keyed dropout stream of layer l's epilogue (nn.gat_drop_state: launch counter and seed)."""
        from .nn import gat_drop_state
        if not hasattr(self, "_gcn_dstate"):
            self._gcn_dstate = {}
        key = (l, str(device))
        if key not in self._gcn_dstate:
            self._gcn_dstate[key] = gat_drop_state(l + 1, device)
        return self._gcn_dstate[key]

    def _layers_gcn_tile(self, blocks, h, norm, lo, hi):
        """model.py:312-333, layers lo..hi-1, for 'gcn' on bounded kernels: per layer one autograd node,
        nn.sage_gcn_tile -- fc_neigh on the tile product, the self-inclusive normalised sum, and ONE epilogue launch with the bias,
        ReLU, the model's dropout and the next layer's row norms."""
        from .nn import sage_gcn_tile
        n_layers = len(self.layers)
        for l in range(lo, hi):
            layer, block = self.layers[l], blocks[l]
            last = l == n_layers - 1
            block.srcdata["embed_norm"] = embed_norm(h) if norm is None else norm            # model.py:318-320
            ew = block.edata["edge_weights"] if "edge_weights" in block.edata else None
            p = float(self.dropout.p) if (self.training and not last) else 0.0
            h, norm = sage_gcn_tile(block, h, ew, layer, not last, p, self._gcn_drop_state(l, h.device) if p > 0 else None, not last)
        return h, norm

    def _layers_mfma(self, blocks, h, norm, lo, hi, parts=False):
        """model.py:312-333, layers lo..hi-1, with the Linear layers on hand-written MFMA tiles: per W-first layer ONE launch
        for fc_neigh + fc_self (+ the feature gather and the input norms), per aggregate-first layer ONE launch for both
        Linears, the bias, ReLU, dropout and the next layer's norms.  The aggregation stays the merge-style SpMM of
        csrc/spmm.hip."""
        from .nn import LazyRows, _SageLinearPair, sage_agg_dual, weighted_aggregate
        n_layers = len(self.layers)
        for l in range(lo, hi):
            layer, block = self.layers[l], blocks[l]
            last = l == n_layers - 1
            S_b, K_b = block.num_dst_nodes(), block.num_src_nodes()
            cd = block._counts_dev.data_ptr() if block._nnz_ptr else 0           # capacity-padded block: true S, K on the device
            src_dev, dst_dev = (cd + 12, cd) if cd else (0, 0)
            ew = block.edata["edge_weights"] if "edge_weights" in block.edata else None
            p = self.dropout.p if (self.training and not last) else 0.0
            ctr, seed = self._dropout_state(l, h.device) if p > 0 else (None, 0)
            fc_n, fc_s = layer.fc_neigh, layer.fc_self
            if layer._in_src_feats > layer._out_feats:                           # fc_neigh before the aggregation
                table, ids = (h.table, h.ids) if isinstance(h, LazyRows) else (h, None)
                z, y, _rows, in_norm = _SageLinearPair.apply(table, ids, fc_n.weight, fc_s.weight, fc_s.bias, K_b, S_b, src_dev, dst_dev,
                                                             self.transforms == "wide")
                block.srcdata["embed_norm"] = in_norm if norm is None else norm  # model.py:318-320 (same bits either way)
                agg = weighted_aggregate(block, z, ew, mean=True)
                if last:
                    h, norm = ((y, agg) if parts else y + agg), None          # (parts: the loss kernel adds them itself)
                else:
                    h, norm = sage_epilogue(y, agg, p, ctr, seed)
            else:
                if isinstance(h, LazyRows):
                    h = h.materialize()
                block.srcdata["embed_norm"] = embed_norm(h) if norm is None else norm
                h, norm = sage_agg_dual(block, h, ew, fc_n.weight, fc_s.weight, fc_s.bias, not last, p, ctr, seed, dst_dev)
                if last:
                    norm = None
        return h, norm

    def _layers_plain(self, blocks, h, norm, lo, hi):
        """model.py:312-333, layers lo..hi-1, on library GEMMs (+ the fused epilogue where it applies)."""
        for l in range(lo, hi):
            layer, block = self.layers[l], blocks[l]
            block.srcdata["embed_norm"] = embed_norm(h) if norm is None else norm          # model.py:318-320
            norm = None
            ew = block.edata["edge_weights"] if "edge_weights" in block.edata else None
            if l < len(self.layers) - 1 and self._fusable(h):
                # rst = fc_self + h_neigh, activation, dropout (:321-333) and the next layer's row norms in ONE kernel
                parts = layer(block, h, edge_weight=ew, parts=True)
                if isinstance(parts, tuple):
                    p = self.dropout.p if self.training else 0.0
                    ctr, seed = self._dropout_state(l, h.device) if p > 0 else (None, 0)
                    h, norm = sage_epilogue(parts[0], parts[1], p, ctr, seed)
                    continue
                h = parts
            else:
                h = layer(block, h, edge_weight=ew)
            if l < len(self.layers) - 1:
                h = self.activation(h)
                h = self.dropout(h)
        return h, norm

    def _layers(self, blocks, x, norm, lo, hi, mfma):
        from .nn import LazyRows
        if mfma == "pool":
            return self._layers_pool_tile(blocks, x, norm, lo, hi)
        if mfma is True:
            return self._layers_mfma(blocks, x, norm, lo, hi)
        if isinstance(x, LazyRows):
            x = x.materialize()
        if lo == 0 and norm is None:
            norm = _gathered_norm(blocks, x)
        if mfma == "gcn":
            return self._layers_gcn_tile(blocks, x, norm, lo, hi)
        return self._layers_plain(blocks, x, norm, lo, hi)

    def forward(self, blocks, x):
        return self._layers(blocks, x, None, 0, len(self.layers), self._mfma_path(x))[0]

    # The bandit update (sampler.exp3) reads every block's INPUT row norms (model.py:318-320) and nothing the output layer
    # computes, so a training loop may run forward_hidden -> exp3 -> next batch's sampler and leave forward_last + loss +
    # backward to a second stream (train.PipelinedTrainStep).  forward(blocks, x) == forward_last(blocks, forward_hidden(...)).
    def forward_hidden(self, blocks, x):
        """Layers 0..L-2 and the output layer's input norms: every block's srcdata['embed_norm'] is set on return."""
        n = len(self.layers)
        if n < 2:
            raise ValueError("forward_hidden needs at least one hidden layer")
        mfma = self._mfma_path(x)
        h, norm = self._layers(blocks, x, None, 0, n - 1, mfma)
        if norm is None:
            norm = embed_norm(h)
        blocks[n - 1].srcdata["embed_norm"] = norm
        return h, norm, mfma

    def forward_last(self, blocks, hidden):
        """The output layer on forward_hidden's result."""
        h, norm, mfma = hidden
        n = len(self.layers)
        return self._layers(blocks, h, norm, n - 1, n, mfma)[0]

    def forward_last_parts(self, blocks, hidden):
        """forward_last as the two addends of ``rst = fc_self + h_neigh`` (model.py:321-329) when the output layer runs
        fc_neigh before the aggregation on the fused path (the loss kernel then adds them itself); else None."""
        h, norm, mfma = hidden
        n = len(self.layers)
        layer = self.layers[n - 1]
        if mfma is not True or layer._in_src_feats <= layer._out_feats:      # (no pool layer runs fc_neigh first)
            return None
        return self._layers_mfma(blocks, h, norm, n - 1, n, parts=True)[0]

    INFERENCE_PATHS = ("chunks", "blocks", "csc", "auto")
    # "csc": the rows are cut into ranges of whole batches and grouped into launches as in GCN.inference (_csc_ranges,
    # _csc_groups); the SpMM keeps no scratch, so the two limits only bound a launch's 32-bit edge offsets
    csc_max_edges = 1 << 23
    csc_spmm_edges = 2 ** 31 - 1
    last_inference_path = None      # the path the last ``inference`` call took

    def csc_refusal(self, g, h, batch_size=128):
        """Why ``inference(path="csc")`` cannot run on this graph, these features and this batch size, or None."""
        if int(batch_size) < 1:
            return "SAGE.inference: the CSC path takes batch_size >= 1, not %d" % int(batch_size)
        if self.aggregator_type == "lstm":
            return ('SAGE.inference: the CSC path covers aggregator_type "mean" and "pool", not "lstm" (DESIGN.md section 37); '
                    'path="blocks" runs it')
        if self.aggregator_type == "gcn":
            return ('SAGE.inference: the CSC path covers aggregator_type "mean" and "pool", not "gcn" (DESIGN.md section 34); '
                    'path="blocks" and "chunks" run it')
        if self.aggregator_type == "pool":
            if self.transforms != "tile":
                return ('SAGE.inference: the CSC path of aggregator_type="pool" has the bits of the tile kernels; build the model '
                        'with transforms="tile" (this one is %r)' % (self.transforms,))
            why = self.tile_refusal(h)
        else:
            why = self.mfma_refusal(h)                # (the default "auto" model on its MFMA path: the tile path's bits)
        if why is not None:
            return why
        if not (g.device.type == "cuda" and h.is_cuda):
            return "SAGE.inference: the CSC path runs on the GPU (graph on %s, features on %s)" % (g.device, h.device)
        return None

    def _inference_blocks(self, g, h, batch_size):
        """The reference's own loop (model.py:366-382): per layer, per contiguous batch of ``batch_size`` nodes, the
        full-neighbour block through layer l of the model's own layer chain (MFMA, pool-tile or library, whichever the model is
        on) in evaluation mode.  The yardstick of the CSC path; slow on purpose."""
        from .graph import full_neighbor_block
        if batch_size < 1:
            raise ValueError("SAGE.inference: batch_size >= 1, not %d" % batch_size)
        V, mfma = g.num_nodes(), self._mfma_path(h)
        for l in range(len(self.layers)):
            y = None
            for b0 in range(0, V, batch_size):
                b1 = min(V, b0 + batch_size)
                blk = full_neighbor_block(g, b0, b1)
                out = self._layers([None] * l + [blk], h[blk.srcdata["_ID"].long()], None, l, l + 1, mfma)[0]
                if y is None:
                    y = torch.empty(V, out.shape[1], dtype=out.dtype, device=out.device)
                y[b0:b1] = out
            h = y
        return h

    def _inference_csc(self, g, h, batch_size):
        """Per layer over ALL rows at once: the dense transforms once on the tile kernels -- the argument
        sets of _SageLinearPair / _SageAggDual / _SagePoolTile without ids, norms, dropout -- and one forward-only
        message-passing launch per group of ranges off the graph's own indptr / indices (nn.sage_infer_spmm).  Evaluation mode:
        no dropout, no norms.  One host read per call (_csc_ranges); nothing of size E is allocated."""
        from .nn import _bf16c, _col_blocks, _tg_args, _tile_gemm, _tile_gemm_by_size, sage_infer_spmm
        groups = _csc_groups(_csc_ranges(g, batch_size, self.csc_max_edges, "SAGE.inference"), self.csc_spmm_edges)
        V, dev, n_layers = g.num_nodes(), h.device, len(self.layers)
        pool, wide = self.aggregator_type == "pool", self.transforms == "wide"
        new = lambda n: torch.empty(V, n, dtype=torch.bfloat16, device=dev)

        def message_passing(table, reduce):
            agg = new(table.shape[1])
            for r0, r1, e0, edges in groups:
                sage_infer_spmm(g.indptr, g.indices, batch_size, r0, r1, e0, edges, table, agg[r0:r1], reduce)
            return agg

        h = _bf16c(h)
        for l, layer in enumerate(self.layers):
            last = l == n_layers - 1
            wn, ws, b = _bf16c(layer.fc_neigh.weight), _bf16c(layer.fc_self.weight), layer.fc_self.bias
            fin, fout = layer._in_src_feats, layer._out_feats
            if pool:
                wp, bp = _bf16c(layer.fc_pool.weight), layer.fc_pool.bias
                pooled = new(fin)
                sets = [_tg_args(h, wp[c0:c1], pooled[:, c0:c1], V, bias=None if bp is None else bp[c0:c1], relu=True)
                        for c0, c1 in _col_blocks(fin)]
                for i in range(0, len(sets), 2):
                    _tile_gemm(sets[i], sets[i + 1] if i + 1 < len(sets) else None)
                neigh = message_passing(pooled, "max")
                out = new(fout)
                _tile_gemm_by_size(_tg_args(neigh, wn, out, V, a2=h, w2=ws, bias=b, relu=not last))
            elif fin > fout:                                                     # fc_neigh before the aggregation
                z, y = new(fout), new(fout)
                _tile_gemm(_tg_args(h, wn, z, V), _tg_args(h, ws, y, V, bias=b), wide=wide)
                agg = message_passing(z, "mean")
                out = y + agg if last else sage_epilogue(y, agg, 0.0, None, 0)[0]
            else:
                agg = message_passing(h, "mean")
                out = new(fout)
                _tile_gemm(_tg_args(agg, wn, out, V, a2=h, w2=ws, bias=b, relu=not last))
            h = out
        return h

    @torch.no_grad()
    def inference(self, g, device=None, batch_size=128, use_uva=False, num_workers=0, node_chunk=16384, path="chunks"):
        """model.py:335-383: layer-wise full-neighbour inference over ALL nodes (no sampling, plain mean, no edge weights).
        Returns y [V, classes] and leaves it in ``g.ndata['h']`` like the reference (:382); the path taken is left in
        ``last_inference_path``.

        ``path="chunks"`` (the default): the reference walks the nodes 128 at a time through a DataLoader; every output row
        depends only on its own in-neighbours, so the rows are computed in chunks of ``node_chunk`` contiguous nodes straight from
        the CSC, the Linear layers on library GEMMs (``batch_size``, ``use_uva`` and ``num_workers`` are accepted for signature
        compatibility).
        ``path="blocks"``: the reference's own loop honouring ``batch_size`` -- the full-neighbour block of every contiguous batch
        through the model's own layer chain, i.e. the kernels the model trains on.
        ``path="csc"``: one pass per layer over all nodes, the dense transforms once on the tile kernels,
        one forward-only message-passing launch per range of rows straight off the graph's CSC -- the bits of "blocks" at the
        same ``batch_size``, no block built (``node_chunk`` is ignored).  Raises NotImplementedError naming the reason
        (``csc_refusal``) when it cannot run.
        ``path="auto"``: "csc" when nothing refuses it, "chunks" otherwise ("blocks" for aggregator_type="gcn" and "lstm", which have no CSC path;
        "lstm" has no chunk path either)."""
        if path not in self.INFERENCE_PATHS:
            raise ValueError("path must be one of %r, not %r" % (self.INFERENCE_PATHS, path))
        h = g.ndata["features"]                                              # :346
        if path in ("csc", "auto"):
            why = self.csc_refusal(g, h, batch_size)
            if path == "csc" and why is not None:
                raise NotImplementedError(why)
            path = "csc" if why is None else ("blocks" if self.aggregator_type in ("gcn", "lstm") else "chunks")
        if path == "chunks" and self.aggregator_type == "lstm":
            raise NotImplementedError('SAGE.inference: path="chunks" covers aggregator_type "mean", "pool" and "gcn", not "lstm" '
                                      '(DESIGN.md section 37); path="blocks" runs it')
        was_training = self.training
        self.eval()                                                          # :364
        try:
            if path == "csc":
                h = self._inference_csc(g, h, int(batch_size))
            elif path == "blocks":
                h = self._inference_blocks(g, h, int(batch_size))
            else:
                h = self._inference_chunks(g, h, node_chunk)
        finally:
            self.train(was_training)
        g.ndata["h"] = h
        self.last_inference_path = path
        return h

    def _inference_chunks(self, g, h, node_chunk):
        """``inference(path="chunks")``: library GEMMs over all rows, the block kernels' message passing per chunk of rows."""
        V = g.num_nodes()
        deg = g.indptr[1:] - g.indptr[:-1]
        dst_all = torch.repeat_interleave(torch.arange(V, device=g.device, dtype=torch.int32), deg)
        pool, gcn = self.aggregator_type == "pool", self.aggregator_type == "gcn"
        for l, layer in enumerate(self.layers):                              # :366
            before = not pool and layer._in_src_feats > layer._out_feats     # SAGEConv 'mean', 'gcn': fc_neigh before aggregation iff in > out
            if pool:                                                         # relu(fc_pool(h)) once over all nodes, fc_neigh after the max
                src_feat = torch.relu(layer.fc_pool(h))
            else:
                src_feat = layer.fc_neigh(h) if before else h
            y = torch.empty(V, layer._out_feats, dtype=h.dtype, device=h.device)
            for b0 in range(0, V, node_chunk):
                b1 = min(V, b0 + node_chunk)
                neigh = _full_neighbor(g, src_feat, b0, b1, dst_all, pool, gcn)
                if not before:
                    neigh = layer.fc_neigh(neigh)
                if gcn:                                                      # (no fc_self: the node's own row rode in the aggregation)
                    out = neigh if layer.bias is None else neigh + layer.bias
                else:
                    out = layer.fc_self(h[b0:b1]) + neigh
                if l < len(self.layers) - 1:
                    out = self.dropout(self.activation(out))                 # :377-379 (dropout is the identity in eval mode)
                y[b0:b1] = out
            h = y
        return h


class SAGELSTM(SAGE):
    """SAGE with the 'lstm' aggregator [DGL-recalled: dglnn.SAGEConv(in, out, 'lstm')], a model of its own because
    ``SAGE(..., aggregator_type="lstm")`` keeps refusing: nn.SAGELSTMConv layers on library GEMMs and the
    recurrent aggregation of csrc/lstm.hip, every layer's input norms as in SAGE.  Every layer's input width is at most 256."""
    SAGE_AGGREGATORS = ("lstm",)

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout):
        super().__init__(in_feats, n_hidden, n_classes, n_layers, activation, dropout, transforms="auto", aggregator_type="lstm")

    def inference(self, g, device=None, batch_size=128, use_uva=False, num_workers=0, node_chunk=16384, path="auto"):
        """SAGE.inference with ``path="auto"`` as the default, which resolves to "blocks" -- the only path this model has:
        "chunks" and "csc" raise NotImplementedError naming the aggregator."""
        return super().inference(g, device, batch_size, use_uva, num_workers, node_chunk, path)


def _csc_ranges(g, batch_size, max_edges, what):
    """Destination ranges of a CSC inference path: [(row0, row1, edge0, edges)], contiguous, whole batches, at least one batch each.
    Cut k is the first batch boundary whose edge offset is at or past k * max_edges, so a range holds fewer than max_edges edges
    plus one batch's -- cut on the device, read by the host ONCE per call."""
    V, E, bs = g.num_nodes(), g.num_edges(), int(batch_size)
    bounds = torch.cat([torch.arange(0, V, bs, device=g.device, dtype=torch.int64), torch.tensor([V], device=g.device, dtype=torch.int64)])
    off = g.indptr[bounds]                                                                    # E0_b of every batch, then E
    cuts = [bounds[:1], bounds[-1:]]
    if E > max_edges:
        targets = off[0] + torch.arange(1, E // int(max_edges) + 1, device=g.device, dtype=torch.int64) * int(max_edges)
        cuts.append(bounds[torch.searchsorted(off, targets).clamp_(max=bounds.numel() - 1)])  # the first boundary at or past a target
    cuts = torch.unique(torch.cat(cuts))                                                      # (sorted)
    both = torch.stack([cuts, g.indptr[cuts]]).tolist()                                       # the call's one host read
    ranges = [(r0, r1, e0, e1 - e0) for r0, r1, e0, e1 in zip(both[0][:-1], both[0][1:], both[1][:-1], both[1][1:])]
    if any(r[3] >= 2 ** 31 for r in ranges):
        raise NotImplementedError("%s: a range of 2^31 or more edges is beyond the CSC path (lower batch_size)" % what)
    return ranges


def _csc_groups(ranges, spmm_edges):
    """The SpMM's launches: consecutive ranges joined while they hold at most spmm_edges edges together."""
    groups = []
    for r0, r1, e0, edges in ranges:
        if groups and groups[-1][3] + edges <= int(spmm_edges):
            p0, _, pe0, pedges = groups[-1]
            groups[-1] = (p0, r1, pe0, pedges + edges)
        else:
            groups.append((r0, r1, e0, edges))
    return groups


def _full_neighbor(g, h, b0, b1, dst_all, pool=False, gcn=False):
    """mean (``pool``: max, no winning edge recorded; ``gcn``: the self-inclusive normalised sum, the destinations' rows h[b0:b1]
    handed over as h_self since they are not the leading source rows) over ALL in-neighbours of nodes b0..b1-1 (a MultiLayerFullNeighborSampler(1)
    block without edge weights, model.py:347-349, 375-376): the CSC columns of a contiguous node range are one contiguous slice."""
    import torch
    from .graph import Block
    from .nn import gcn_aggregate, max_aggregate, weighted_aggregate
    e0, e1 = int(g.indptr[b0]), int(g.indptr[b1])
    indptr = (g.indptr[b0:b1 + 1] - e0).to(torch.int32)
    src = g.indices[e0:e1]
    dst = dst_all[e0:e1] - b0
    blk = Block(None, h.shape[0], b1 - b0, indptr, src, dst, src, src, torch.empty(0, dtype=torch.int32, device=h.device))
    blk._transposed = (None, None)
    if gcn:
        return gcn_aggregate(blk, h, None, h_self=h[b0:b1])
    return max_aggregate(blk, h, None) if pool else weighted_aggregate(blk, h, None, mean=True)


class GCN(nn.Module):
    """model.py:386-439: stacked ``dglnn.GraphConv(norm='both', allow_zero_in_degree=True)`` with the sampler's edge
    weights.  (Unreachable from the reference's CLI -- ``--model gcn`` trains SAGE, train_lightning.py:597-607 -- kept
    for API completeness.)"""

    def __init__(self, in_feats, n_hidden, n_classes, n_layers, activation, dropout, transforms="library"):
        super().__init__()
        from .nn import GCN_TRANSFORMS, GraphConv
        if transforms not in GCN_TRANSFORMS:
            raise ValueError("transforms must be one of %r, not %r" % (GCN_TRANSFORMS, transforms))
        # "tile" (DESIGN.md section 26): the layers on the bounded kernels of csrc/gcn.hip and the MFMA entry points, the model's
        # dropout inside each layer's epilogue launch -- the path that runs under a batch capacity; "library": the launches and
        # bits of before; "wide" (section 29): "tile" with in_feats up to nn.TILE_WIDE_MAX_K
        self.transforms = transforms
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        mk = lambda i, o, act: GraphConv(i, o, activation=act, allow_zero_in_degree=True, transforms=transforms)
        self.layers = nn.ModuleList()
        if n_layers > 1:
            self.layers.append(mk(in_feats, n_hidden, activation))
            for _ in range(1, n_layers - 1):
                self.layers.append(mk(n_hidden, n_hidden, activation))
            self.layers.append(mk(n_hidden, n_classes, None))
        else:
            self.layers.append(mk(in_feats, n_classes, None))
        for l, layer in enumerate(self.layers):                    # the dropout stream of layer l (nn.GraphConv._drop_state)
            layer._drop_salt = l + 1
        self.dropout = nn.Dropout(dropout)
        self.activation = activation

    def tile_refusal(self):
        """Why this model cannot take the tile path (a layer outside its limits), or None."""
        for l, layer in enumerate(self.layers):
            why = layer.tile_refusal("GCN layer %d" % l)
            if why is not None:
                return why
        return None

    def _forward_tile(self, blocks, x):
        """``forward`` on the bounded kernels: per layer the norms, the degree-normalised SpMM, one MFMA product and ONE epilogue
        launch that carries the bias, the layer's ReLU, the model's dropout (:437-438) and the next block's embed_norm."""
        if len(blocks) != len(self.layers):
            raise ValueError("%d blocks for %d layers" % (len(blocks), len(self.layers)))
        n = len(self.layers)
        h, norm = x, _gathered_norm(blocks, x)
        for l, (layer, block) in enumerate(zip(self.layers, blocks)):
            last = l == n - 1
            if norm is None:
                norm = embed_norm(h)
            block.srcdata["embed_norm"] = norm                                                    # model.py:425-427
            p = float(self.dropout.p) if (self.training and not last) else 0.0
            h, norm = layer.tile_forward(block, h, block.edata["edge_weights"] if "edge_weights" in block.edata else None, p=p,
                                         want_norm=not last, what="GCN layer %d" % l)
        return h

    def forward(self, blocks, x):
        if self.transforms in TILE_KINDS:
            return self._forward_tile(blocks, x)
        h, norm = x, _gathered_norm(blocks, x)
        for l, (layer, block) in enumerate(zip(self.layers, blocks)):
            block.srcdata["embed_norm"] = embed_norm(h) if (l > 0 or norm is None) else norm      # model.py:425-427
            h = layer(block, h, edge_weight=(block.edata["edge_weights"] if "edge_weights" in block.edata else None))
            if l < len(self.layers) - 1:
                h = self.dropout(h)                                           # model.py:437-438
        return h

    INFERENCE_PATHS = ("auto", "blocks", "csc")
    # "csc": a destination range closes at the first batch boundary at or after a multiple of this many edges.  The by-source sort
    # of a range costs about 24 bytes of scratch per edge (t_edge, three key / value arrays, rocPRIM's pair of buffers): 200 MB at 2^23
    csc_max_edges = 1 << 23
    # the SpMM keeps no scratch, and a launch lasts at least as long as its longest row: one launch takes consecutive ranges as long
    # as they hold at most this many edges together (32-bit offsets inside a launch)
    csc_spmm_edges = 2 ** 31 - 1
    last_inference_path = None      # the path the last ``inference`` call took

    def csc_refusal(self, g, h, batch_size=128):
        """Why ``inference(path="csc")`` cannot run on this graph, these features and this batch size, or None."""
        if int(batch_size) < 1:
            return "GCN.inference: the CSC path takes batch_size >= 1, not %d" % int(batch_size)
        if not (g.device.type == "cuda" and h.is_cuda):
            return "GCN.inference: the CSC path runs on the GPU (graph on %s, features on %s)" % (g.device, h.device)
        for l, layer in enumerate(self.layers):
            why = layer.infer_refusal(h, "GCN layer %d" % l)
            if why is not None:
                return why
        return None

    def _csc_ranges(self, g, batch_size):
        """Destination ranges of the CSC path: [(row0, row1, edge0, edges)], contiguous, whole batches, at least one batch each.
        Cut k is the first batch boundary whose edge offset is at or past k * csc_max_edges, so a range holds fewer than
        csc_max_edges edges plus one batch's -- cut on the device, read by the host ONCE per call."""
        return _csc_ranges(g, batch_size, self.csc_max_edges, "GCN.inference")

    def _csc_groups(self, ranges):
        """The SpMM's launches: consecutive ranges joined while they hold at most csc_spmm_edges edges together."""
        return _csc_groups(ranges, self.csc_spmm_edges)

    def _inference_csc(self, g, h, batch_size):
        """The per-edge source norms of the batch structure ONCE per call (they do not depend on the layer; [E] fp32 kept for the
        call; one by-source sort per destination range), then per layer: a weight-first product once over all rows, one SpMM
        launch per group of ranges off the graph's own indptr / indices, an aggregate-first product and the epilogue once over
        all rows."""
        from .nn import gcn_infer_src_norms, gcn_infer_state
        ranges = self._csc_ranges(g, batch_size)
        V, state = g.num_nodes(), gcn_infer_state()
        ns = torch.empty(max(g.num_edges(), 1), dtype=torch.float32, device=h.device)
        for r0, r1, e0, edges in ranges:
            gcn_infer_src_norms(g.indptr, g.indices, batch_size, r0, r1, e0, edges, ns[e0:e0 + edges], state)
        del state
        groups = self._csc_groups(ranges)
        for layer in self.layers:
            table = layer.infer_transform(h)
            agg = torch.empty(V, table.shape[1], dtype=torch.bfloat16, device=h.device)
            for r0, r1, e0, edges in groups:
                layer.infer_rows(g, batch_size, r0, r1, e0, edges, ns[e0:e0 + edges], table, agg[r0:r1])
            del table
            h = layer.infer_finish(agg)
            g.ndata["h"] = h
        return h

    @torch.no_grad()
    def inference(self, g, device=None, batch_size=128, use_uva=False, num_workers=0, path="auto"):
        """model.py:441-488.  GraphConv(norm='both') normalises by the BLOCK's out-degrees, so the result depends on how
        the nodes are batched: ``batch_size`` is honoured exactly (contiguous batches, unshuffled, last one short).

        ``path="blocks"``: the full-neighbour block of every batch through the layers' ``forward``.
        ``path="csc"``: straight off the graph's CSC -- the same batches, the same bits for a
        ``transforms="tile"`` model, no block built.  Raises NotImplementedError naming the reason when it cannot run.
        ``path="auto"``: "csc" when nothing refuses it (a ``transforms="tile"`` model with bf16 features on the GPU), "blocks"
        otherwise.  The path taken is left in ``last_inference_path``."""
        if path not in self.INFERENCE_PATHS:
            raise ValueError("path must be one of %r, not %r" % (self.INFERENCE_PATHS, path))
        h = g.ndata["features"]
        if path != "blocks":
            why = self.csc_refusal(g, h, batch_size)
            if path == "csc" and why is not None:
                raise NotImplementedError(why)
            path = "csc" if why is None else "blocks"
        was_training = self.training
        self.eval()
        try:
            if path == "csc":
                h = self._inference_csc(g, h, int(batch_size))
            else:
                n = len(self.layers)
                h = _blockwise_inference(self.layers, g, h, int(batch_size), lambda l, out: self.dropout(out) if l < n - 1 else out)
        finally:
            self.train(was_training)
        self.last_inference_path = path
        return h


def _blockwise_inference(layers, g, h, batch_size, finish):
    """The shared loop of the reference's three ``inference`` methods: per layer, walk all nodes in contiguous batches,
    run the layer on the full-neighbour block of the batch and write the rows into y (model.py:267-288, 472-487)."""
    from .graph import full_neighbor_block
    V = g.num_nodes()
    for l, layer in enumerate(layers):
        y = None
        for b0 in range(0, V, batch_size):
            b1 = min(V, b0 + batch_size)
            blk = full_neighbor_block(g, b0, b1)
            out = finish(l, layer(blk, h[blk.srcdata["_ID"].long()]))
            if y is None:
                y = torch.empty(V, out.shape[1], dtype=h.dtype, device=h.device)
            y[b0:b1] = out
        h = y
        g.ndata["h"] = h
    return h


class GATv2(nn.Module):
    """model.py:115-234.  ``forward`` stores embed_norm (srcdata) and the head-mean pre-softmax logits ``a_ij`` (edata)
    that the bandit's calculate_alpha consumes (model.py:211-213, 224-227)."""

    def __init__(self, num_layers, in_dim, num_hidden, num_classes, heads, activation, feat_drop, attn_drop, negative_slope,
                 residual, transforms="library"):
        super().__init__()
        from .nn import GAT_TRANSFORMS, GATv2Conv
        if transforms not in GAT_TRANSFORMS:
            raise ValueError("transforms must be one of %r, not %r" % (GAT_TRANSFORMS, transforms))
        # "tile" (DESIGN.md section 22): the dense transforms on the MFMA tile kernels and the glue between the layers in one
        # bounded launch per direction -- the path that runs under a batch capacity; "library": the launches and bits of before;
        # "wide" (section 29): "tile" with in_dim up to nn.TILE_WIDE_MAX_K
        self.transforms = transforms
        self.num_layers, self.activation = num_layers, activation
        self.num_hidden, self.num_classes, self.heads = num_hidden, num_classes, heads
        mk = lambda i, o, h, res, act: GATv2Conv(i, o, h, feat_drop, attn_drop, negative_slope, res, act, bias=False,
                                                 share_weights=True, allow_zero_in_degree=True, transforms=transforms)
        self.gatv2_layers = nn.ModuleList()
        if num_layers > 1:
            self.gatv2_layers.append(mk(in_dim, num_hidden, heads[0], False, activation))                     # :141-155
            for l in range(1, num_layers - 1):
                self.gatv2_layers.append(mk(num_hidden * heads[l - 1], num_hidden, heads[l], residual, activation))
            self.gatv2_layers.append(mk(num_hidden * heads[-2], num_classes, heads[-1], residual, None))       # :175-189
        else:
            self.gatv2_layers.append(mk(in_dim, num_classes, heads[-1], residual, None))
        for l, layer in enumerate(self.gatv2_layers):              # the attention-dropout stream of layer l (nn.GATv2Conv._fused_state)
            layer._drop_salt = l + 1

    def tile_refusal(self):
        """Why this model cannot take the tile path (a layer outside its limits), or None."""
        for l, layer in enumerate(self.gatv2_layers):
            why = layer.tile_refusal("GATv2 layer %d" % l)
            if why is not None:
                return why
        return None

    def _forward_tile(self, blocks, inputs):
        """``forward`` on the bounded kernels: per layer the two Linears (one or two tile launches), the fused message passing, the
        head mean of the logits and ONE glue launch (residual, activation, flatten / head mean, the next layer's feat_drop)."""
        from .nn import _block_words, _glue_act, gat_glue, gat_head_mean
        if len(blocks) != len(self.gatv2_layers):
            raise ValueError("%d blocks for %d layers" % (len(blocks), len(self.gatv2_layers)))
        why = self.tile_refusal()
        if why is None and not (inputs.is_cuda and inputs.dtype == torch.bfloat16):
            why = 'GATv2: transforms="%s" takes bf16 features on the GPU' % self.transforms
        if why is not None:
            raise NotImplementedError(why)
        n = len(blocks)
        norm = _gathered_norm(blocks, inputs)
        h = inputs                                                                   # the layer input before its feat_drop
        h_drop = self.gatv2_layers[0].tile_feat_drop(blocks[0], h)
        for l, block in enumerate(blocks):
            layer, last = self.gatv2_layers[l], l == n - 1
            block.srcdata["embed_norm"] = embed_norm(h) if (l > 0 or norm is None) else norm                   # :211-213
            rst, res, e = layer.tile_parts(block, h_drop, "GATv2 layer %d" % l)
            dst_dev, _, edges_dev = _block_words(block)
            block.edata["a_ij"] = gat_head_mean(e, block.num_edges(), edges_dev)                               # :224-227
            nxt = None if last else self.gatv2_layers[l + 1]
            p = float(nxt.feat_drop.p) if (nxt is not None and self.training) else 0.0
            h_drop, h = gat_glue(rst, res, layer._num_heads, layer._out_feats, act=_glue_act(layer.activation, "GATv2 layer %d" % l),
                                 head_mean=last, p=p, state=nxt._feat_state(rst.device) if p > 0 else None,
                                 n_rows=block.num_dst_nodes(), rows_dev=dst_dev, want_pre=True)                 # :101-106, :228-232, :66
        return h_drop

    def forward(self, blocks, inputs):
        if self.transforms in TILE_KINDS:
            return self._forward_tile(blocks, inputs)
        h = inputs.bfloat16()
        norm = _gathered_norm(blocks, h)
        for l, block in enumerate(blocks):
            block.srcdata["embed_norm"] = embed_norm(h) if (l > 0 or norm is None) else norm                   # :211-213
            h, a = self.gatv2_layers[l](block, h, edge_weight=(block.edata["edge_weights"] if "edge_weights" in block.edata else None),
                                        get_attention=True)
            block.edata["a_ij"] = a.squeeze(-1).mean(dim=1)                                                    # :224-227
            h = h.flatten(1) if l < len(blocks) - 1 else h.mean(1)                                             # :228-232
        return h

    INFERENCE_PATHS = ("auto", "blocks", "csc")
    csc_min_rows = 1 << 16          # "csc": a destination range holds at least this many rows (``node_chunk`` may ask for more) ...
    csc_max_edges = 1 << 22         # ... and about this many edges at most: the fp32 partial rows of the scratch grow with edges / 256
    last_inference_path = None      # the path the last ``inference`` call took

    def csc_refusal(self, g, h):
        """Why ``inference(path="csc")`` cannot run on this graph and these features, or None."""
        if not (g.device.type == "cuda" and h.is_cuda):
            return "GATv2.inference: the CSC path runs on the GPU (graph on %s, features on %s)" % (g.device, h.device)
        for l, layer in enumerate(self.gatv2_layers):
            why = layer.infer_refusal(h, "GATv2 layer %d" % l)
            if why is not None:
                return why
        return None

    def _csc_ranges(self, g, node_chunk):
        """Destination ranges of the CSC path: [(row0, row1, edges)], contiguous, each at most max(node_chunk, csc_min_rows) rows
        and (a single longer row aside) csc_max_edges + one row's edges -- cut on the device, read by the host ONCE per call."""
        V, E = g.num_nodes(), g.num_edges()
        rows = max(int(node_chunk), int(self.csc_min_rows), 1)
        cuts = [torch.arange(0, V, rows, device=g.device, dtype=torch.int64), torch.tensor([V], device=g.device, dtype=torch.int64)]
        if E > self.csc_max_edges:
            targets = g.indptr[0] + torch.arange(1, E // int(self.csc_max_edges) + 1, device=g.device, dtype=torch.int64) * int(self.csc_max_edges)
            cuts.append((torch.searchsorted(g.indptr, targets, right=True) - 1).clamp_(0, V))      # the last row starting at or before a target
        cuts = torch.unique(torch.cat(cuts))                                                      # (sorted)
        both = torch.stack([cuts, g.indptr[cuts]]).tolist()                                       # the call's one host read
        ranges = [(r0, r1, e1 - e0) for r0, r1, e0, e1 in zip(both[0][:-1], both[0][1:], both[1][:-1], both[1][1:])]
        if any(e >= 2 ** 31 for _, _, e in ranges):
            raise NotImplementedError("GATv2.inference: a node with 2^31 or more in-edges is beyond the CSC path")
        return ranges

    def _inference_csc(self, g, h, node_chunk):
        """Per layer: fc_src (and a Linear res_fc) ONCE over all rows, then one launch pair per destination range off the graph's
        own indptr / indices -- finished rows (residual, ELU, flatten) out of the message-passing kernel; the last layer's head
        mean is one glue launch per range."""
        from .nn import gat_glue, gat_infer_state
        ranges = self._csc_ranges(g, node_chunk)
        state = gat_infer_state(h.device)
        V, n = g.num_nodes(), len(self.gatv2_layers)
        for l, layer in enumerate(self.gatv2_layers):
            H, D = layer._num_heads, layer._out_feats
            feat_src, res = layer.infer_transform(h)
            last = l == n - 1
            y = torch.empty(V, D if last else H * D, dtype=torch.bfloat16, device=h.device)
            rows = torch.empty(max(r1 - r0 for r0, r1, _ in ranges), H * D, dtype=torch.bfloat16, device=h.device) if last else None
            for r0, r1, edges in ranges:
                out = rows[: r1 - r0] if last else y[r0:r1]
                layer.infer_rows(g, r0, r1, edges, feat_src, res, out, state)
                if last:
                    y[r0:r1] = gat_glue(out, None, H, D, head_mean=True)[0]                         # :282-285
            del feat_src, res
            h = y
            g.ndata["h"] = h
        err = int(state["err"].item())
        if err:
            from . import _lib
            raise RuntimeError("GATv2.inference (csc): error 0x%x (%s)" % (err, _lib.err_string(err)))
        return h

    @torch.no_grad()
    def inference(self, g, device=None, batch_size=128, use_uva=False, num_workers=0, node_chunk=4096, path="auto"):
        """model.py:236-289.  Every output row depends only on its own in-edges (edge softmax is per destination), so the
        nodes are walked in contiguous ranges instead of the reference loader's ``batch_size``; the rows are the same.

        ``path="blocks"``: the full-neighbour block of ``node_chunk`` nodes at a time through the layers' ``forward``.
        ``path="csc"``: straight off the graph's CSC -- each layer's transforms once over all nodes, one
        forward-only message-passing launch per destination range; ``node_chunk`` only sizes the ranges (with the floor
        ``csc_min_rows``) and never changes the result.  Raises NotImplementedError naming the reason when it cannot run.
        ``path="auto"``: "csc" for a ``transforms="tile"`` model within the CSC path's limits, "blocks" otherwise.
        The path taken is left in ``last_inference_path``."""
        if path not in self.INFERENCE_PATHS:
            raise ValueError("path must be one of %r, not %r" % (self.INFERENCE_PATHS, path))
        h = g.ndata["features"].bfloat16()
        if path != "blocks":
            why = self.csc_refusal(g, h)
            if path == "csc" and why is not None:
                raise NotImplementedError(why)
            path = "csc" if (why is None and (path == "csc" or self.transforms in TILE_KINDS)) else "blocks"
        was_training = self.training
        self.eval()                                                                                            # :265
        try:
            if path == "csc":
                h = self._inference_csc(g, h, int(node_chunk))
            else:
                n = len(self.gatv2_layers)
                h = _blockwise_inference(self.gatv2_layers, g, h, int(node_chunk),
                                         lambda l, out: out.flatten(1) if l < n - 1 else out.mean(1))          # :282-285
        finally:
            self.train(was_training)
        self.last_inference_path = path
        return h
