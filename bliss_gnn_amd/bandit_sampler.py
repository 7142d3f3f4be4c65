"""EXP3-bandit LADIES samplers on MI355X -- same names, constructor arguments and call sites as the
reference's ``bandit_sampler.py`` so that ``train_lightning.py:358-370, 469-471`` work unchanged:

    sampler = PoissonBanditLadiesSampler(fanouts, importance_sampling=..., node_embedding='features',
                                         num_steps=..., eta=..., model=...)
    input_nodes, output_nodes, blocks = sampler.sample_blocks(g, seed_nodes)
    ...forward / backward / optimiser step...
    sampler.exp3(blocks, g)

The bodies are hand-written gfx950 kernels behind the C ABI of include/bliss_gnn.h.
"""
import ctypes as C

import torch

from . import _lib
from ._engine import DrawState, LayerEngine, _Draw, _stream
from .graph import EID, NID, Graph, _publish, as_graph


def find_indices_in(a, b):
    """bandit_sampler.py:5-14 -- kept for API compatibility (the kernels never need it: seeds are
    local ids 0..S-1 by construction)."""
    b_sorted, indices = torch.sort(b)
    sorted_indices = torch.searchsorted(b_sorted, a)
    sorted_indices[sorted_indices >= indices.shape[0]] = 0
    return indices[sorted_indices]


def union(*arrays):
    """bandit_sampler.py:16-18."""
    return torch.unique(torch.cat(arrays))


def normalized_edata(g: Graph, weight=None):
    """bandit_sampler.py:20-27 with weight=None: ``w_e = 1 / indeg(dst(e))`` in bf16, by edge id."""
    if weight is not None:
        raise NotImplementedError("only the weight=None form is used by the reference (train_lightning.py:359,362)")
    w_pos = torch.empty(g.num_edges(), dtype=torch.bfloat16, device=g.device)
    cg = _lib.Graph(g.indptr.data_ptr(), g.indices.data_ptr(), 0, g.num_nodes(), g.num_edges())
    _lib.check(_lib.lib.bliss_normalized_edata(C.byref(cg), w_pos.data_ptr(), _stream()), "bliss_normalized_edata")
    return g.by_edge_id(w_pos)


class BlockSampler:
    """The part of ``dgl.dataloading.BlockSampler`` the DataLoader relies on."""

    def __init__(self, *args, **kwargs):
        pass

    def sample(self, g, seed_nodes, exclude_eids=None):
        return self.sample_blocks(g, seed_nodes, exclude_eids=exclude_eids)


class DeviceDraw:
    """The ``draw=`` keyword of the two multinomial samplers.  ``"host"`` (default): ``torch.multinomial`` on the host, the
    reference's draw, one sync per layer.  ``"device"``: the keyed exponential race of csrc/mn_draw.hip
    -- no host round trip, so ``sample_blocks_static`` exists and the sampler can run inside a captured train step; the
    draw is a function of (seed, draw step, layer, node id) and consumes nothing from torch's generator.
    (fit.NeighborSampler shares the keyword and the draw state: its device draw is csrc/neighbor.hip, keyed by the edge.)

    The two Poisson samplers share the keyword.  ``"host"`` (default): the Bernoulli draw against torch's
    CPU MT19937 stream, regenerated on the device -- the reference's bits, at the price of the host staging the generator state
    around every step.  ``"device"``: the keyed Bernoulli draw of bliss_poisson_select_keyed -- candidate ``nid`` of sampling
    layer n is kept iff ``keyed_uniform(seed, draw step, n, nid) < P``; no generator, no staging, so a captured train step runs
    free.  ``layer_dependency=True`` (device draw only): layer 0's variate for every layer, i.e. one variate per node and step.

    ``"device-replace"`` (the multinomial samplers only): the reference's ``replace=True`` on the device --
    ``min(num, C)`` keyed categorical draws WITH replacement over the importances (csrc/replace_draw.hip, integers only), the
    duplicates dropped by the union as the reference drops them.  It sets ``draw = "device"`` and ``replace = True``: everything
    that holds for ``draw="device"`` holds for it."""

    _NO_STATIC = "the multinomial draw is torch.multinomial on the host: no static-shape variant (use draw='device')"

    def _init_draw(self, draw, replace, layer_dependency=False):
        if draw == "device-replace":
            if self._poisson:
                raise ValueError("draw='device-replace' belongs to the multinomial samplers: a Poisson draw has no replacement")
            draw, replace = "device", True
        elif draw not in ("host", "device"):
            raise ValueError("draw must be 'host', 'device' or 'device-replace', not %r" % (draw,))
        elif draw == "device" and replace:
            raise NotImplementedError("draw='device' is the draw without replacement; the device draw with replacement is "
                                      "draw='device-replace' (replace=True otherwise needs draw='host')")
        if layer_dependency and not (self._poisson and draw == "device"):
            raise ValueError("layer_dependency=True belongs to the Poisson samplers' keyed draw (draw='device')")
        self.draw = draw
        self.replace = bool(replace)
        self.layer_dependency = bool(layer_dependency)
        self._draw_init, self._draw_state = (None, 0), None

    def reset_draw(self, seed=None, step=0):
        """Set the draw state: ``seed`` (None = ``torch.initial_seed()``, taken at first use) and the step counter."""
        self._draw_init, self._draw_state = (seed, int(step)), None

    def draw_step(self):
        """The step counter (one sync): how many sampler calls have drawn since the state was set, plus its start."""
        return self._draw_init[1] if self._draw_state is None else self._draw_state.step()

    def _draw_state_on(self, device):
        if self.draw != "device":
            return None
        if self._draw_state is None:
            seed, step = self._draw_init
            self._draw_state = DrawState(torch.initial_seed() if seed is None else seed, step, device)
        return self._draw_state

    # -- the engine: one per graph, of the kind of layer this sampler's constructor arguments fix (_engine.KINDS) -------------
    def _kind(self):
        if self._poisson:
            return "poisson_keyed" if self.draw == "device" else "stream"
        if self.draw != "device":
            return "multinomial_host"
        return "multinomial_replace" if self.replace else "multinomial"

    def _graph(self, g):
        """The bliss Graph behind ``g`` (a DGLGraph-like object is converted once and cached, graph.as_graph)."""
        return as_graph(g, self.__dict__.setdefault("_graphs", {}))

    def _bind(self, g):
        g = self._graph(g)
        if self._engine is None or self._engine.g is not g:
            self._engine = LayerEngine(g, self._kind())
        return self._engine

    def _draw_on(self, device, prob=None, iterations=0):
        """The engine's per-call record."""
        return _Draw(self._draw_state_on(device), prob, self.layer_dependency, iterations)


class BanditLadiesSampler(DeviceDraw, BlockSampler):
    """bandit_sampler.py:29-367.  ``select_neighbors`` (:84-99) is ``torch.multinomial`` on the device-computed
    importances, drawn on the host (one sync per layer, like the reference), or with ``draw="device"`` the keyed draw on
    the device (DeviceDraw)."""

    _poisson = False

    def __init__(self, nodes_per_layer, importance_sampling=True, weight="w", out_weight="edge_weights",
                 node_embedding="nfeat", node_prob="node_prob", replace=False, eta=0.4, num_steps=5000,
                 model="sage", *, draw="host", layer_dependency=False):
        super().__init__()
        self._init_draw(draw, replace, layer_dependency)
        self.nodes_per_layer = nodes_per_layer
        self.importance_sampling = importance_sampling
        self.edge_weight = weight
        self.output_weight = out_weight
        self.node_prob = node_prob
        self.node_embedding = node_embedding
        self.eta = eta
        self.T = num_steps
        self.model = model
        self.eps = 0.9999
        self.delta = 0.01                      # bandit_sampler.py:233
        self._delta_f = float(torch.tensor(self.delta, dtype=torch.float32))
        self._w_pos = None                     # exp3 weights [L, |E|] bf16 in CSC-position order
        self._row_sum = None                   # exact row sums, int64 [L, 3 * 32 replicas]
        self._engine = None

    def _mode(self):
        return _lib.MODE_BANDIT | (0 if self.importance_sampling else _lib.MODE_UNIFORM_NODES)

    # -- state ------------------------------------------------------------------------------
    def _fields(self):
        return [("edata", self.output_weight, "_edge_weights"), ("edata", "q_ij", "_q"), ("srcdata", self.node_prob, "_node_prob")]

    def _ensure_weights(self, g):
        if self._w_pos is None:                                         # bandit_sampler.py:342-343
            L, E = len(self.nodes_per_layer), g.num_edges()
            self._w_pos = torch.ones(L, E, dtype=torch.bfloat16, device=g.device)
            rs = torch.zeros(L, 96, dtype=torch.int64, device=g.device)      # 32 replicas of three limbs, summed by the readers
            rs[:, 2] = E                                                # sum of E ones = E * 2^64
            self._row_sum = rs
            self._scratch = torch.zeros(L, 98, dtype=torch.int64, device=g.device)
            self._err = torch.zeros(1, dtype=torch.int32, device=g.device)
            self._norms = torch.zeros(L, dtype=torch.bfloat16, device=g.device)

    @property
    def exp3_weights(self):
        """[L, |E|] bf16 indexed by EDGE ID like the reference's attribute (bandit_sampler.py:43)."""
        if self._w_pos is None:
            return None
        return self._engine.g.by_edge_id(self._w_pos)

    @exp3_weights.setter
    def exp3_weights(self, value):
        if value is None:
            self._w_pos = None
            return
        g = self._engine.g
        value = value.to(torch.bfloat16)
        # bliss_row_sum has no error word: what the exact row sum cannot hold (exp3.hip, row_digits) is refused here, where
        # outside weights enter the state (a set-up path: the sync is fine)
        v = value.float()
        if not bool((torch.isfinite(v) & (v >= 0) & (v < 2.0 ** 24)).all()):
            raise ValueError("exp3_weights must be finite, non-negative and below 2**24")
        self._w_pos = g.by_position(value).contiguous().clone()
        L = self._w_pos.shape[0]
        self._row_sum = torch.zeros(L, 96, dtype=torch.int64, device=g.device)
        self._scratch = torch.zeros(L, 98, dtype=torch.int64, device=g.device)
        self._err = torch.zeros(1, dtype=torch.int32, device=g.device)
        self._norms = torch.zeros(L, dtype=torch.bfloat16, device=g.device)
        for l in range(L):
            _lib.check(_lib.lib.bliss_row_sum(self._w_pos[l].data_ptr(), g.num_edges(), self._row_sum[l].data_ptr(),
                                              _stream()), "bliss_row_sum")

    # -- sampling ---------------------------------------------------------------------------
    def sample_blocks(self, g, seed_nodes, exclude_eids=None, uniforms=None):
        """bandit_sampler.py:341-367.  ``uniforms``: optional list (sampling order, last layer first)
        of fp32 vectors used instead of the global CPU generator."""
        g = self._graph(g)
        eng = self._bind(g)
        self._ensure_weights(g)
        output_nodes = seed_nodes
        order = list(reversed(range(len(self.nodes_per_layer))))          # :350
        rows, fan = [self._w_pos[b] for b in order], [self.nodes_per_layer[b] for b in order]
        if self._poisson:
            blks = eng.sample_blocks(rows, seed_nodes, fan, self._mode(), self.eta, self.eps, uniforms,
                                     draw_state=self._draw_state_on(g.device), layer_dependency=self.layer_dependency)
        else:                                                             # select_neighbors :84-99 (torch.multinomial)
            blks = eng.sample_blocks_multinomial(rows, seed_nodes, fan, self._mode(), self.eta, self.replace, draw=self.draw,
                                                 draw_state=self._draw_state_on(g.device))
        return _publish(blks, output_nodes, self._fields())                 # :324-328, :364-367

    def sample_blocks_static(self, g, seed_nodes, slot=0, chain_rng=False, external_rng=False, part=None, last_block=True, ready_flag=0,
                             n_live_dev=None):
        """sample_blocks with capacity-padded (static-shape) blocks and no host round trip: everything is only
        ENQUEUED, so the whole train step can be recorded into a HIP graph.  Call ``engine.stage_rng_from_torch()``
        before and ``finish_static()`` after the stream has been synchronised.  Padded rows / edges are inert:
        ids past the true K point at node 0 and no edge references them; edges past the true B are ignored by
        every kernel (the true counts live on the device)."""
        if not self._poisson and self.draw != "device":
            raise NotImplementedError(self._NO_STATIC)
        g = self._graph(g)
        eng = self._bind(g)
        self._ensure_weights(g)
        order = list(reversed(range(len(self.nodes_per_layer))))
        blks = eng.enqueue_static([self._w_pos[b] for b in order], seed_nodes, [self.nodes_per_layer[b] for b in order],
                                  self._mode(), self.eta, self.eps, slot=slot, chain_rng=chain_rng, external_rng=external_rng, part=part,
                                  last_block=last_block, ready_flag=ready_flag, n_live_dev=n_live_dev, draw=self._draw_on(g.device))
        return _publish(blks, seed_nodes, self._fields())

    def finish_static(self, slot=0, commit=True):
        return self._engine.finish(slot, commit)

    # -- bandit update ----------------------------------------------------------------------
    def exp3(self, mfgs, g, apply=True, factors=None, bounds=None):
        """bandit_sampler.py:251-267: rewards + weight update + L1 renormalisation, per block.

        ``apply=False`` (multi-GPU replicas, bliss_gnn_amd/dist.py) only computes the rewards and, into
        ``factors[idx]`` (bf16 [B]), the multiplicative updates; ``apply_updates`` then applies every
        rank's updates in rank order.  ``bounds[idx]``: process at most that many edges of block idx (the length of
        ``factors[idx]``); a longer block is flagged (error bit 8)."""
        g = self._graph(g)
        self._bind(g)
        st = _stream()
        edge_w_pos = g.edata_by_position(self.edge_weight)
        cg = self._engine.c_graph
        fused = apply and factors is None and len(mfgs) <= 8         # all blocks in two launches (bliss_exp3_step)
        keep = []                                                    # (tensors the launch reads must outlive the loop)
        recs = (_lib.Exp3Block * len(mfgs))() if fused else None
        for idx, mfg in enumerate(mfgs):
            B = mfg.num_edges()
            alpha = None
            if self.model == "gat":                                    # calculate_alpha, bandit_sampler.py:146-154
                a_ij = mfg.edata["a_ij"].detach()
                a_ij = a_ij.bfloat16().contiguous() if a_ij.dtype != torch.bfloat16 else a_ij.contiguous()
                alpha = torch.empty(B, dtype=torch.bfloat16, device=g.device)
                _lib.check(_lib.lib.bliss_gat_alpha(mfg.indptr.data_ptr(), mfg.num_dst_nodes(), mfg.edata["q_ij"].data_ptr(),
                                                    a_ij.data_ptr(), alpha.data_ptr(), self._err.data_ptr(), st), "bliss_gat_alpha")
            n_edges_ptr = mfg._counts_dev.data_ptr() + 16             # LayerCounts::B, already on the device
            rewards = torch.empty(B, dtype=torch.bfloat16, device=g.device)
            en = mfg.srcdata["embed_norm"]
            if en.dtype != torch.bfloat16:
                en = en.bfloat16()
            en = en.contiguous()
            if fused:
                keep.append((alpha, en))
                recs[idx] = _lib.Exp3Block(self._w_pos[idx].data_ptr(), self._row_sum[idx].data_ptr(), self._scratch[idx].data_ptr(),
                                           self._norms[idx:].data_ptr(), mfg.indptr.data_ptr(), mfg.src.data_ptr(), mfg.dst.data_ptr(),
                                           mfg.pos.data_ptr(), mfg.edata["q_ij"].data_ptr(), mfg.srcdata[self.node_prob].data_ptr(),
                                           en.data_ptr(), 0 if alpha is None else alpha.data_ptr(), mfg.dstdata[NID].data_ptr(),
                                           n_edges_ptr, rewards.data_ptr(), B)
                mfg.edata["rewards"] = rewards                          # :193
                continue
            _lib.check(_lib.lib.bliss_exp3_update(
                C.byref(cg), edge_w_pos.data_ptr(), self._w_pos[idx].data_ptr(), self._row_sum[idx].data_ptr(),
                mfg.indptr.data_ptr(), mfg.src.data_ptr(), mfg.dst.data_ptr(), mfg.pos.data_ptr(),
                mfg.edata["q_ij"].data_ptr(), mfg.srcdata[self.node_prob].data_ptr(), en.contiguous().data_ptr(),
                0 if alpha is None else alpha.data_ptr(), mfg.dstdata[NID].data_ptr(), mfg.num_dst_nodes(),
                n_edges_ptr, B if bounds is None else min(B, int(bounds[idx])), self._delta_f, rewards.data_ptr(),
                0 if factors is None else factors[idx].data_ptr(), int(apply), self._err.data_ptr(), st), "bliss_exp3_update")
            mfg.edata["rewards"] = rewards                              # :193
            if not apply:
                continue
            _lib.check(_lib.lib.bliss_exp3_normalize(self._w_pos[idx].data_ptr(), g.num_edges(),
                                                     self._row_sum[idx].data_ptr(), self._scratch[idx].data_ptr(),
                                                     self._norms[idx:].data_ptr(), st), "bliss_exp3_normalize")
        if fused and len(mfgs):
            _lib.check(_lib.lib.bliss_exp3_step(C.byref(cg), edge_w_pos.data_ptr(), recs, len(mfgs), self._delta_f,
                                                self._err.data_ptr(), st), "bliss_exp3_step")

    def apply_updates(self, idx, pos, factor, g, n_dev=None):
        """w[pos] *= factor on layer ``idx`` (positions unique within one call), bandit_sampler.py:248.  ``n_dev``: optional
        int32 device tensor holding how many leading entries are valid (capacity-padded lists, graph capture)."""
        bound = int(pos.numel())
        if bound == 0:
            return
        if n_dev is None:
            n_dev = torch.tensor([bound], dtype=torch.int32, device=pos.device)
        _lib.check(_lib.lib.bliss_exp3_apply(self._w_pos[idx].data_ptr(), self._row_sum[idx].data_ptr(), pos.data_ptr(),
                                             factor.data_ptr(), n_dev.data_ptr(), bound, self._err.data_ptr(), _stream()),
                   "bliss_exp3_apply")

    def apply_updates_ranks(self, block_ids, gathered, rank_stride, n_ranks, pos_off, factor_off_bf16, count_off, bounds):
        """apply_updates for the packed (position, factor, count) lists of ``n_ranks`` ranks and several blocks in ONE launch,
        rank after rank (bliss_exp3_apply_ranks; ``gathered`` int32 = the all-gathered buffers, offsets per block inside one
        rank's buffer).  Same bits as the corresponding apply_updates calls in rank order."""
        m = _lib.Exp3RankLists()
        for j, idx in enumerate(block_ids):
            m.w_pos[j], m.row_sum[j] = self._w_pos[idx].data_ptr(), self._row_sum[idx].data_ptr()
            m.pos_off_words[j], m.factor_off_bf16[j], m.count_off_words[j], m.bound[j] = pos_off[j], factor_off_bf16[j], count_off[j], bounds[j]
        m.n_blocks, m.n_ranks, m.rank_stride_words = len(block_ids), int(n_ranks), int(rank_stride)
        if getattr(self, "_apply_bar", None) is None:
            self._apply_bar = torch.zeros(2, dtype=torch.int32, device=gathered.device)
        _lib.check(_lib.lib.bliss_exp3_apply_ranks(C.byref(m), gathered.data_ptr(), self._apply_bar.data_ptr(), self._err.data_ptr(),
                                                   _stream()), "bliss_exp3_apply_ranks")

    def normalize(self, idx, g):
        """F.normalize(self.exp3_weights[idx], p=1, dim=0), bandit_sampler.py:249 (bit-exact, skipped on the
        device when the bf16 norm is 1.0)."""
        _lib.check(_lib.lib.bliss_exp3_normalize(self._w_pos[idx].data_ptr(), g.num_edges(), self._row_sum[idx].data_ptr(),
                                                 self._scratch[idx].data_ptr(), self._norms[idx:].data_ptr(), _stream()),
                   "bliss_exp3_normalize")

    def check_errors(self):
        """Raise if any exp3 kernel flagged a non-finite weight (one sync; call off the hot path)."""
        bits = int(self._err.item()) | int((self._scratch[:, 0] >> 20).max().item())
        if bits:
            raise RuntimeError(f"exp3 kernel error 0x{bits:x}: {_lib.err_string(bits)}")


class PoissonBanditLadiesSampler(BanditLadiesSampler):
    """bandit_sampler.py:369-425.  ``draw="device"`` (with ``layer_dependency``): the keyed Bernoulli draw, DeviceDraw."""

    _poisson = True
