"""The experiment protocol around the hot path: what ``train_lightning.py`` asks of
pytorch_lightning, reduced to plain loops -- Lightning / torchmetrics / tensorboard_reducer are absent on this platform.

  * ``MultiLayerFullNeighborSampler`` / ``NeighborSampler``: the two non-LADIES ``--sampler`` choices
    (train_lightning.py:349-357).  (With them the reference's models fail at ``block.edata["edge_weights"]``,
    model.py:321-329 -- DGL's own samplers attach no such field -- so they are baselines here, with unit weights.)
    ``NeighborSampler(..., draw="device")``: the keyed per-column draw of csrc/neighbor.hip, graph-capturable;
    with ``prob=`` the weighted draw of csrc/neighbor_w.hip.
  * ``BanditNeighborSampler``: the node-wise bandit sampler (GCN-BS) -- that weighted draw over the EXP3 edge probabilities, with
    ``BanditLadiesSampler``'s state and reward update.
  * ``LaborSampler``: LABOR-0, the node-wise baseline with one random variate per SOURCE vertex shared by all seeds of a layer
    (csrc/labor.hip) -- the sampler the reference's training script was derived from and dropped.
    ``ImportanceLaborSampler``: LABOR-i, the same draw after i fixed-point iterations over per-vertex importances
    (csrc/labor_is.hip).
    ``WeightedLaborSampler``: LABOR-0 with edge probabilities (DGL's ``prob=``), and ``BanditLaborSampler``: the same draw over the
    EXP3 edge probabilities with ``BanditLadiesSampler``'s state and reward update (csrc/labor_w.hip).
  * ``fit``: epochs of TrainStep, ``StepLR(gamma=0.01, step_size=5)`` stepped per epoch (:205-216), validation with the same
    sampler (:179-203, :410-422), best-``val_acc`` checkpoint (:620-625), early stop on ``val_acc_target`` / patience
    (:627-634), then the best checkpoint reloaded for the layer-wise full-neighbour inference and the Final Accuracy of the
    three splits (:662-705).  Accuracy = micro-F1 (:68-70).
  * ``k_runs``: mean / std of the final metrics over repeated runs (:711-733).
"""
import copy
import math
import os

import torch

from . import _lib
from .bandit_sampler import BanditLadiesSampler, BlockSampler, DeviceDraw
from .graph import NID, Block, _publish, as_graph
from .ladies_sampler import PoissonLadiesSampler
from .train import BatchLoader, GraphedEvalStep, GraphedTrainStep, TrainStep, _inputs, _keep_static_caps, _rng_kept


# ----------------------------------------------------------------------------------------------- baseline samplers
class MultiLayerFullNeighborSampler(BlockSampler):
    """``dgl.dataloading.MultiLayerFullNeighborSampler(n_layers)`` (train_lightning.py:349-350): every in-edge of every seed,
    layer after layer.  Built on the LADIES kernels with a fanout no candidate set can exceed: the Poisson scale then takes
    its early-out (everything kept, P = 1, ladies_sampler.py:147-148); the edge weights are then set to exactly 1 (the
    Horvitz-Thompson weight bf16(1/deg) * deg is 1 only up to a bf16 rounding) -- the plain mean the reference's inference
    uses (model.py:347-349)."""

    def __init__(self, num_layers):
        super().__init__()
        self.num_layers = int(num_layers)
        self.nodes_per_layer = [-1] * self.num_layers          # (-1 = every in-neighbour, DGL's convention for "no fanout")
        self._inner = None

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        g = as_graph(g, self.__dict__.setdefault("_graphs", {}))
        if self._inner is None:
            self._inner = PoissonLadiesSampler([g.num_nodes() + 1] * self.num_layers)
        if "w" not in g.edata:
            from .bandit_sampler import normalized_edata
            g.edata["w"] = normalized_edata(g)
        inp, outp, blocks = self._inner.sample_blocks(g, seed_nodes)
        for b in blocks:
            b.edata["edge_weights"] = torch.ones_like(b.edata["edge_weights"])
        return inp, outp, blocks


class NeighborSampler(DeviceDraw, BlockSampler):
    """``dgl.dataloading.NeighborSampler(fanouts)`` (train_lightning.py:351-357): up to ``fanout`` in-neighbours per
    destination, uniformly without replacement, per layer.  No parity claim (DGL draws with its own RNG).

    ``draw="host"`` (default): a baseline outside the hot path -- device tensor ops (random key per frontier edge, rank inside
    its column), its own torch generator, one host read per layer.  ``draw="device"``: the keyed per-column draw of
    csrc/neighbor.hip -- a function of (seed, draw step, layer, CSC position), no host round trip, so
    ``sample_blocks_static`` exists and the sampler runs inside a captured train step; ``seed`` starts its draw state
    (``reset_draw`` / ``draw_step`` as for the multinomial samplers) and no torch generator is touched.

    ``prob`` (DGL's keyword; ``draw="device"`` only, the host draw raises): unnormalised edge probabilities, a tensor [|E|] by EDGE ID
    or the name of an entry of ``g.edata``, converted to bf16 by CSC position once per graph.  The draw is then the weighted one of
    csrc/neighbor_w.hip (a keyed exponential race per column, an edge with probability <= 0 taken only as
    a filler); ``edge_weights`` carry the Hajek weights under the mean aggregation and ``edata["q_ij"]`` the probabilities.

    ``replace=True`` (DGL's keyword; ``draw="device"`` only, the host draw raises): every destination with an in-edge gets exactly
    ``fanout`` edges, drawn WITH replacement -- also when it has fewer in-edges than that -- uniformly or with ``prob``: the keyed
    categorical draw of csrc/replace_draw.hip (integers only, a function of seed, draw step, layer, the
    destination's node id and the draw's index).  Repeats are separate block edges; with ``prob`` the weights are
    ``(1 / q_e) * fanout / sum (1 / q_e')`` over the column's edges, the exact per-draw importance weights.  Fanouts are limited to
    ``NeighborSampler.MAX_REPLACE_FANOUT``."""

    _poisson = False                                       # (DeviceDraw's Poisson / replace checks have no subject here)
    MAX_REPLACE_FANOUT = _lib.NR_MAX_FANOUT

    def __init__(self, fanouts, seed=0, *, draw="host", prob=None, replace=False, **_ignored):
        super().__init__()
        if draw not in ("host", "device"):
            raise ValueError("draw must be 'host' or 'device', not %r" % (draw,))
        self._init_draw(draw, False)
        if prob is not None and draw != "device":
            raise NotImplementedError("NeighborSampler: edge probabilities (prob=) need draw='device'; the host draw is uniform")
        if replace and draw != "device":
            raise NotImplementedError("NeighborSampler: replace=True needs draw='device'; the host draw is without replacement")
        if replace and any(int(f) == 0 or int(f) > self.MAX_REPLACE_FANOUT for f in fanouts):
            raise ValueError("NeighborSampler(replace=True): fanouts must be negative (whole columns) or 1 .. %d, got %r"
                             % (self.MAX_REPLACE_FANOUT, list(fanouts)))
        self.replace = bool(replace)
        self.prob, self._prob_pos = prob, None
        self._draw_init = (seed, 0)
        self.fanouts, self.nodes_per_layer = list(fanouts), list(fanouts)
        self._seed, self._gen = seed, None
        self._engine = None

    # -- draw="device" ----------------------------------------------------------------------------------------------
    def _kind(self):
        return "neighbor_replace" if self.replace else "neighbor" if self.prob is None else "wneighbor"

    def _nb_prob(self, eng):
        """The engine's probability record of the weighted draw (None without ``prob``); bf16 by position, once per graph."""
        if self.prob is None:
            return None
        g = eng.g
        if self._prob_pos is None or self._prob_pos[0] is not g:
            p = g.edata[self.prob] if isinstance(self.prob, str) else torch.as_tensor(self.prob)
            if p.dim() != 1 or p.numel() != g.num_edges():
                raise ValueError("NeighborSampler: prob must hold one value per edge, by edge id")
            self._prob_pos = (g, g.by_position(p.to(g.device).to(torch.bfloat16)).contiguous())
        return eng.neighbor_prob(self._prob_pos[1])

    def _fields(self):
        return [("edata", "edge_weights", "_edge_weights")] + ([("edata", "q_ij", "_q")] if self.prob is not None else [])

    def _blocks(self, blks, seed_nodes):
        return _publish(blks, seed_nodes, self._fields())

    def sample_blocks_static(self, g, seed_nodes, slot=0, **split):
        """sample_blocks with capacity-padded blocks, only ENQUEUED (the contract of the LADIES samplers' method of this name);
        whole calls only: any split / external-generator keyword raises."""
        if self.draw != "device":
            raise NotImplementedError("the host draw reads sizes back per layer: no static-shape variant (use draw='device')")
        eng = self._bind(g)
        fan = list(reversed(self.fanouts))
        return self._blocks(eng.enqueue_static(None, seed_nodes, fan, 0, 0.0, slot=slot,
                                               draw=self._draw_on(eng.g.device, self._nb_prob(eng)), **split), seed_nodes)

    def finish_static(self, slot=0, commit=True):
        return self._engine.finish(slot, commit)

    def check_errors(self):
        pass                                               # no bandit state; sampler errors surface through finish()

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        g = as_graph(g, self.__dict__.setdefault("_graphs", {}))
        if self.draw == "device":
            eng = self._bind(g)
            blks = eng.sample_blocks_neighbor(seed_nodes, list(reversed(self.fanouts)), self._draw_state_on(g.device),
                                              nb_prob=self._nb_prob(eng), replace=self.replace)
            return self._blocks(blks, seed_nodes)
        dev = g.device
        if self._gen is None:
            self._gen = torch.Generator(device=dev)
            self._gen.manual_seed(self._seed)
        blocks, seeds = [], seed_nodes.to(torch.int32)
        for fanout in reversed(self.fanouts):
            s64 = seeds.long()
            start, deg = g.indptr[s64], g.indptr[s64 + 1] - g.indptr[s64]
            S, E = s64.numel(), int(deg.sum())
            dst = torch.repeat_interleave(torch.arange(S, device=dev), deg, output_size=E)
            seg = torch.cumsum(deg, 0) - deg
            pos = start[dst] + (torch.arange(E, device=dev) - seg[dst])
            key = dst.double() + torch.rand(E, generator=self._gen, device=dev, dtype=torch.float64) * 0.999999
            order = torch.argsort(key)
            rank = torch.arange(E, device=dev) - seg[dst[order]]
            keep = order[rank < fanout]
            keep = keep[torch.argsort(keep)]                                   # back to column order
            e_dst, e_pos = dst[keep], pos[keep]
            src_g = g.indices[e_pos].long()
            local = torch.full((g.num_nodes(),), -1, dtype=torch.int64, device=dev)
            local[s64] = torch.arange(S, device=dev)
            new = torch.unique(src_g[local[src_g] < 0])
            local[new] = S + torch.arange(new.numel(), device=dev)
            src_nid = torch.cat([s64, new]).to(torch.int32)
            kd = torch.bincount(e_dst, minlength=S)
            indptr = torch.zeros(S + 1, dtype=torch.int32, device=dev)
            indptr[1:] = torch.cumsum(kd, 0)
            eid = g.eid[e_pos] if g.eid is not None else e_pos.to(torch.int32)
            blk = Block(g, src_nid.numel(), S, indptr, local[src_g].to(torch.int32), e_dst.to(torch.int32), e_pos.to(torch.int32), eid, src_nid)
            blk.edata["edge_weights"] = torch.ones(keep.numel(), dtype=torch.bfloat16, device=dev)
            blocks.insert(0, blk)
            seeds = src_nid
        return blocks[0].srcdata[NID], seed_nodes, blocks


class _BanditNodeWise(BanditLadiesSampler):
    """What the two node-wise bandit samplers share: a weighted node-wise draw over the EXP3 edge probabilities, layer ``b``'s row
    of the EXP3 weights for block ``b``."""

    def _fields(self):
        return super()._fields() + ([("edata", "p_ij", "_p")] if self._kind() == "wlabor" else [])

    def _sample(self, g, seed_nodes, static, **kw):
        g = self._graph(g)
        eng = self._bind(g)
        self._ensure_weights(g)
        order = list(reversed(range(len(self.fanouts))))   # sampling order: the last block first
        fan = [self.fanouts[b] for b in order]
        prob = eng.neighbor_prob([self._w_pos[b] for b in order], eta=self.eta)
        ds = self._draw_state_on(g.device)
        if static:
            blks = eng.enqueue_static(None, seed_nodes, fan, 0, 0.0, draw=self._draw_on(g.device, prob), **kw)
        elif self._kind() == "wlabor":
            blks = eng.sample_blocks_labor(seed_nodes, fan, ds, self.layer_dependency, lb_prob=prob)
        else:
            blks = eng.sample_blocks_neighbor(seed_nodes, fan, ds, nb_prob=prob)
        return _publish(blks, seed_nodes, self._fields())

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        return self._sample(g, seed_nodes, False)


class BanditNeighborSampler(_BanditNodeWise):
    """The node-wise bandit sampler (Liu et al., "Bandit Samplers for Training GNNs", GCN-BS; BLISS is its layer-wise extension): up
    to ``fanout`` in-neighbours per destination, drawn without replacement with the EXP3 edge probabilities q_ij = eta / n_i +
    (1 - eta) * w_ij / sum_j w_ij -- the weighted draw of csrc/neighbor_w.hip in EXP3 mode, layer ``b``'s row
    of the EXP3 weights for block ``b``.  No parity claim: a defined mode restated by tests/wneighbor_ref.py.

    The EXP3 state (``exp3_weights`` [L, |E|] by edge id, exact row sums), ``exp3(mfgs, g)`` (also ``model="gat"``) and
    ``check_errors`` are ``BanditLadiesSampler``'s; blocks carry ``edge_weights`` (Hajek weights under the mean aggregation),
    ``q_ij`` and ``node_prob`` = 1.  Always ``draw="device"``: ``reset_draw`` / ``draw_step`` / ``sample_blocks_static`` /
    ``finish_static`` as ``NeighborSampler(draw="device")`` has them, it runs inside a captured train step, and the pipelined
    two-stream loop refuses it."""

    def __init__(self, fanouts, eta=0.4, num_steps=5000, model="sage", seed=0, replace=False, **_ignored):
        if replace:
            raise NotImplementedError("BanditNeighborSampler(replace=True): the EXP3 update rewrites w[pos] once per block edge and "
                                      "relies on a position occurring at most once per block; a draw with replacement repeats "
                                      "positions (NeighborSampler(draw='device', replace=True, prob=...) draws from fixed "
                                      "probabilities)")
        super().__init__(list(fanouts), eta=eta, num_steps=num_steps, model=model, draw="device")
        self.fanouts = list(fanouts)
        self._draw_init = (seed, 0)

    def _kind(self):
        return "wneighbor"                                  # (B exactly bounded: a column keeps at most fanout edges, as the uniform draw)

    def sample_blocks_static(self, g, seed_nodes, slot=0, **split):
        """sample_blocks with capacity-padded blocks, only ENQUEUED; whole calls only: any split / external-generator keyword
        raises."""
        return self._sample(g, seed_nodes, True, slot=slot, **split)


class LaborSampler(NeighborSampler):
    """``dgl.dataloading.LaborSampler(fanouts, importance_sampling=0)`` -- LABOR-0 (Balin & Catalyurek, "Layer-Neighbor Sampling"):
    per layer, one uniform variate r_u per SOURCE vertex shared by all seeds; the edge u -> s is kept iff r_u < fanout / deg(s).
    Per destination that is the neighbor sampler's expected edge count and estimator variance, out of far fewer distinct
    sources.  No parity claim (DGL draws with its own RNG): a defined mode, the keyed draw of csrc/labor.hip restated by
    tests/labor_ref.py.  Every kept edge of a column has the same inclusion probability, so the Hajek
    weight under the mean aggregation is exactly 1: unit ``edge_weights``.  A destination may keep no edge at all.

    There is no host path: ``draw`` is always ``"device"`` -- a function of (seed, draw step, layer, source node id), no host
    round trip, so ``sample_blocks_static`` exists and the sampler runs inside a captured train step (``reset_draw`` /
    ``draw_step`` / ``finish_static`` / ``check_errors`` as ``NeighborSampler(draw="device")`` has them); no torch generator is
    touched.  ``layer_dependency=True``: the same variate per vertex in all layers of a step.  Out of scope (raise):
    ``importance_sampling != 0`` (LABOR-i's fixed-point iterations), ``prob``, ``batch_dependency != 1``, ``edge_dir != "in"``.
    (LABOR-i is a class of its own: ``ImportanceLaborSampler``.)"""

    _iterations = 0                                         # (ImportanceLaborSampler: LABOR-i layers, csrc/labor_is.hip)

    def __init__(self, fanouts, edge_dir="in", prob=None, importance_sampling=0, layer_dependency=False, batch_dependency=1, seed=0,
                 **_ignored):
        if importance_sampling != 0:
            raise NotImplementedError("LaborSampler is LABOR-0: importance_sampling must be 0 (LABOR-i's importance iterations "
                                      "are out of scope)")
        if prob is not None:
            raise NotImplementedError("LaborSampler: edge probabilities (prob=) are out of scope")
        if batch_dependency != 1:
            raise NotImplementedError("LaborSampler: batch_dependency must be 1 (variates shared across batches are out of scope)")
        if edge_dir != "in":
            raise NotImplementedError("LaborSampler samples in-edges only (edge_dir='in')")
        super().__init__(fanouts, seed=seed, draw="device")
        self.layer_dependency = bool(layer_dependency)

    def _kind(self):
        return "labor"                                      # (B not exactly bounded: a column's kept count is data dependent)

    def sample_blocks_static(self, g, seed_nodes, slot=0, **split):
        """sample_blocks with capacity-padded blocks, only ENQUEUED; whole calls only: any split / external-generator keyword
        raises.  A step over its calibrated capacities is reported by ``finish_static``."""
        eng = self._bind(g)
        fan = list(reversed(self.fanouts))
        return self._blocks(eng.enqueue_static(None, seed_nodes, fan, 0, 0.0, slot=slot,
                                               draw=self._draw_on(eng.g.device, self._nb_prob(eng), self._iterations), **split), seed_nodes)

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        g = as_graph(g, self.__dict__.setdefault("_graphs", {}))
        eng = self._bind(g)
        blks = eng.sample_blocks_labor(seed_nodes, list(reversed(self.fanouts)), self._draw_state_on(g.device),
                                       self.layer_dependency, iterations=self._iterations, lb_prob=self._nb_prob(eng))
        return self._blocks(blks, seed_nodes)


class ImportanceLaborSampler(LaborSampler):
    """LABOR-i (Balin & Catalyurek, "Layer-Neighbor Sampling"; ``dgl.dataloading.LaborSampler(fanouts, importance_sampling=i)``):
    LABOR-0's one variate r_u per source vertex, with the edge u -> s kept iff r_u < c_s * pi_u, where the per-vertex importances
    pi come from ``iterations`` fixed-point iterations (pi_u <- the largest c_s * pi_u over the layer's edges out of u) and c_s
    is the scale at which column s keeps ``fanout`` edges in expectation.  Every destination's expected edge count stays
    ``fanout``; the set of distinct sources shrinks with every iteration.  No parity claim (DGL is not installable here and draws
    with its own RNG; its form also seems to clamp the per-edge probability at 1 inside the maximum -- from memory, unchecked): a
    defined mode in unsigned integers, csrc/labor_is.hip restated by tests/labor_is_ref.py.
    ``edge_weights`` are the Hajek weights under the mean aggregation, (1 / p_e) * k_s / sum over the column's kept edges of
    1 / p_e', exactly 1 in a column that is kept whole.

    Everything else is ``LaborSampler``'s: always the device draw, ``layer_dependency``, ``reset_draw`` / ``draw_step`` /
    ``sample_blocks_static`` / ``finish_static`` / ``check_errors``; it runs inside a captured train step.  ``iterations`` is a
    launch-time constant in 0 .. 8 (0 = LABOR-0 through these kernels); DGL's ``-1`` (iterate until convergence) is out of scope:
    a data-dependent launch count cannot be captured."""

    def __init__(self, fanouts, iterations=1, layer_dependency=False, seed=0, **_ignored):
        if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= int(iterations) <= 8:
            raise ValueError("ImportanceLaborSampler: iterations must be an integer in 0 .. 8, got %r" % (iterations,))
        super().__init__(fanouts, layer_dependency=layer_dependency, seed=seed)
        self.iterations = self._iterations = int(iterations)

    def _kind(self):
        return "labor_is"                                   # (also iterations = 0 runs csrc/labor_is.hip, not csrc/labor.hip)


class WeightedLaborSampler(LaborSampler):
    """``dgl.dataloading.LaborSampler(fanouts, prob=...)`` with ``importance_sampling=0``: LABOR-0's one variate r_u per source
    vertex, the edge u -> s kept iff r_u < p_us with p_us proportional to the edge's probability inside its column, scaled so
    that the column keeps ``fanout`` edges in expectation and clamped below 1 (the scale then rises for the other edges).  No
    parity claim: a defined mode in unsigned integers from the bf16 bits of the probabilities, csrc/labor_w.hip restated by
    tests/wlabor_ref.py.  A column with fewer than ``fanout`` edges of comparable weight (within about
    2^-8 of its largest) keeps fewer than ``fanout`` edges in expectation; an edge whose probability is not positive and finite, or
    below 2^-32 of the column's largest, is never kept unless the column is kept whole (DGL's behaviour; the weighted neighbor
    draw's filler rule does not apply).

    ``prob``: unnormalised edge probabilities, a tensor [|E|] by EDGE ID or the name of an entry of ``g.edata``, converted to bf16
    by CSC position once per graph.  Blocks carry ``edge_weights`` (the Hajek weights under the mean aggregation, from the true
    inclusion probabilities), ``edata["q_ij"]`` (the edge probabilities) and ``edata["p_ij"]`` (the inclusion probabilities, 1 in
    a column kept whole).  Everything else is ``LaborSampler``'s: always the device draw, ``layer_dependency``, ``reset_draw`` /
    ``draw_step`` / ``sample_blocks_static`` / ``finish_static`` / ``check_errors``; it runs inside a captured train step."""

    def __init__(self, fanouts, prob, layer_dependency=False, seed=0, **_ignored):
        if prob is None:
            raise ValueError("WeightedLaborSampler needs edge probabilities (prob=); without them it is LaborSampler")
        super().__init__(fanouts, layer_dependency=layer_dependency, seed=seed)
        self.prob = prob

    def _kind(self):
        return "wlabor"

    def _fields(self):
        return [("edata", "p_ij", "_p")] + super()._fields()


class BanditLaborSampler(_BanditNodeWise):
    """LABOR with learned edge probabilities: ``WeightedLaborSampler``'s draw over the EXP3 edge probabilities q_ij = eta / n_i +
    (1 - eta) * w_ij / sum_j w_ij -- csrc/labor_w.hip in EXP3 mode, layer ``b``'s row of the EXP3 weights for
    block ``b``.  Unlike ``BanditNeighborSampler``'s blocks, these shrink as the probabilities concentrate: one variate per source
    vertex is shared by all seeds of a layer.  No parity claim: a defined mode restated by tests/wlabor_ref.py.

    The EXP3 state (``exp3_weights`` [L, |E|] by edge id, exact row sums), ``exp3(mfgs, g)`` (also ``model="gat"``) and
    ``check_errors`` are ``BanditLadiesSampler``'s; blocks carry ``edge_weights`` (Hajek weights under the mean aggregation),
    ``q_ij`` (what the reward divides by), ``p_ij`` (the inclusion probabilities) and ``node_prob`` = 1.  Always ``draw="device"``:
    ``reset_draw`` / ``draw_step`` / ``sample_blocks_static`` / ``finish_static`` as ``LaborSampler`` has them, it runs inside a
    captured train step, and the pipelined two-stream loop refuses it."""

    def __init__(self, fanouts, eta=0.4, num_steps=5000, model="sage", layer_dependency=False, seed=0, replace=False, **_ignored):
        if replace:
            raise NotImplementedError("BanditLaborSampler(replace=True): the EXP3 update rewrites w[pos] once per block edge and "
                                      "relies on a position occurring at most once per block; LABOR keeps an edge at most once "
                                      "and has no draw with replacement")
        super().__init__(list(fanouts), eta=eta, num_steps=num_steps, model=model, draw="device")
        self.fanouts = list(fanouts)
        self.layer_dependency = bool(layer_dependency)
        self._draw_init = (seed, 0)

    def _kind(self):
        return "wlabor"                                     # (B not exactly bounded: a column's kept count is data dependent)

    def sample_blocks_static(self, g, seed_nodes, slot=0, **split):
        """sample_blocks with capacity-padded blocks, only ENQUEUED; whole calls only: any split / external-generator keyword
        raises.  A step over its calibrated capacities is reported by ``finish_static``."""
        return self._sample(g, seed_nodes, True, slot=slot, **split)


def make_sampler(name, fanouts, importance_sampling=1, num_steps=5000, eta=0.1, model="sage", draw="host", replace=False):
    """The sampler-name dispatch of DataModule.__init__ (train_lightning.py:348-370).  ``draw``: where the two multinomial
    samplers ("ladies", "bandit") and "neighbor" draw -- "host" (torch.multinomial / torch tensor ops) or "device" (the keyed
    draws, graph-capturable).  "labor" and "labor-<i>" (i in 1 .. 8: ``ImportanceLaborSampler`` with i iterations) always draw on
    the device.  "neighbor-exp3": ``BanditNeighborSampler`` (EXP3-weighted node-wise draw, always on the device); "labor-exp3":
    ``BanditLaborSampler`` (EXP3-weighted LABOR draw, always on the device).  The Poisson names ignore ``draw`` (they keep the
    draw against torch's stream); their keyed draw on the device has names of its own:
    "poisson-bandit-keyed" and "poisson-ladies-keyed".  ``replace=True``: the draws with replacement, on
    the device only -- "ladies" and "bandit" with ``draw="device"`` (built with ``draw="device-replace"``) and "neighbor" (which
    gets ``replace=True``); every other name raises."""
    from . import BanditLadiesSampler, LadiesSampler, PoissonBanditLadiesSampler, PoissonLadiesSampler as PLS
    if replace:
        if name == "neighbor":
            return NeighborSampler(fanouts, draw=draw, replace=True)
        if name not in ("ladies", "bandit"):
            raise ValueError("replace=True: only 'ladies', 'bandit' and 'neighbor' draw with replacement, not %r" % (name,))
        if draw != "device":
            raise ValueError("replace=True with %r needs draw='device' (the keyed draw with replacement)" % (name,))
        draw = "device-replace"
    if name == "poisson-ladies-keyed":
        return PLS(fanouts, draw="device")
    if name == "poisson-bandit-keyed":
        return PoissonBanditLadiesSampler(fanouts, importance_sampling=importance_sampling, node_embedding="features",
                                          num_steps=num_steps, eta=eta, model=model, draw="device")
    if name == "full":
        return MultiLayerFullNeighborSampler(len(fanouts))
    if name == "neighbor":
        return NeighborSampler(fanouts, draw=draw)
    if name == "neighbor-exp3":                             # the node-wise bandit sampler; always the device draw
        return BanditNeighborSampler(fanouts, eta=eta, num_steps=num_steps, model=model)
    if name == "labor-exp3":                                # LABOR over the EXP3 edge probabilities; always the device draw
        return BanditLaborSampler(fanouts, eta=eta, num_steps=num_steps, model=model)
    if name == "labor":
        return LaborSampler(fanouts)                        # (LABOR-0; always the device draw)
    if name.startswith("labor-"):                           # "labor-1" .. "labor-8": LABOR-i
        i = name[len("labor-"):]
        if i not in ("1", "2", "3", "4", "5", "6", "7", "8"):
            raise ValueError("unknown sampler %r (LABOR-i: 'labor-1' .. 'labor-8'; LABOR-0 is 'labor')" % (name,))
        return ImportanceLaborSampler(fanouts, iterations=int(i))
    if "ladies" in name and "bandit" not in name:
        return PLS(fanouts) if "poisson" in name else LadiesSampler(fanouts, draw=draw)
    if "bandit" in name:
        kw = dict(importance_sampling=importance_sampling, node_embedding="features", num_steps=num_steps, eta=eta, model=model)
        return PoissonBanditLadiesSampler(fanouts, **kw) if "poisson" in name else BanditLadiesSampler(fanouts, draw=draw, **kw)
    raise ValueError("unknown sampler %r" % (name,))


# ----------------------------------------------------------------------------------------------- metrics / control
def micro_f1(pred, labels, multilabel=False):
    """torchmetrics Multiclass / MultilabelF1Score(average='micro') (train_lightning.py:68-70): accuracy for single-label
    predictions; for multilabel 2 TP / (2 TP + FP + FN) over all (node, class) pairs at threshold 0.5."""
    if not multilabel:
        return float((pred.argmax(1) == labels.long()).float().mean())
    hit = torch.sigmoid(pred.float()) > 0.5
    y = labels > 0.5
    tp, fp, fn = float((hit & y).sum()), float((hit & ~y).sum()), float((~hit & y).sum())
    return 2 * tp / max(2 * tp + fp + fn, 1.0)


def _split_f1(pred, labels, nid, multilabel):
    """micro_f1(pred[nid], labels[nid]) of a full-graph prediction.  bf16 on the GPU: counted by metrics.MicroF1 straight from
    ``pred`` and the label table through ``row_ids`` / ``label_ids`` -- neither slice is materialised --, and the counts give
    micro_f1's own float (metrics.micro_f1_from_counts)."""
    if pred.is_cuda and pred.dtype == torch.bfloat16 and pred.dim() == 2:
        from .metrics import MicroF1, micro_f1_from_counts
        ids = nid.to(device=pred.device, dtype=torch.int32).contiguous()
        m = MicroF1(multilabel)
        m.update(pred, label_table=labels, label_ids=ids, row_ids=ids)
        m.check_errors()
        return micro_f1_from_counts(m.counts(), multilabel, pred.device)
    return micro_f1(pred[nid.long()].float(), labels[nid.long()], multilabel)


class StepLR:
    """``th.optim.lr_scheduler.StepLR(optimizer, gamma=0.01, step_size=5)`` stepped once per EPOCH (train_lightning.py:205-216,
    Lightning's default interval): lr x 0.01 every 5 epochs.  Works with any optimiser exposing ``param_groups``."""

    def __init__(self, optimizer, step_size=5, gamma=0.01):
        self.opt, self.step_size, self.gamma, self.epoch = optimizer, int(step_size), float(gamma), 0
        self.base = [g["lr"] for g in optimizer.param_groups]

    def lr_at(self, epoch):
        return [b * self.gamma ** (epoch // self.step_size) for b in self.base]

    def step(self):
        self.epoch += 1
        for g, lr in zip(self.opt.param_groups, self.lr_at(self.epoch)):
            g["lr"] = lr
        if hasattr(self.opt, "sync_lr"):
            self.opt.sync_lr()


class EarlyStopping:
    """``EarlyStopping(monitor='val_acc', stopping_threshold=val_acc_target, mode='max', patience=...)`` (:627-634)."""

    def __init__(self, stopping_threshold=1.0, patience=1000):
        self.threshold, self.patience, self.best, self.bad = stopping_threshold, int(patience), -math.inf, 0

    def should_stop(self, val_acc):
        if val_acc > self.best:
            self.best, self.bad = val_acc, 0
        else:
            self.bad += 1
        # Lightning's stopping_threshold in mode='max' is STRICT: stop once the monitored value is better than the threshold
        return val_acc > self.threshold or self.bad >= self.patience


class BatchSizeController:
    """``BatchSizeCallback(limit, factor)`` (``--vertex-limit``, train_lightning.py:425-486): steers the batch size towards
    ``limit`` input-layer vertices per step.  Every step's ``mfgs[0].num_src_nodes()`` goes through ``push`` (a running mean
    ``m`` and sum of squared deviations ``s`` over ``n`` steps; the device keeps the same three words, ``load`` takes them from
    ``GraphedTrainStep.batch_stats()``).  At an epoch's end ``propose(batch_size)`` answers with a new size once the mean is at
    least ``factor`` standard errors away from the limit,

        limit > 0  and  n >= 2  and  |limit - m| * n >= sqrt(s / (n - 1)) * factor,

    namely ``int(batch_size * limit / m)`` -- and only then are the statistics cleared; otherwise they keep accumulating
    across epochs.  The reference lets that size reach 0 or pass the split and then fails; here it is clamped to
    ``[1, max_size]`` and ``clamped`` says whether the clamp changed it."""

    def __init__(self, limit, factor=3):
        self.limit, self.factor, self.clamped = limit, factor, False
        self.clear()

    def clear(self):
        self.n, self.m, self.s = 0, 0.0, 0.0

    def push(self, x):
        self.n += 1
        m = self.m
        self.m += (x - m) / self.n
        self.s += (x - m) * (x - self.m)

    def load(self, n, m, s):
        self.n, self.m, self.s = int(n), float(m), float(s)

    def propose(self, batch_size, max_size=None):
        """The batch size of the next epoch, or None for "keep it"."""
        if not (self.limit > 0 and self.n >= 2):
            return None
        if abs(self.limit - self.m) * self.n < math.sqrt(self.s / (self.n - 1)) * self.factor:
            return None
        want = int(batch_size * self.limit / self.m)
        new = max(want, 1)
        if max_size is not None:
            new = min(new, int(max_size))
        self.clamped = new != want
        self.clear()
        return new


class ModelCheckpoint:
    """``ModelCheckpoint(monitor='val_acc', save_top_k=1, mode='max')`` (:620-625): keep the best parameters (in memory, and
    on disk when a path is given; the EXP3 state is NOT part of it, as in the reference -- bandit_sampler.py:43).

    On disk the file has the layout of the reference's Lightning ``.ckpt`` as far as its reload path reads it
    (train_lightning.py:64, :671-682: ``load_from_checkpoint`` takes ``checkpoint['state_dict']``, whose keys carry the
    ``module.`` prefix of ``ModelLightning.module``): ``{'state_dict': {'module.<name>': tensor}, 'epoch', 'monitor', 'best'}``
    -- tensors and plain numbers only, so ``torch.load(path, weights_only=True)`` reads it."""

    PREFIX = "module."

    def __init__(self, path=None):
        self.path, self.best, self.state, self.epoch = path, -math.inf, None, -1

    def update(self, val_acc, model, epoch=-1):
        if val_acc > self.best:
            self.best, self.epoch = val_acc, int(epoch)
            self.state = copy.deepcopy({k: v.detach().clone() for k, v in model.state_dict().items()})
            if self.path:
                os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
                torch.save({"state_dict": {self.PREFIX + k: v for k, v in self.state.items()}, "epoch": self.epoch,
                            "monitor": "val_acc", "best": float(self.best)}, self.path)
            return True
        return False

    def restore(self, model):
        if self.state is not None:
            model.load_state_dict(self.state)

    @classmethod
    def load(cls, path, model, strict=True):
        """Load a checkpoint written by ``update`` -- or a Lightning ``.ckpt`` of the reference whose tensors the safe loader
        accepts -- into ``model`` (``strict=False`` like the reference's GCN reload, train_lightning.py:675-680)."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
        sd = {(k[len(cls.PREFIX):] if k.startswith(cls.PREFIX) else k): v for k, v in sd.items()}
        return model.load_state_dict(sd, strict=strict)


@torch.no_grad()
def evaluate(g, sampler, model, ids, batch_size, multilabel=False, loss_fn=None, step=None):
    """validation_step over a split (train_lightning.py:179-203): the same sampler object, no bandit update, no optimiser.
    ``step``: a train.GraphedEvalStep built on the same (g, sampler, model, batch_size) -- the pass is then its ``run(ids)``:
    full batches replayed from one graph, metric and loss kept on the device and read back once."""
    if step is not None:
        return step.run(ids)
    was = model.training
    model.eval()
    preds, labels, losses = [], [], []
    for seeds in BatchLoader(ids, batch_size, shuffle=False, drop_last=False):
        _, _, mfgs = sampler.sample(g, seeds)
        pred = model(mfgs, _inputs(model, mfgs))
        y = mfgs[-1].dstdata["labels"]
        preds.append(pred.float()); labels.append(y)
        if loss_fn is not None:
            losses.append(float(loss_fn(pred, y)) * seeds.numel())
    model.train(was)
    if hasattr(loss_fn, "check_errors"):
        loss_fn.check_errors()                                                   # (every batch's loss was read back above)
    pred, y = torch.cat(preds), torch.cat(labels)
    return micro_f1(pred, y, multilabel), (sum(losses) / max(ids.numel(), 1) if losses else None)


def fit(g, sampler, model, train_nid, val_nid, test_nid=None, batch_size=1024, lr=0.002, max_epochs=10, max_steps=None,
        multilabel=False, val_acc_target=1.0, early_stopping_patience=1000, checkpoint_path=None, seed=0, log=None,
        eval_step="eager", train_metric=False, train_step="eager", vertex_limit=-1, limit_factor=3, batch_capacity=None,
        inference_path=None):
    """One run of ``trainer.fit`` + the final evaluation (train_lightning.py:640-705).  Returns a dict of metrics.
    ``eval_step``: "eager" (``evaluate`` as it stands) or "graphed" (one train.GraphedEvalStep serves every epoch's validation;
    the sampler needs a static-shape path).  ``train_metric``: keep train_acc (:143) on the device beside every step and add it,
    reset per epoch, to the history entries.  ``train_step``: "eager" (TrainStep, a loss read back per step) or "graphed" (the
    epoch's steps replayed from one captured train.GraphedTrainStep whose ledger keeps the epoch's statistics on the device,
    DESIGN.md section 18: the same batches, random streams and bits; the sampler needs a static-shape path and the model the
    one-launch Adam); its history entries also carry ``sampled_nodes`` / ``sampled_edges``.

    ``vertex_limit`` > 0 (``--vertex-limit``, train_lightning.py:425-486): a ``BatchSizeController(vertex_limit,
    limit_factor)`` sees every step's input-layer size and, at each epoch's end, may set the batch size of the following epochs
    (training and validation), clamped to ``[1, min(len(train_nid), batch_capacity)]``.  The history entries then carry
    ``batch_size`` (the epoch's), ``batch_size_clamped``, ``input_nodes`` (the controller's ``n``, ``m``, ``s`` at the epoch's end)
    and ``sampled_nodes`` / ``sampled_edges`` in both loops.  The graphed loop runs under ``batch_capacity`` seeds (default twice
    the batch size): one captured step serves every size, nothing is re-captured, and the statistics come with the epoch's one
    read-back.  ``-1`` (and no ``batch_capacity``): the loops as they were.

    ``inference_path``: when not None, passed as ``path=`` to the final ``model.inference(g)`` (SAGE, GCN and GATv2 each name their
    paths in ``INFERENCE_PATHS``); None: the call as it was."""
    if eval_step not in ("eager", "graphed"):
        raise ValueError("eval_step must be 'eager' or 'graphed', not %r" % (eval_step,))
    if train_step not in ("eager", "graphed"):
        raise ValueError("train_step must be 'eager' or 'graphed', not %r" % (train_step,))
    g = as_graph(g)
    ctl = BatchSizeController(vertex_limit, limit_factor) if vertex_limit > 0 else None
    if batch_capacity is not None and not int(batch_size) <= int(batch_capacity):
        raise ValueError("batch_capacity (%d) must be at least the batch size (%d)" % (int(batch_capacity), int(batch_size)))
    if train_step == "graphed":
        return _fit_graphed(g, sampler, model, train_nid, val_nid, test_nid, batch_size, lr, max_epochs, max_steps, multilabel,
                            val_acc_target, early_stopping_patience, checkpoint_path, seed, log, eval_step, train_metric, ctl,
                            batch_capacity, inference_path)
    step = TrainStep(g, sampler, model, lr=lr, multilabel=multilabel, train_metric=train_metric)
    ev_cap = batch_capacity
    if ev_cap is None and ctl is not None and eval_step == "graphed":
        ev_cap = 2 * int(batch_size)                  # (the replayed validation follows the batch size inside a capacity)
    max_bs = int(train_nid.numel()) if ev_cap is None else min(int(train_nid.numel()), int(ev_cap))
    cur_bs, clamped = int(batch_size), False
    ev = GraphedEvalStep(g, sampler, model, batch_size, multilabel, loss_fn=step.loss_fn, batch_capacity=ev_cap) if eval_step == "graphed" else None
    sched, stopper, ckpt = StepLR(step.opt, 5, 0.01), EarlyStopping(val_acc_target, early_stopping_patience), ModelCheckpoint(checkpoint_path)
    loader = BatchLoader(train_nid, batch_size, shuffle=True, drop_last=True, seed=seed)
    history, n_steps = [], 0
    for epoch in range(max_epochs):
        model.train()
        tot, cnt = 0.0, 0
        for seeds in loader:
            tot += float(step(seeds)); cnt += 1; n_steps += 1
            if ctl is not None:
                ctl.push(step.last["mfgs"][0].num_src_nodes())                   # :467
            if max_steps is not None and n_steps >= max_steps:
                break
        val_acc, val_loss = evaluate(g, sampler, model, val_nid, cur_bs, multilabel, step.loss_fn, step=ev)
        ckpt.update(val_acc, model, epoch)
        history.append(dict(epoch=epoch, train_loss=tot / max(cnt, 1), val_acc=val_acc, val_loss=val_loss, lr=step.opt.param_groups[0]["lr"]))
        if train_metric:
            history[-1]["train_acc"] = step.train_acc.compute()                 # (one read-back per epoch)
            step.train_acc.reset()
            step.train_acc.check_errors()
        if ctl is not None:
            L = len(sampler.nodes_per_layer)
            history[-1].update(batch_size=cur_bs, batch_size_clamped=clamped, input_nodes=dict(n=ctl.n, m=ctl.m, s=ctl.s),
                               sampled_nodes=[step.num_sampled_nodes(i) for i in range(L + 1)],
                               sampled_edges=[step.num_sampled_edges(i) for i in range(L)])
            new = ctl.propose(cur_bs, max_bs)                                    # on_train_epoch_end, :472-486
            if new is not None:
                cur_bs, clamped = new, ctl.clamped
                loader.set_batch_size(new)
                if ev is not None:
                    ev.set_batch_size(new)
        if log:
            log(history[-1])
        sched.step()                                                             # per epoch (:205-216)
        if stopper.should_stop(val_acc) or (max_steps is not None and n_steps >= max_steps):
            break
    if ev is not None:
        ev.close()
    return dict(history=history, best_val_acc=ckpt.best, steps=n_steps, final=_final_metrics(g, model, ckpt, train_nid, val_nid, test_nid,
                                                                                             multilabel, inference_path))


def _final_metrics(g, model, ckpt, train_nid, val_nid, test_nid, multilabel, inference_path=None):
    """The best checkpoint reloaded, then the Final Accuracy of the three splits (train_lightning.py:662-705).  ``inference_path``:
    the ``path=`` of ``model.inference`` when not None."""
    ckpt.restore(model)                                                          # the best val_acc checkpoint (:662-685)
    final = {}
    if hasattr(model, "inference") and "features" in g.ndata:
        pred = model.inference(g) if inference_path is None else model.inference(g, path=inference_path)     # :686-693 layer-wise full-neighbour inference
        for name, nid in (("Train", train_nid), ("Validation", val_nid), ("Test", test_nid)):
            if nid is not None and nid.numel():
                final[name] = _split_f1(pred, g.ndata["labels"], nid, multilabel)                            # :694-705
    return final


def _fit_graphed(g, sampler, model, train_nid, val_nid, test_nid, batch_size, lr, max_epochs, max_steps, multilabel, val_acc_target,
                 early_stopping_patience, checkpoint_path, seed, log, eval_step, train_metric, ctl=None, batch_capacity=None,
                 inference_path=None):
    """``fit`` with the epoch's steps replayed from one captured train step (train.GraphedTrainStep with its ledger): the same
    protocol, batches, random streams and bits as the eager loop; the host reads one ledger record per epoch."""
    static = hasattr(sampler, "sample_blocks_static") and (getattr(sampler, "_poisson", False) or getattr(sampler, "draw", "host") == "device")
    if not static:
        raise NotImplementedError("fit(train_step='graphed') needs a sampler with a static-shape path; %s%s has none (the Poisson "
                                  "samplers have one, and the samplers that draw on the device: draw='device', labor, neighbor-exp3)"
                                  % (type(sampler).__name__, " with draw='host'" if hasattr(sampler, "draw") else ""))
    from .optim import Adam
    # a batch-size controller needs room to move: the step is captured once for ``cap`` seeds and runs any live count below it
    cap = batch_capacity
    if cap is None and ctl is not None:
        cap = 2 * int(batch_size)
    if cap is not None:
        cap = max(min(int(cap), int(train_nid.numel())), int(batch_size))
    cur_bs, clamped = int(batch_size), False
    step = GraphedTrainStep(g, sampler, model, batch_size, lr=lr, multilabel=multilabel, train_metric=train_metric, ledger=True,
                            batch_capacity=cap)
    if not isinstance(step.opt, Adam):
        raise TypeError("fit(train_step='graphed') needs the one-launch Adam of bliss_gnn_amd.optim (contiguous bf16 parameters on the "
                        "GPU, at most %d tensors): a replayed step runs no Python, so the learning rate StepLR rewrites must live on "
                        "the device; this model's parameters get %s" % (_lib.ADAM_MAX_TENSORS, type(step.opt).__name__))
    ev = GraphedEvalStep(g, sampler, model, batch_size, multilabel, loss_fn=step.loss_fn, batch_capacity=cap) if eval_step == "graphed" else None
    sched, stopper, ckpt = StepLR(step.opt, 5, 0.01), EarlyStopping(val_acc_target, early_stopping_patience), ModelCheckpoint(checkpoint_path)
    loader = BatchLoader(train_nid, batch_size, shuffle=True, drop_last=True, seed=seed)
    L = len(sampler.nodes_per_layer)
    history, n_steps = [], 0
    try:
        model.train()
        # capacities from a second loader with the same ids and seed, leaving torch's generator and the draw step where they
        # were: the epoch's batches and the sampler's random stream stay those of the eager loop
        with _rng_kept(sampler, g):
            step.calibrate(BatchLoader(train_nid, batch_size if cap is None else cap, shuffle=True, drop_last=True, seed=seed).forever())
        eng = sampler._engine
        for epoch in range(max_epochs):
            model.train()
            batches = iter(loader)                                               # (a new batch size takes effect here)
            n = len(loader) if max_steps is None else min(len(loader), max_steps - n_steps)
            step.run(batches, n)                                                 # (the first one captures: its steps are epoch 0's)
            n_steps += n
            rec = step.ledger()                                                  # THE read-back of the epoch
            step.reset_epoch()
            if ev is not None:
                val_acc, val_loss = evaluate(g, sampler, model, val_nid, cur_bs, multilabel, step.loss_fn, step=ev)
            else:
                with _keep_static_caps(eng):                                     # (eager sampling beside the captured train graph)
                    val_acc, val_loss = evaluate(g, sampler, model, val_nid, cur_bs, multilabel, step.loss_fn)
            ckpt.update(val_acc, model, epoch)
            history.append(dict(epoch=epoch, train_loss=rec["loss_sum"] / max(rec["steps_epoch"], 1), val_acc=val_acc, val_loss=val_loss,
                                lr=step.opt.param_groups[0]["lr"]))
            if train_metric:
                history[-1]["train_acc"] = step.train_acc.compute()             # (one read-back per epoch)
                step.train_acc.reset()
                step.train_acc.check_errors()
            history[-1]["sampled_nodes"] = [step.num_sampled_nodes(i, rec) for i in range(L + 1)]
            history[-1]["sampled_edges"] = [step.num_sampled_edges(i, rec) for i in range(L)]
            if ctl is not None:
                ctl.load(**step.batch_stats(rec))                                # the device's n, m, s: came with the read-back above
                history[-1].update(batch_size=cur_bs, batch_size_clamped=clamped, input_nodes=dict(n=ctl.n, m=ctl.m, s=ctl.s))
                new = ctl.propose(cur_bs, min(int(train_nid.numel()), cap))      # on_train_epoch_end, :472-486
                if new is not None:                                              # the loader's size; the live count follows the
                    cur_bs, clamped = new, ctl.clamped                           # batches -- no re-capture
                    loader.set_batch_size(new)
                    step.clear_batch_stats()
                    if ev is not None:
                        ev.set_batch_size(new)
            if log:
                log(history[-1])
            sched.step()                                                         # per epoch (:205-216)
            step.opt.sync_lr()                                                   # a replay runs no Python: the new rate goes to the device here
            if stopper.should_stop(val_acc) or (max_steps is not None and n_steps >= max_steps):
                break
    finally:
        if ev is not None:
            ev.close()
        step.close()
    return dict(history=history, best_val_acc=ckpt.best, steps=n_steps, final=_final_metrics(g, model, ckpt, train_nid, val_nid, test_nid,
                                                                                             multilabel, inference_path))


def k_runs(run_fn, k):
    """``--k-runs`` (train_lightning.py:565, :711-733): repeat a run, reduce every final metric to mean / std (what
    tensorboard_reducer writes with reduce_ops = ('mean', 'std'); population std, as numpy's default)."""
    outs = [run_fn(i) for i in range(k)]
    keys = sorted({("final", n) for o in outs for n in o["final"]} | {("best_val_acc", None)})
    red = {}
    for kind, n in keys:
        xs = [o["final"][n] if kind == "final" else o["best_val_acc"] for o in outs if kind != "final" or n in o["final"]]
        m = sum(xs) / len(xs)
        red[n or "best_val_acc"] = dict(mean=m, std=(sum((x - m) ** 2 for x in xs) / len(xs)) ** 0.5, n=len(xs))
    return dict(runs=outs, reduced=red)
