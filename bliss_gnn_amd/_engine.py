"""Host-side driver of the gfx950 sampler kernels.

One ``sample_blocks`` call = L x (frontier_prob, mt19937, poisson_select, build_block) enqueued on
the current stream with NO host round trip in between: every size (S, E, C, K, B) stays on the
device and the next layer reads its seed count from the previous layer's counts record.  A single
device->host copy at the end returns all sizes, the error words and the advanced generator state
(the reference syncs >= 24 times per step).

Buffers are sized by per-layer capacities; if a capacity is exceeded the kernels clamp, flag it,
and the whole call is repeated with larger buffers from the same generator snapshot (steady state:
never).  PyTorch is used for device memory and the current stream only.
"""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .graph import Block, Graph

_CHUNK = 1024
_CAP_ERRS = 1 | 2 | 4 | 8 | 64      # (128, the random stream, is fatal: the stream is sized for the worst case)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up8(n):
    return (int(n) + 7) & ~7


def spmm_partials(B, D, device, floor=None):
    """The fp32 head / tail partials of the balanced SpMM walk (csrc/spmm_walk.cuh): two rows of D per chunk of B edges.
    ``floor`` = the least number of floats to allocate; None = no buffer at all for a block without edges."""
    ec = _lib.lib.bliss_spmm_chunk_edges(B)
    n = 2 * ((B + ec - 1) // ec) * D
    if floor is None:
        return torch.empty(n, dtype=torch.float32, device=device) if B > 0 else None
    return torch.empty(max(n, floor), dtype=torch.float32, device=device)


# ---------------------------------------------------------------------- the kinds of layer an engine runs
class _Kind(NamedTuple):
    """What the host driver knows about one kind of layer; an engine runs one kind (``LayerEngine.kind``)."""
    family: str                 # "layer": frontier_prob -> draw -> build_block; "node": one *_layer call + the by-source index
    k_slack: int = None         # K capacity >= fanout + S + this; 0: K is exactly bounded (``exact_k``).  None: no such floor
    b_limit: int = None         # B capacity = S * fanout (fanout >= 0) capped by this, 0 = |E| (``exact_b``).  None: B may overflow
    fatal: int = 3              # error bits that end the exact-shape call instead of growing the buffers ...
    fatal_no_bins: int = 0      # ... and those that do so only on the atomic passes (n_bins == 0)
    own_messages: bool = False  # bits 1 and 2 raise with messages of their own
    keyed: bool = True          # draws from a DrawState; a repeated call rolls the draw step back
    torch_rng: bool = False     # consumes torch's CPU generator (snapshot, stage, commit) unless uniforms are given
    split: bool = False         # split enqueue, external and chained generator exist
    keys: bool = False          # the race keys go into the blocks' _trace
    prob: str = None            # probability record (neighbor_prob): None = takes none, "raw" = optional raw-mode, "any" = required
    entry: str = None           # node-wise: the C entry point, ...
    scratch: object = None      # ... its scratch: (engine, cap_s, cap_b) -> zeroed int32 tensor, ...
    tail: object = None         # ... its own arguments after the eleven shared ones: (draw record, probability row) -> tuple
    p_out: bool = False         # ... and whether it writes p_ij (the blocks' _p)


def _prob_args(d, row):
    return d.prob["mode"], row.data_ptr(), d.prob["eta_f"], d.prob["ome_f"]


def _dep(d):
    return int(bool(d.layer_dependency))


KINDS = {
    # Poisson from the MT stream (or explicit uniforms) / keyed Poisson
    "stream": _Kind("layer", fatal=1, fatal_no_bins=2, own_messages=True, keyed=False, torch_rng=True, split=True),
    "poisson_keyed": _Kind("layer", fatal=1, fatal_no_bins=2, own_messages=True),
    # torch.multinomial on the host / the keyed race of csrc/mn_draw.hip / the draw with replacement of csrc/replace_draw.hip
    "multinomial_host": _Kind("layer", k_slack=64, fatal=2, keyed=False),
    "multinomial": _Kind("layer", k_slack=0, fatal=1, fatal_no_bins=2, keys=True),
    "multinomial_replace": _Kind("layer", k_slack=0, fatal=1, fatal_no_bins=2),
    # node-wise: csrc/neighbor.hip, neighbor_w.hip, replace_draw.hip, labor.hip, labor_is.hip, labor_w.hip
    "neighbor": _Kind("node", b_limit=0, entry="bliss_neighbor_layer", tail=lambda d, row: (),
                      scratch=lambda e, s, b: e._scratch_once("_nb_scr", "bliss_neighbor_scratch_bytes", 1)),
    "wneighbor": _Kind("node", b_limit=0, prob="any", entry="bliss_wneighbor_layer", tail=lambda d, row: _prob_args(d, row) + (0,),
                       scratch=lambda e, s, b: e._scratch_once("_wn_scr", "bliss_wneighbor_scratch_bytes", e.V, e.Eg)),
    # (a column of fewer than fanout edges holds fanout block edges: |E| is no bound on B)
    "neighbor_replace": _Kind("node", b_limit=2 ** 31 - 1, prob="raw", entry="bliss_neighbor_replace_layer",
                              tail=lambda d, row: (_ptr(row), 0),
                              scratch=lambda e, s, b: e._scratch_once("_nr_scr", "bliss_neighbor_replace_scratch_bytes", 1)),
    "labor": _Kind("node", entry="bliss_labor_layer", tail=lambda d, row: (_dep(d),),
                   scratch=lambda e, s, b: e._scratch_grown("_lb_scr", "bliss_labor_scratch_bytes", s)),
    "labor_is": _Kind("node", entry="bliss_labor_is_layer", tail=lambda d, row: (_dep(d), int(d.iterations)),
                      scratch=lambda e, s, b: e._scratch_grown("_li_scr", "bliss_labor_is_scratch_bytes", s, b)),
    "wlabor": _Kind("node", prob="any", entry="bliss_wlabor_layer", tail=lambda d, row: (_dep(d),) + _prob_args(d, row), p_out=True,
                    scratch=lambda e, s, b: e._scratch_grown("_wl_scr", "bliss_wlabor_scratch_bytes", s, b)),
}


class _Draw(NamedTuple):
    """The per-call values of a layer that are not its kind."""
    state: object = None        # DrawState of the keyed draws
    prob: dict = None           # neighbor_prob(...)'s record
    layer_dependency: bool = False
    iterations: int = 0         # LABOR-i


# caller-owned outputs of one layer, capacity-sized (LayerEngine._layer_buffers)
_LayerOut = NamedTuple("_LayerOut", [(name, object) for name in
                                     "indptr src dst pos eid w q kept_nid node_prob counts t_indptr t_edge".split()])


def _exact_b(rule, Eg, s, f):
    """The exact edge bound of a neighbor layer: at most ``fanout`` edges per seed."""
    return int(min(rule.b_limit or Eg, s * f))


def layer_caps(kind, V, Eg, S0, fanouts, have=None):
    """Per-layer capacities (sampling order) of ``kind`` for S0 seeds on a graph of V nodes and Eg edges.  ``have``: the
    capacities so far; they are kept while they hold S0 seeds, else merged (max) with fresh ones.  Pure: returns ``have`` itself
    when nothing changes, new dicts otherwise."""
    rule = KINDS[kind]
    if have is not None and len(have) != len(fanouts):
        have = None
    if have is not None and have[0]["S"] >= S0:
        if rule.k_slack is None:
            return have
        caps = [dict(c) for c in have]
    else:
        caps, s = [], int(S0)
        for f in fanouts:
            f = int(f)
            if rule.family == "layer":
                k = min(V, int(1.25 * (f + s)) + 64)
                b = int(min(Eg, max(1 << 16, 48 * k)))
            elif f < 0:                     # whole columns: nothing bounds K or B
                k, b = V, int(min(Eg, max(1 << 16, 48 * s)))
            else:                           # besides its seeds a layer keeps at most one new source per kept edge
                # (LABOR keeps fanout edges per column in expectation, not at most: twice that, the regrow loop covers the rest)
                b = _exact_b(rule, Eg, s, f) if rule.b_limit is not None else int(min(Eg, 2 * s * f + 4096))
                k = int(min(V, s + min(b, Eg)))
            caps.append(dict(S=s, C=V, K=k, B=b))
            s = k
        if have is not None:
            caps = [{k: max(a.get(k, 0), b[k]) for k in b} for a, b in zip(have, caps)]
    if rule.k_slack is not None:            # a multinomial draw keeps union(drawn, seeds): make room
        for n, f in enumerate(fanouts):
            caps[n]["K"] = max(caps[n]["K"], min(V, int(f) + caps[n]["S"] + rule.k_slack))
            if n + 1 < len(caps):           # a layer's seeds are the previous layer's kept nodes
                caps[n + 1]["S"] = max(caps[n + 1]["S"], caps[n]["K"])
    return have if caps == have else caps


def static_caps(kind, V, Eg, S0, fanouts, max_sizes, k_margin=1.5, b_margin=3.0):
    """Capacities fixed from sizes observed in exact mode (``LayerEngine.set_static_caps``); exact bounds where ``kind`` has them."""
    rule = KINDS[kind]
    caps, s = [], int(S0)
    for n, f in enumerate(fanouts):
        k = min(V, int(k_margin * max_sizes[n]["K"]) + 256)
        if rule.k_slack == 0:               # (device-drawn multinomial layer: the exact bound, such a step cannot overflow K)
            k = min(V, int(f) + s)
        b = int(min(Eg, int(b_margin * max_sizes[n]["B"]) + 4096))
        if rule.b_limit is not None and int(f) >= 0:    # (neighbor layer: the exact bound, such a step cannot overflow B)
            b = _exact_b(rule, Eg, s, int(f))
        # E only sizes launch grids (every kernel strides over the true count): a tight bound lets the hardware balance
        # the workgroups instead of a capped grid looping unevenly
        e = int(min(Eg, int(1.5 * max_sizes[n].get("E", Eg)) + 65536))
        # X: how many block edges a multi-GPU step EXCHANGES per block (update lists are sent capacity-sized; B's margin
        # is for memory that costs nothing, X's for bytes that cross xGMI every step); a longer list is flagged
        x = int(min(b, int(1.5 * max_sizes[n]["B"]) + 2048))
        caps.append(dict(S=s, C=V, K=k, B=b, E=e, X=x))
        s = k
    return caps


def _parse_counts(counts_host, L):
    """The L LayerCounts records of a pinned counts tensor (after a synchronisation) and the OR of their error words."""
    raw = counts_host.numpy().tobytes()
    cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
    bad = 0
    for c in cnts:
        bad |= c.err
    return cnts, bad


class _LayerWs:
    """Persistent per-layer scratch (internal to the sampler, reused every call)."""

    def __init__(self, dev, cap_s, cap_c):
        self.cap_s, self.cap_c = cap_s, cap_c
        self.seg_ptr = torch.empty(cap_s + 1, dtype=torch.int32, device=dev)
        self.seed_acc = torch.empty(72 * cap_s + 64, dtype=torch.uint8, device=dev)    # 7 x u64 per seed + k_seg_scan's long-column list (16 B each, two counts)
        self.cand_nid = torch.empty(cap_c, dtype=torch.int32, device=dev)
        self.new_id = torch.empty(cap_c, dtype=torch.int32, device=dev)
        self.p = torch.empty(cap_c, dtype=torch.bfloat16, device=dev)
        self.P = torch.empty(cap_c, dtype=torch.bfloat16, device=dev)
        self.uniforms = torch.empty(cap_c, dtype=torch.float32, device=dev)     # explicit-uniforms path only
        # device-side multinomial draw (csrc/mn_draw.hip): race keys + bins / ticket / tie counts (zero once, left zero by every call)
        self.keys = torch.empty(cap_c, dtype=torch.float32, device=dev)
        self.draw_scr = torch.zeros(int(_lib.lib.bliss_multinomial_draw_scratch_bytes(cap_c)) // 4, dtype=torch.int32, device=dev)
        self.rdraw_scr = None               # csrc/replace_draw.hip's layer-wise draw: ticket, per-chunk and per-candidate prefixes (zero once)
        self.src_cnt = None
        self.tr_temp = None                 # neighbor layers: bliss_block_transpose's temporary, (capacities, bytes, tensor)


class DrawState:
    """Seed and step counter of the keyed draws (``draw="device"``: multinomial, neighbor, LABOR, keyed Poisson).  The counter
    lives on the device: the last layer of every sampler call bumps it, also when the call is a replayed HIP graph."""

    def __init__(self, seed, step, device):
        self.seed = int(seed) & ((1 << 64) - 1)
        self.step_dev = torch.tensor([int(step)], dtype=torch.int64, device=device)

    def step(self):
        return int(self.step_dev.item())


class LayerEngine:
    """Per-graph sampling state.  Not re-entrant and not shareable between DataLoader workers --
    the same ownership rule as the reference sampler's mutable state (bandit_sampler.py:43)."""

    def __init__(self, g: Graph, kind="stream"):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, not %r" % (", ".join(KINDS), kind))
        if g.device.type != "cuda":
            raise RuntimeError("bliss_gnn_amd samples on the GPU only; move the graph with g.to('cuda') "
                               "(the reference's --data-cpu/--use-uva modes are out of scope)")
        self.g = g
        dev = g.device
        V = g.num_nodes()
        self.V, self.Eg = V, g.num_edges()
        if self.Eg >= 2 ** 31:
            raise RuntimeError("int32 edge positions: graphs with >= 2^31 edges are not supported")
        # Scratch shared by the layers exists ``scratch_sets`` times, layer n (sampling order) uses set n % scratch_sets: the
        # block passes of layer n touch none of what the candidate pipeline of layer n + 1 touches, so a caller may run them
        # beside each other on two streams (train.PipelinedTrainStep does, with one set per layer).
        self.scratch_sets = 2
        self._sets = {}
        self.first_pos = torch.full((V,), -1, dtype=torch.int32, device=dev)      # 0xFFFFFFFF
        self.acc_p2 = torch.zeros(V, dtype=torch.int64, device=dev)
        self.c_graph = _lib.Graph(g.indptr.data_ptr(), g.indices.data_ptr(), _ptr(g.eid), V, self.Eg)
        self.flags = torch.zeros(16, dtype=torch.int32, device=dev)              # cross-stream hand-offs (bliss_flag_wait)
        self.fs_ticket = torch.zeros(1, dtype=torch.int32, device=dev)           # bliss_layer_ws_t::fs_ticket
        self.fuse_scale = os.environ.get("BLISS_FUSE_SCALE", "1") != "0"
        self.flag_err = torch.zeros(1, dtype=torch.int32, device=dev)
        # binned candidate pipeline (csrc/sampler.hip): LDS-resident per-source reductions when |V| / n_bins slots fit in
        # 64 KiB; otherwise (or with BLISS_BINS=0) the memory-side atomic passes.  Scratch shared by all layers.
        self.n_bins = 0
        for nb in ((int(os.environ["BLISS_NBINS"]),) if os.environ.get("BLISS_NBINS") else (256, 1024)):
            if -(-V // nb) * 12 <= 64 * 1024:
                self.n_bins = nb
                break
        if os.environ.get("BLISS_BINS", "1") == "0" or self.Eg > 2048 * 4096 * 32:     # (bitmap tiles: MAX_TILES in sampler.hip)
            self.n_bins = 0
        self._bins = None
        self.hist = torch.zeros(32768, dtype=torch.int32, device=dev)      # self-cleaning (k_poisson_scale)
        self.mt_dev = torch.empty(626, dtype=torch.int32, device=dev)
        self.mt_host = torch.empty(626, dtype=torch.int32).pin_memory()        # state handed to the device
        self.mt_back = torch.empty(626, dtype=torch.int32).pin_memory()        # state handed back
        self._static = {}
        self._static_draw = {}
        self.kind = kind                    # a key of KINDS; the sampler that binds the engine fixes it
        self._nr_scr = None                 # csrc/replace_draw.hip's node-wise draw: csrc/neighbor.hip's words
        self._nb_scr = None                 # csrc/neighbor.hip: tickets + node bitmap (zero once, left zero by every call)
        self._wn_scr = None                 # csrc/neighbor_w.hip: the same words + a record per seed and a staged key per CSC position
        self._lb_scr = None                 # csrc/labor.hip: the same words + one kept count per seed column; (cap_s, tensor)
        self._li_scr = None                 # csrc/labor_is.hip: + two |V|-word importance buffers, scales, p_e; (cap_s, cap_b, tensor)
        self._wl_scr = None                 # csrc/labor_w.hip: + three records per seed column and p_e; (cap_s, cap_b, tensor)
        self._wl_p = {}                     # its p_ij outputs: per static slot (slot, layer, cap_b) -> bf16 [cap_b]
        self._slot_bufs, self._slot_counts, self._slot_counts_host = {}, {}, {}
        self.caps = None
        self.ws = None
        self.counts_host = None
        self.retries = 0

    def _set(self, n):
        """The shared-scratch set of layer n: dense node maps (-1 = clean), span table, chunk counters, spill buffers."""
        i = n % self.scratch_sets
        if i not in self._sets:
            dev, V = self.g.device, self.V
            local_id = torch.full((V,), -1, dtype=torch.int32, device=dev)
            self._sets[i] = dict(local_id=local_id, kept_map=torch.full((V,), -1, dtype=torch.int32, device=dev),
                                 span_seg=torch.zeros(self.Eg // 256 + 2, dtype=torch.int32, device=dev),
                                 chunk_cnt=torch.empty(max(self.Eg, V) // _CHUNK + 2, dtype=torch.int32, device=dev),
                                 kept_rec=None, span_cnt=None,
                                 c_maps=_lib.NodeMaps(local_id.data_ptr(), self.first_pos.data_ptr(), self.acc_p2.data_ptr()))
        return self._sets[i]

    # ------------------------------------------------------------------ capacities
    # What the kind implies (read-only).  exact_k: device-drawn multinomial layers keep at most fanout + S nodes, K capacities are
    # that bound.  exact_b: neighbor layers keep at most fanout edges per seed, B capacities are that bound; nb_replace: drawn WITH
    # replacement, B <= S * fanout but not <= |E|.  labor_is: LABOR layers run csrc/labor_is.hip also with 0 iterations.
    exact_k = property(lambda self: KINDS[self.kind].k_slack == 0)
    exact_b = property(lambda self: KINDS[self.kind].b_limit is not None)
    nb_replace = property(lambda self: bool(KINDS[self.kind].b_limit))
    labor_is = property(lambda self: self.kind == "labor_is")

    def _use(self, kind):
        """The kind of the exact-shape call at hand; capacities fixed with / without replacement do not carry over."""
        if bool(KINDS[kind].b_limit) != self.nb_replace:
            self.caps, self.ws = None, None
        self.kind = kind
        return KINDS[kind]

    def _ensure(self, S0, fan):
        caps = layer_caps(self.kind, self.V, self.Eg, S0, fan, self.caps)
        if self.caps is None or [c["S"] for c in caps] != [c["S"] for c in self.caps]:
            self.ws = None
        self.caps = caps
        if self.ws is None:
            dev = self.g.device
            self.ws = [_LayerWs(dev, c["S"], c["C"]) for c in self.caps]
            self.counts_host = torch.empty(len(fan) * 10, dtype=torch.int32).pin_memory()
            # one random stream per call: the layers consume consecutive slices of it
            self.rng_cap = sum(c["C"] for c in self.caps)
            # (jump-ahead tables for this capacity: the stream is then generated by several workgroups at once, csrc/rng.hip)
            plan = (C.c_int32 * 4)()
            _lib.check(_lib.lib.bliss_rng_prepare(self.rng_cap, plan), "bliss_rng_prepare")
            self.rng_plan = tuple(plan)
            n_words = 624 * (max(plan[3], self.rng_cap // 624 + 1) + 2)
            self.rng_out = torch.empty(n_words, dtype=torch.float32, device=dev)
            self.rng_raw = torch.empty(n_words, dtype=torch.int32, device=dev)
            self.rng_ctl = torch.zeros(8 + len(fan), dtype=torch.int32, device=dev)     # ctl[8] + per-layer offsets

    def _bin_buffers(self):
        if self._bins is None:
            dev, nb = self.g.device, self.n_bins
            cap = int(1.25 * self.Eg / nb) + 8192
            words = (-(-self.Eg // 4096) + 1) * 128 + 4
            self._bins = dict(cap=cap, cursor=torch.zeros(nb + 1, dtype=torch.int32, device=dev),
                              rec=torch.empty(nb * cap, dtype=torch.int64, device=dev),
                              bitmap=torch.zeros(words, dtype=torch.int32, device=dev),
                              prefix=torch.empty(2048 + words, dtype=torch.int32, device=dev),
                              tkey=torch.empty(self.V, dtype=torch.int64, device=dev),
                              tsum=torch.empty(self.V, dtype=torch.int64, device=dev))
        return self._bins

    def _grow(self, errs):
        for n, e in enumerate(errs):
            c = self.caps[n]
            if e & 2 and self.n_bins:       # a bin overflowed (extremely skewed source ids): use the atomic passes
                self.n_bins = 0
            if e & 64:
                c["S"] = min(self.V, 2 * c["S"])
            if e & 4:
                c["K"] = min(self.V, 2 * c["K"])
            if e & 8:
                c["B"] = int(min(self.Eg, 2 * c["B"]))
        for n in range(len(self.caps) - 1):                       # a layer's seeds are the previous layer's kept nodes
            self.caps[n + 1]["S"] = max(self.caps[n + 1]["S"], self.caps[n]["K"])
        self.ws = None
        self.retries += 1

    # ------------------------------------------------------------------ torch CPU generator <-> device
    @staticmethod
    def _rng_fields(state_bytes):
        a = state_bytes.numpy()
        return a[8:12].view(np.int32), a[16:24].view(np.int64), a[24:24 + 624 * 8].view(np.uint64)

    def _stage_rng(self, snapshot):
        """Host half of the hand-over: put the generator state where the (possibly graph-captured) H2D copy reads it."""
        left, nxt, st = self._rng_fields(snapshot)
        h = self.mt_host.numpy()
        h[:624] = st.astype(np.uint32).view(np.int32)
        h[624], h[625] = int(left[0]), int(nxt[0])

    def _commit_rng(self, snapshot):
        """Make the global CPU generator continue after the numbers the device consumed."""
        left, nxt, st = self._rng_fields(snapshot)
        h = self.mt_back.numpy()
        st[:] = h[:624].view(np.uint32).astype(np.uint64)
        left[0], nxt[0] = int(h[624]), int(h[625])
        torch.set_rng_state(snapshot)

    # ------------------------------------------------------------------ the exact-shape call
    def _raise_fatal(self, bad):
        """End the call on error bits that larger buffers do not cure (the kind's rule); the other bits of _CAP_ERRS regrow."""
        rule = KINDS[self.kind]
        fatal = rule.fatal | (0 if self.n_bins else rule.fatal_no_bins)
        if bad & ~_CAP_ERRS or (bad & fatal and not rule.own_messages):
            raise RuntimeError(f"sampler kernel error 0x{bad:x}: {_lib.err_string(bad)}")
        if bad & fatal & 1:
            raise RuntimeError("frontier longer than the graph has edges (repeated seeds?) or >= 2^31 positions")
        if bad & fatal & 2:
            raise RuntimeError("candidate capacity exceeded / seed id out of range")

    def _run(self, kind, w_rows, seeds, fanouts, mode, eta, eps, draw, uniforms=None):
        """All layers enqueued, one copy of the counts, ONE sync; repeated with larger buffers -- from the same generator
        snapshot, on the same draw step -- while a capacity was exceeded.  Returns the blocks in sampling order."""
        rule = self._use(kind)
        if rule.keyed and draw.state is None:
            raise ValueError("draw='device' needs a draw_state")
        seeds = seeds.to(torch.int32).contiguous()
        L, S0 = len(fanouts), int(seeds.numel())
        self._ensure(S0, fanouts)
        snapshot = torch.get_rng_state() if rule.torch_rng and uniforms is None else None
        while True:
            counts, layers = self._enqueue(w_rows, seeds, fanouts, mode, eta, eps, uniforms, snapshot, draw)
            self.counts_host.copy_(counts, non_blocking=True)
            if snapshot is not None:
                self.mt_back.copy_(self.mt_dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()                 # the ONE sync of the step's sampling
            cnts, bad = _parse_counts(self.counts_host, L)
            self._raise_fatal(bad)
            if bad == 0:
                break
            if rule.keyed:
                draw.state.step_dev.sub_(1)                            # the repeated call is the same draw step
            self._grow([c.err for c in cnts])
            self._ensure(S0, fanouts)
        if snapshot is not None:
            self._commit_rng(snapshot)
        return [self._block(n, lay, c) for n, (lay, c) in enumerate(zip(layers, cnts))]

    def sample_blocks(self, w_rows, seeds, fanouts, mode, eta, eps=0.9999, uniforms=None, draw_state=None, layer_dependency=False):
        """The ``for block_id in reversed(range(L))`` loop of bandit_sampler.py:350-366 /
        ladies_sampler.py:112-122.  ``w_rows[n]`` / ``fanouts[n]`` are in SAMPLING order (last block
        first).  Returns the blocks in sampling order.

        ``uniforms``: optional list of fp32 vectors replacing the draws from torch's global CPU
        generator (the stream ATen's CPU ``torch.bernoulli`` consumes).
        ``draw_state`` (a DrawState): the keyed Poisson draw instead -- candidate ``nid`` of sampling layer n
        is kept iff ``keyed_uniform(seed, step, n, nid) < P`` (layer 0 for every n with ``layer_dependency``); torch's generator
        and the staged MT state are neither read nor advanced, and the call bumps the draw step once."""
        if draw_state is not None and uniforms is not None:
            raise ValueError("uniforms= replaces the stream draw; the keyed draw (draw_state=) has no uniforms to replace")
        if layer_dependency and draw_state is None:
            raise ValueError("layer_dependency belongs to the keyed draw (draw_state=)")
        return self._run("stream" if draw_state is None else "poisson_keyed", w_rows, seeds, fanouts, mode, eta, eps,
                         _Draw(draw_state, None, layer_dependency), uniforms)

    # ------------------------------------------------------------------ non-Poisson samplers (multinomial draw)
    def sample_blocks_multinomial(self, w_rows, seeds, fanouts, mode, eta, replace=False, fp32_importance=False, draw="host",
                                  draw_state=None):
        """BanditLadiesSampler / LadiesSampler (bandit_sampler.py:84-99, ladies_sampler.py:54-69): the node importances
        are computed on the device; the draw is ``torch.multinomial`` itself, on the host, on those bits (ATen's CPU
        kernel takes its exponentials from an MKL stream seeded by the global generator -- there is nothing to restate),
        so this path syncs once per layer like the reference does.  ``fp32_importance``: hand the draw fp32 importances
        (LadiesSampler's non-importance branch builds fp32 ones, ladies_sampler.py:50; ATen draws in the input's dtype).

        ``draw="device"`` (with ``draw_state``, a DrawState): the keyed draw of csrc/mn_draw.hip instead -- frontier_prob,
        multinomial_draw, multinomial_select_marked and build_block of all L layers are only enqueued and the call synchronises
        once, at the end, like sample_blocks; torch's CPU generator is not touched."""
        if draw == "device":                   # (``replace``: the keyed draw WITH replacement of csrc/replace_draw.hip, section 24)
            return self._run("multinomial_replace" if replace else "multinomial", w_rows, seeds, fanouts, mode, eta, 0.0,
                             _Draw(draw_state))
        if draw != "host":
            raise ValueError("draw must be 'host' or 'device', not %r" % (draw,))
        self._use("multinomial_host")
        seeds = seeds.to(torch.int32).contiguous()
        L, S0 = len(fanouts), int(seeds.numel())
        self._ensure(S0, fanouts)
        while True:
            dev, st = self.g.device, _stream()
            counts = torch.empty(L * 10, dtype=torch.int32, device=dev)
            eta_f, ome_f = float(np.float32(eta)), float(np.float32(1.0 - eta))
            layers, state = [], (seeds, S0, 0)
            for n in range(L):
                cur_seeds, n_seeds, n_seeds_dev = state
                c_ws, c_out, lay, cnt_ptr, kept_nid = self._layer_buffers(n, counts)
                w_pos = w_rows[n]
                _lib.check(_lib.lib.bliss_frontier_prob(C.byref(self.c_graph), C.byref(self._set(n)["c_maps"]), w_pos.data_ptr(),
                                                        cur_seeds.data_ptr(), n_seeds, n_seeds_dev, self.caps[n]["S"], mode,
                                                        eta_f, ome_f, self.Eg, C.byref(c_ws), st), "bliss_frontier_prob")
                self.counts_host.copy_(counts, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                Cn = int(self.counts_host[10 * n + 2])
                prob = self.ws[n].p[:Cn].cpu()
                if fp32_importance:
                    prob = prob.float()
                chosen = torch.multinomial(prob, min(int(fanouts[n]), Cn), replacement=replace)        # bandit_sampler.py:98
                chosen_dev = chosen.to(torch.int32).to(dev)
                _lib.check(_lib.lib.bliss_multinomial_select(C.byref(c_ws), chosen_dev.data_ptr(), int(chosen_dev.numel()), st),
                           "bliss_multinomial_select")
                _lib.check(_lib.lib.bliss_build_block(C.byref(self.c_graph), C.byref(self._set(n)["c_maps"]), w_pos.data_ptr(),
                                                      cur_seeds.data_ptr(), self.caps[n]["S"], mode, eta_f, ome_f, self.Eg,
                                                      C.byref(c_ws), C.byref(c_out), st), "bliss_build_block")
                layers.append(lay)
                state = (kept_nid, -1, cnt_ptr + 12)
            self.counts_host.copy_(counts, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            cnts, bad = _parse_counts(self.counts_host, L)
            self._raise_fatal(bad)
            if bad == 0:
                return [self._block(n, lay, c) for n, (lay, c) in enumerate(zip(layers, cnts))]
            self._grow([c.err for c in cnts])
            self._ensure(S0, fanouts)

    # ------------------------------------------------------------------ node-wise samplers (keyed per-column / per-source draws)
    def sample_blocks_neighbor(self, seeds, fanouts, draw_state, nb_prob=None, replace=False):
        """fit.NeighborSampler with ``draw="device"`` (csrc/neighbor.hip): the L layers (``fanouts`` in
        SAMPLING order) are only enqueued and the call synchronises once, at the end; torch's generators are not touched.
        ``nb_prob``: the weighted draw of csrc/neighbor_w.hip -- ``neighbor_prob(...)``'s record.
        ``replace``: the draw WITH replacement of csrc/replace_draw.hip, uniform or over a raw-mode
        ``nb_prob``."""
        kind = "neighbor_replace" if replace else "neighbor" if nb_prob is None else "wneighbor"
        return self._run(kind, None, seeds, fanouts, 0, 0.0, 0.0, _Draw(draw_state, nb_prob))

    def sample_blocks_labor(self, seeds, fanouts, draw_state, layer_dependency=False, iterations=0, lb_prob=None):
        """fit.LaborSampler (csrc/labor.hip): the L layers (``fanouts`` in SAMPLING order) are only enqueued
        and the call synchronises once, at the end; torch's generators are not touched.  ``layer_dependency``: one variate per
        vertex for all layers of a step.  ``iterations`` > 0: LABOR-i layers (fit.ImportanceLaborSampler, csrc/labor_is.hip,
        DESIGN.md section 16).  ``lb_prob``: LABOR layers with edge probabilities (csrc/labor_w.hip) --
        ``neighbor_prob(...)``'s record; the blocks then carry ``_p``, the inclusion probabilities."""
        kind = "labor_is" if iterations > 0 or self.labor_is else "labor"
        if lb_prob is not None:
            if kind == "labor_is":
                raise NotImplementedError("LABOR-i with edge probabilities is out of scope")
            kind = "wlabor"
        return self._run(kind, None, seeds, fanouts, 0, 0.0, 0.0, _Draw(draw_state, lb_prob, layer_dependency, iterations))

    # ------------------------------------------------------------------ node-wise layers: scratch (zero once, left zero by every call)
    def _zeros(self, what, *dims):
        nbytes = int(getattr(_lib.lib, what)(self.V, *dims))
        if nbytes < 0:
            raise RuntimeError(what + " failed")
        return torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device)

    def _scratch_once(self, attr, what, *dims):
        """Scratch sized once, for any seed capacity up to |V|: ``attr`` holds the tensor."""
        if getattr(self, attr) is None:
            setattr(self, attr, self._zeros(what, *dims))
        return getattr(self, attr)

    def _scratch_grown(self, attr, what, cap_s, cap_b=None):
        """Scratch sized for any seed capacity up to |V| and (``cap_b``) the largest edge capacity of the layers, regrown with
        either: ``attr`` holds (rows, tensor) or (rows, edges, tensor)."""
        scr, need = getattr(self, attr), (cap_s,) if cap_b is None else (cap_s, cap_b)
        if scr is None or any(have < n for have, n in zip(scr, need)):
            dims = (max(self.V, int(cap_s)),) + (() if cap_b is None else (max(int(cap_b), max(c["B"] for c in self.caps)),))
            scr = dims + (self._zeros(what, *dims),)
            setattr(self, attr, scr)
        return scr[-1]

    def _wlabor_p(self, n, slot, cap_b):
        """The p_ij output of weighted LABOR layer n: persistent per static slot, fresh memory per call otherwise."""
        if slot is None:
            return torch.empty(max(cap_b, 1), dtype=torch.bfloat16, device=self.g.device)
        key = (slot, n, cap_b)
        if key not in self._wl_p:
            self._wl_p[key] = torch.empty(max(cap_b, 1), dtype=torch.bfloat16, device=self.g.device)
        return self._wl_p[key]

    def neighbor_prob(self, rows, eta=None):
        """The probability source of weighted neighbor layers (csrc/neighbor_w.hip) and weighted LABOR layers (csrc/labor_w.hip).  ``rows``: bf16 [|E|] tensors by CSC position,
        one per layer in SAMPLING order (or one tensor for all layers).  ``eta`` None: raw mode, the rows are the unnormalised
        edge probabilities; a number: EXP3 mode, the rows are the EXP3 weights."""
        rows = [rows] if torch.is_tensor(rows) else list(rows)
        for r in rows:
            if r.dtype != torch.bfloat16 or r.dim() != 1 or r.numel() != self.Eg or not r.is_contiguous() or not r.is_cuda:
                raise ValueError("neighbor probabilities: contiguous bf16 [|E|] rows by CSC position on the device")
        if eta is None:
            return dict(mode=_lib.WN_RAW, rows=rows, eta_f=0.0, ome_f=0.0)
        return dict(mode=_lib.WN_EXP3, rows=rows, eta_f=float(np.float32(eta)), ome_f=float(np.float32(1.0 - eta)))

    def _enqueue_node_layer(self, n, fanout, cur_seeds, n_seeds, n_seeds_dev, draw, last, c_ws, c_out, lay, cnt_ptr, st, p_out=None):
        """The one ``*_layer`` call of a node-wise kind (KINDS: entry point, scratch, its own arguments; p_ij into ``p_out``) + the
        by-source index of its block (bliss_block_transpose on the device-resident B)."""
        rule, cap, ws = KINDS[self.kind], self.caps[n], self.ws[n]
        f, prob = int(fanout), draw.prob
        if self.kind == "neighbor_replace":
            if prob is not None and prob["mode"] != _lib.WN_RAW:
                raise NotImplementedError("the draw with replacement is the neighbor layers', uniform or over raw probabilities")
            if f == 0 or f > _lib.NR_MAX_FANOUT:
                raise ValueError("the draw with replacement takes fanouts of 1 .. %d (or negative: whole columns), not %d"
                                 % (_lib.NR_MAX_FANOUT, f))
        row = None if prob is None else prob["rows"][n if len(prob["rows"]) > 1 else 0]
        scr = rule.scratch(self, cap["S"], c_out.cap_b)
        args = (C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"], f, 0, draw.state.seed,
                draw.state.step_dev.data_ptr(), n, int(last)) + tuple(rule.tail(draw, row)) + (C.byref(c_ws), C.byref(c_out))
        if rule.p_out:
            args += (p_out.data_ptr(),)
        _lib.check(getattr(_lib.lib, rule.entry)(*args, scr.data_ptr(), st), rule.entry)
        if lay.t_indptr is None:
            return                                                     # (Block.transposed builds it on demand)
        ck, cb = cap["K"], cap["B"]
        if ws.tr_temp is None or ws.tr_temp[0] != (cb, ck):
            nbytes = int(_lib.lib.bliss_block_transpose_temp_bytes(cb, ck)) if cb else 0
            if nbytes < 0:
                raise RuntimeError("bliss_block_transpose_temp_bytes failed")
            ws.tr_temp = ((cb, ck), nbytes, torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.g.device))
        _, nbytes, temp = ws.tr_temp
        _lib.check(_lib.lib.bliss_block_transpose(lay.src.data_ptr(), cnt_ptr + 16, cb, cb, ck, lay.t_indptr.data_ptr(),
                                                  lay.t_edge.data_ptr(), temp.data_ptr(), nbytes, st), "bliss_block_transpose")

    def _layer_buffers(self, n, counts, slot=None):
        """Caller-owned outputs of layer n (one int32 and one bf16 allocation, sliced) + the C descriptors.
        ``slot``: static-shape callers keep one persistent set of outputs per slot (a pipelined train loop holds two
        batches at a time); None = fresh memory per call."""
        dev = self.g.device
        cap, ws = self.caps[n], self.ws[n]
        cs, ck, cb = cap["S"], cap["K"], cap["B"]
        build_t = cs <= 32768                     # by-source index built by the sampler kernels themselves
        if ws.src_cnt is None or ws.src_cnt.numel() < ck + 1:
            ws.src_cnt = torch.empty(ck + 1, dtype=torch.int32, device=dev)
        key = (slot, n, cs, ck, cb)
        if slot is not None and key in self._slot_bufs:
            ibuf, hbuf = self._slot_bufs[key]
        else:
            ibuf = torch.empty(_up8(cs + 1) + 4 * _up8(cb) + _up8(ck) + (2 * _up8(cb) + _up8(ck + 1) if build_t else 0),
                               dtype=torch.int32, device=dev)
            hbuf = torch.empty(2 * _up8(cb) + _up8(ck), dtype=torch.bfloat16, device=dev)
            if slot is not None:
                self._slot_bufs[key] = (ibuf, hbuf)
        o = 0
        b_indptr = ibuf[o:o + cs + 1]; o += _up8(cs + 1)
        b_src = ibuf[o:o + cb]; o += _up8(cb)
        b_dst = ibuf[o:o + cb]; o += _up8(cb)
        b_pos = ibuf[o:o + cb]; o += _up8(cb)
        b_eid = ibuf[o:o + cb]; o += _up8(cb)
        kept_nid = ibuf[o:o + ck]; o += _up8(ck)
        t_indptr = t_edge = t_scr = None
        if build_t:
            t_indptr = ibuf[o:o + ck + 1]; o += _up8(ck + 1)
            t_edge = ibuf[o:o + cb]; o += _up8(cb)
            t_scr = ibuf[o:o + cb]
        b_w = hbuf[0:cb]
        b_q = hbuf[_up8(cb):_up8(cb) + cb]
        node_prob = hbuf[2 * _up8(cb):2 * _up8(cb) + ck]
        cnt_ptr = counts.data_ptr() + 40 * n
        sset = self._set(n)                       # which set of shared scratch this layer uses
        c_ws = _lib.LayerWs(cnt_ptr, ws.seg_ptr.data_ptr(), ws.seed_acc.data_ptr(), sset["chunk_cnt"].data_ptr(),
                            ws.cand_nid.data_ptr(), ws.p.data_ptr(), ws.P.data_ptr(), ws.new_id.data_ptr(),
                            kept_nid.data_ptr(), node_prob.data_ptr(), self.hist.data_ptr(),
                            ws.src_cnt.data_ptr() if build_t else 0, cap["C"], ck)
        c_ws.kept_map, c_ws.span_seg = sset["kept_map"].data_ptr(), sset["span_seg"].data_ptr()
        e_bound = max(c.get("E", self.Eg) for c in self.caps)        # one buffer for all layers (descriptors of earlier layers stay valid)
        if e_bound <= (1 << 24):        # spill buffer for the block passes: 16 B per frontier position, only for bounded frontiers
            pos = -(-e_bound // 1024) * 1024
            if sset["kept_rec"] is None or sset["kept_rec"].numel() < pos * 2:
                sset["kept_rec"] = torch.empty(pos * 2, dtype=torch.int64, device=dev)
                sset["span_cnt"] = torch.zeros(pos // 256 + 4, dtype=torch.int32, device=dev)
            kr, sc = sset["kept_rec"], sset["span_cnt"]
            c_ws.kept_rec, c_ws.span_cnt, c_ws.kept_rec_positions = kr.data_ptr(), sc.data_ptr(), kr.numel() // 2
        if self.n_bins:
            b = self._bin_buffers()
            c_ws.n_bins, c_ws.bin_cap = self.n_bins, b["cap"]
            c_ws.bin_cursor, c_ws.bin_rec = b["cursor"].data_ptr(), b["rec"].data_ptr()
            c_ws.bitmap, c_ws.word_prefix = b["bitmap"].data_ptr(), b["prefix"].data_ptr()
            c_ws.touched_key, c_ws.touched_sum = b["tkey"].data_ptr(), b["tsum"].data_ptr()
        c_out = _lib.BlockOut(b_indptr.data_ptr(), b_src.data_ptr(), b_dst.data_ptr(), b_pos.data_ptr(), b_eid.data_ptr(),
                              b_w.data_ptr(), b_q.data_ptr(), _ptr(t_indptr), _ptr(t_edge), _ptr(t_scr), cb)
        lay = _LayerOut(b_indptr, b_src, b_dst, b_pos, b_eid, b_w, b_q, kept_nid, node_prob, counts[10 * n:10 * n + 10], t_indptr, t_edge)
        return c_ws, c_out, lay, cnt_ptr, kept_nid

    # ------------------------------------------------------------------ static-shape (graph-capturable) variant
    def set_static_caps(self, S0, fanouts, max_sizes, k_margin=1.5, b_margin=3.0):
        """Fix the capacities from sizes observed in exact mode (``max_sizes[n] = dict(K=, B=)`` in sampling
        order).  Static shapes mean no host round trip inside a step and a step that can be captured in a HIP graph;
        the price is that a step whose true sizes exceed these capacities is detected only afterwards."""
        self.caps, self.ws = static_caps(self.kind, self.V, self.Eg, S0, fanouts, max_sizes, k_margin, b_margin), None
        self._ensure(S0, fanouts)

    def stage_rng_from_torch(self):
        """Host side, before enqueueing / replaying a static step: snapshot torch's CPU generator for the device."""
        self._static_snapshot = torch.get_rng_state()
        self._stage_rng(self._static_snapshot)

    def static_rng_begin(self, chain_rng=False):
        """Start the random-number generator of the NEXT enqueue_static(..., external_rng=True) now, on the current stream:
        a pipelined loop calls this before the sampler's other inputs are ready, so the serial MT19937 chain is off the
        critical path.  Plain launches (not graph-captured): the generator runs on the library's own stream."""
        if not chain_rng:
            self.mt_dev.copy_(self.mt_host, non_blocking=True)
        _lib.check(_lib.lib.bliss_rng_stream_begin(self.mt_dev.data_ptr(), self.rng_ctl.data_ptr(), self.rng_out.data_ptr(),
                                                   self.rng_raw.data_ptr(), self.rng_cap, _stream()), "bliss_rng_stream_begin")

    def static_rng_end(self, slot=0):
        """Join the generator started by static_rng_begin and leave the state after exactly sum(C) draws in mt_dev / mt_back."""
        _lib.check(_lib.lib.bliss_rng_stream_end(self.mt_dev.data_ptr(), self.rng_ctl.data_ptr(), self.rng_raw.data_ptr(),
                                                 self.rng_cap, self._slot_counts[slot].data_ptr() + 20, _stream()), "bliss_rng_stream_end")
        self.mt_back.copy_(self.mt_dev, non_blocking=True)
        self._slot_counts_host[slot].copy_(self._slot_counts[slot], non_blocking=True)

    def static_rng_chain(self, slot, counts_host):
        """static_rng_end(slot) + static_rng_begin(chain_rng=True) without touching the current stream: the hand-over runs on
        the generator's own stream (bliss_rng_stream_chain), ordered after what the current stream holds now (the sampler of
        ``slot``); the counts records of ``slot`` arrive in ``counts_host`` (a pinned int32 tensor or a view of one).  Call
        static_rng_ready() before enqueueing the next sampler.  The generator state is not handed back to the host: finish a
        chain with static_rng_end."""
        cd = self._slot_counts[slot]
        assert counts_host.is_pinned() and counts_host.numel() >= cd.numel() and counts_host.dtype == torch.int32
        _lib.check(_lib.lib.bliss_rng_stream_chain(self.mt_dev.data_ptr(), self.rng_ctl.data_ptr(), self.rng_out.data_ptr(),
                                                   self.rng_raw.data_ptr(), self.rng_cap, cd.data_ptr(), cd.numel(),
                                                   counts_host.data_ptr(), _stream()), "bliss_rng_stream_chain")

    def static_rng_record(self, event):
        """Record ``event`` on the generator's stream, i.e. behind the hand-over kernel of the last static_rng_chain (which
        wrote that call's counts_host) and the generator it started."""
        if getattr(self, "_gen_stream", None) is None:
            h = int(_lib.lib.bliss_rng_stream_handle())
            if not h:
                raise RuntimeError("bliss_rng_stream_handle failed")
            self._gen_stream = torch.cuda.ExternalStream(h)
        event.record(self._gen_stream)

    def static_rng_ready(self):
        _lib.check(_lib.lib.bliss_rng_stream_ready(_stream()), "bliss_rng_stream_ready")

    def enqueue_static(self, w_rows, seeds, fanouts, mode, eta, eps=0.9999, slot=0, chain_rng=False, external_rng=False, part=None,
                       last_block=True, ready_flag=0, n_live_dev=None, draw=_Draw()):
        """Enqueue one sample_blocks on the current stream with capacity-padded outputs and NO sync.  Returns the
        blocks (sampling order); sizes, errors and the generator state are read back by finish().  The layers are of the
        engine's ``kind`` (KINDS); the node-wise kinds ignore ``w_rows`` / ``mode`` / ``eta`` / ``eps``.

        ``slot``: which persistent set of output buffers to fill.  ``chain_rng``: continue from the generator state the
        previous enqueue left on the device instead of the host-staged one (several batches sampled per host round trip).
        ``part``: None = the whole call.  "main" = everything except the blocks of all but the last-sampled layer, and layer
        n raises ``flags[n]`` when it starts; "early_blocks" = only those blocks, each behind a bliss_flag_wait on
        ``flags[n + 1]`` -- to be enqueued on ANOTHER stream, with ``scratch_sets`` >= the number of layers (block n then shares
        no scratch with any later layer) and external_rng.  The caller orders the next "main" after both parts.
        ``last_block=False`` with "main": the last-sampled layer's block is left out as well and ``flags[L]`` is raised at the end
        (its draw is done); part "last_block" = only that block, behind a bliss_flag_wait on ``flags[L]``; ``ready_flag``
        (address of a device flag) is raised as soon as the block's forward arrays are final, before its by-source index.
        Only the "stream" kind has a generator to chain or run externally and a split enqueue; every other kind is enqueued
        as a whole call.
        ``draw`` (a _Draw): the DrawState of the keyed kinds, the ``neighbor_prob(...)`` record of the weighted ones (the
        blocks of weighted LABOR layers then carry ``_p``, the inclusion probabilities), ``layer_dependency`` (keyed Poisson,
        LABOR: one variate per node for all layers) and LABOR-i's ``iterations``.
        ``n_live_dev`` (an int32 word on the device): ``seeds`` is a buffer of CAPACITY length -- the
        capacity the static shapes were fixed for -- of which only the first ``n_live_dev[0]`` slots are this batch's seeds.
        The first-sampled layer is then launched like every later one, with its seed count read on the device, so a captured
        call serves every batch size up to the capacity; the output block's counts record holds the live S.  Slots past the
        live count are read for no result (they hold valid node ids: zero, or an earlier batch's).  Whole calls only."""
        rule = KINDS[self.kind]
        whole = part is None and not external_rng and not chain_rng
        if self.kind == "multinomial_host":
            raise NotImplementedError("torch.multinomial on the host syncs per layer: no static-shape enqueue")
        if rule.keyed and draw.state is None:
            raise ValueError("the %s layers need a draw_state" % self.kind)
        if not whole and (n_live_dev is not None or not rule.split):
            raise NotImplementedError("a live seed count and the %s layers have no split / external-generator enqueue (the "
                                      "pipelined two-stream loop is out of scope)" % self.kind)
        if n_live_dev is not None:
            if not (torch.is_tensor(n_live_dev) and n_live_dev.dtype == torch.int32 and n_live_dev.numel() == 1
                    and n_live_dev.device == self.g.device):
                raise ValueError("n_live_dev: one int32 word on the graph's device")
            if self.caps is None or int(seeds.numel()) != self.caps[0]["S"] or seeds.dtype != torch.int32 or not seeds.is_contiguous():
                raise ValueError("a live seed count needs a contiguous int32 seed buffer of exactly the static seed capacity (%s), "
                                 "got %d slots" % (None if self.caps is None else self.caps[0]["S"], int(seeds.numel())))
        if part is not None and (self.scratch_sets < len(fanouts) or not external_rng):
            raise ValueError("split enqueue needs one scratch set per layer and an external generator")
        L = len(fanouts)
        counts_dev, layers = self._enqueue(w_rows, seeds, fanouts, mode, eta, eps, None, True, draw, slot=slot, chain_rng=chain_rng,
                                           external_rng=external_rng, part=part, last_block=last_block, ready_flag=ready_flag,
                                           n_live_dev=n_live_dev)
        self._static_draw[slot] = rule.keyed
        if slot not in self._slot_counts_host:
            self._slot_counts_host[slot] = torch.empty(L * 10, dtype=torch.int32).pin_memory()
        if not external_rng:                     # (external: static_rng_end copies both, off the consumer's critical path)
            self._slot_counts_host[slot].copy_(counts_dev, non_blocking=True)
            if not rule.keyed:
                self.mt_back.copy_(self.mt_dev, non_blocking=True)
        blocks = [self._block(n, lay, None, counts_dev) for n, lay in enumerate(layers)]
        self._static[slot] = (blocks, L)    # kept: a captured graph replays this enqueue without re-running it
        return blocks

    def finish(self, slot=0, commit=True):
        """After the stream has been synchronised: true sizes, error check, generator hand-back."""
        blocks, L = self._static[slot]
        cnts, bad = _parse_counts(self._slot_counts_host[slot], L)
        for b, c in zip(blocks, cnts):
            b._counts = c
        if commit and not self._static_draw.get(slot):       # (the device draw consumed nothing from torch's generator)
            self._commit_rng(self._static_snapshot)
        if bad:
            raise RuntimeError(f"static-shape step exceeded its capacities or hit a kernel error 0x{bad:x} "
                               f"({_lib.err_string(bad)}); the step's results are invalid -- raise the margins")
        return cnts

    def _enqueue(self, w_rows, seeds, fanouts, mode, eta, eps, uniforms, snapshot, draw, slot=None, chain_rng=False, external_rng=False,
                 part=None, last_block=True, ready_flag=0, n_live_dev=None):
        """The launches of one call of the engine's kind, on the current stream; returns (counts on the device, [_LayerOut])."""
        kind, rule, draw_state = self.kind, KINDS[self.kind], draw.state
        poisson = kind in ("stream", "poisson_keyed")
        if (draw.prob is None) if rule.prob == "any" else (draw.prob is not None and rule.prob is None):
            raise ValueError("the %s layers %s" % (kind, "need neighbor_prob(...)'s record" if rule.prob else "take no probabilities"))
        dev, st = self.g.device, _stream()
        L = len(fanouts)
        if not rule.keyed and snapshot is not None and not chain_rng and not external_rng:
            if snapshot is not True:
                self._stage_rng(snapshot)
            self.mt_dev.copy_(self.mt_host, non_blocking=True)
        if slot is None:
            counts = torch.empty(L * 10, dtype=torch.int32, device=dev)
        else:
            if slot not in self._slot_counts or self._slot_counts[slot].numel() != L * 10:
                self._slot_counts[slot] = torch.empty(L * 10, dtype=torch.int32, device=dev)
            counts = self._slot_counts[slot]
        use_rng = uniforms is None and not rule.keyed
        if use_rng and not external_rng:      # fork the generator: it runs beside everything below
            _lib.check(_lib.lib.bliss_rng_stream_begin(self.mt_dev.data_ptr(), self.rng_ctl.data_ptr(), self.rng_out.data_ptr(),
                                                       self.rng_raw.data_ptr(), self.rng_cap, st), "bliss_rng_stream_begin")
        eta_f = float(np.float32(eta))
        ome_f = float(np.float32(1.0 - eta))
        layers = []
        self._wl_out = []                       # the p_ij outputs of weighted LABOR layers, in sampling order
        cur_seeds, n_seeds, n_seeds_dev = seeds, int(seeds.numel()), 0
        if n_live_dev is not None:              # the first-sampled layer reads its seed count on the device, like the others
            n_seeds, n_seeds_dev = -1, n_live_dev.data_ptr()
        for n in range(L):
            cap = self.caps[n]
            cs, ws = cap["S"], self.ws[n]
            c_ws, c_out, lay, cnt_ptr, kept_nid = self._layer_buffers(n, counts, slot)
            last = n == L - 1
            if rule.family == "node":           # neighbor / LABOR layer: 6 / 7 launches and the by-source index, nothing else
                p_out = None
                if rule.p_out:
                    p_out = self._wlabor_p(n, slot, cap["B"])
                    self._wl_out.append(p_out)
                self._enqueue_node_layer(n, fanouts[n], cur_seeds, n_seeds, n_seeds_dev, draw, last, c_ws, c_out, lay, cnt_ptr, st, p_out)
                layers.append(lay)
                cur_seeds, n_seeds, n_seeds_dev = kept_nid, -1, cnt_ptr + 12
                continue
            w_pos = w_rows[n]
            if part == "main":                  # layer n raises flag n when it starts (= everything before it has completed)
                c_ws.entry_flag = self.flags.data_ptr() + 4 * n
            if part in (None, "main"):          # candidates, probabilities, draw: all the next layer needs (its seeds = kept_nid)
                if poisson and self.n_bins and self.fuse_scale:
                    # the Poisson scale rides in the last workgroup of the candidate numbering (one launch less per layer)
                    c_ws.fs_ticket = self.fs_ticket.data_ptr()
                    c_ws.fs_fanout, c_ws.fs_eps = int(fanouts[n]), float(eps)
                    if use_rng:
                        c_ws.fs_rng_ctl, c_ws.fs_layer_off = self.rng_ctl.data_ptr(), self.rng_ctl.data_ptr() + 4 * (8 + n)
                        c_ws.fs_is_last, c_ws.fs_rng_cap = int(n == L - 1), self.rng_cap
                _lib.check(_lib.lib.bliss_frontier_prob(C.byref(self.c_graph), C.byref(self._set(n)["c_maps"]), w_pos.data_ptr(),
                                                        cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cs, mode, eta_f, ome_f,
                                                        cap.get("E", self.Eg), C.byref(c_ws), st), "bliss_frontier_prob")
                if kind == "multinomial_replace":   # the keyed categorical draw with replacement: 3 launches, the same mark format
                    if ws.rdraw_scr is None:
                        nbytes = int(_lib.lib.bliss_multinomial_draw_replace_scratch_bytes(cap["C"]))
                        ws.rdraw_scr = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
                    _lib.check(_lib.lib.bliss_multinomial_draw_replace(ws.p.data_ptr(), cnt_ptr, cap["C"], int(fanouts[n]), 0,
                                                                       draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                                       ws.rdraw_scr.data_ptr(), ws.new_id.data_ptr(), 0, st),
                               "bliss_multinomial_draw_replace")
                elif kind == "multinomial":     # the keyed race: 5 launches
                    _lib.check(_lib.lib.bliss_multinomial_draw(ws.cand_nid.data_ptr(), ws.p.data_ptr(), cnt_ptr, cap["C"], int(fanouts[n]), 0,
                                                               draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                               ws.draw_scr.data_ptr(), ws.keys.data_ptr(), ws.new_id.data_ptr(), st),
                               "bliss_multinomial_draw")
                elif kind == "poisson_keyed":   # keyed Poisson draw: no generator, no uniforms buffer; the last select bumps the step
                    _lib.check(_lib.lib.bliss_poisson_select_keyed(C.byref(c_ws), int(fanouts[n]), float(eps), draw_state.seed,
                                                                   draw_state.step_dev.data_ptr(), 0 if draw.layer_dependency else n,
                                                                   int(last), cap["C"], st), "bliss_poisson_select_keyed")
                elif use_rng:
                    off_ptr = self.rng_ctl.data_ptr() + 4 * (8 + n)
                    _lib.check(_lib.lib.bliss_poisson_select(C.byref(c_ws), int(fanouts[n]), float(eps), self.rng_out.data_ptr(),
                                                             off_ptr, self.rng_ctl.data_ptr(), int(n == L - 1), self.rng_cap,
                                                             cap["C"], st), "bliss_poisson_select")
                else:
                    u = uniforms[n].to(dev, torch.float32).reshape(-1)
                    m = min(u.numel(), cap["C"])
                    ws.uniforms[:m].copy_(u[:m])
                    _lib.check(_lib.lib.bliss_poisson_select(C.byref(c_ws), int(fanouts[n]), float(eps), ws.uniforms.data_ptr(),
                                                             0, 0, 0, 0, cap["C"], st), "bliss_poisson_select")
                if not poisson:                 # (both multinomial draws leave marks: 4 launches)
                    _lib.check(_lib.lib.bliss_multinomial_select_marked(C.byref(c_ws), st), "bliss_multinomial_select_marked")
            # the block of this layer: nothing the next layer's candidate pipeline reads or writes (own scratch set)
            if part is None or (part == "main" and last and last_block) or (part == "early_blocks" and not last) or \
                    (part == "last_block" and last):
                if part == "last_block" and ready_flag:
                    c_ws.block_ready_flag = int(ready_flag)
                if part in ("early_blocks", "last_block"):   # on another stream: wait until layer n + 1 has started (the last
                    # layer: until the "main" part has raised flags[L]), i.e. layer n's draw is done
                    _lib.check(_lib.lib.bliss_flag_wait(self.flags.data_ptr() + 4 * (n + 1), self.flag_err.data_ptr(), st), "bliss_flag_wait")
                _lib.check(_lib.lib.bliss_build_block(C.byref(self.c_graph), C.byref(self._set(n)["c_maps"]), w_pos.data_ptr(),
                                                      cur_seeds.data_ptr(), cs, mode, eta_f, ome_f, cap.get("E", self.Eg), C.byref(c_ws),
                                                      C.byref(c_out), st), "bliss_build_block")
            layers.append(lay)
            cur_seeds, n_seeds, n_seeds_dev = kept_nid, -1, cnt_ptr + 12          # next layer: S = this layer's K
        if part == "main" and not last_block:
            _lib.check(_lib.lib.bliss_flag_raise(self.flags.data_ptr() + 4 * L, st), "bliss_flag_raise")
        if use_rng and not external_rng:      # join; mt_dev = generator state after exactly sum(C) draws
            _lib.check(_lib.lib.bliss_rng_stream_end(self.mt_dev.data_ptr(), self.rng_ctl.data_ptr(), self.rng_raw.data_ptr(),
                                                     self.rng_cap, counts.data_ptr() + 20, _stream()), "bliss_rng_stream_end")
        return counts, layers

    def _block(self, n, lay, c, counts_dev=None):
        """The Block of layer n from its outputs.  ``c`` (its LayerCounts): sliced to the true sizes, with the candidate pipeline's
        _trace.  None: the static path's capacity-sized block -- true sizes stay on the device (``_nnz_ptr`` into
        ``counts_dev``) and ``_counts`` is filled in by finish()."""
        cap, rule = self.caps[n], KINDS[self.kind]
        S, K, B = (cap["S"], cap["K"], cap["B"]) if c is None else (c.S, c.K, c.B)
        cut = (lambda t, m: t) if c is None else (lambda t, m: t[:m])      # (capacity-sized: the buffers as they are)
        blk = Block(self.g, K, S, cut(lay.indptr, S + 1), cut(lay.src, B), cut(lay.dst, B), cut(lay.pos, B), cut(lay.eid, B),
                    cut(lay.kept_nid, K))
        blk._edge_weights, blk._q, blk._node_prob = cut(lay.w, B), cut(lay.q, B), cut(lay.node_prob, K)
        if rule.p_out:
            blk._p = self._wl_out[n][:B]
        blk._counts, blk._counts_dev = c, lay.counts
        if lay.t_indptr is not None:
            blk._transposed = (cut(lay.t_indptr, K + 1), cut(lay.t_edge, max(B, 1)))
        if c is None:
            blk._nnz_ptr = counts_dev.data_ptr() + 40 * n + 16
            blk._xcap = int(cap.get("X", cap["B"]))
            blk._trace = {}
            return blk
        ws = self.ws[n]
        blk._trace = dict(p=ws.p[:c.C], P=ws.P[:c.C], cand_nid=ws.cand_nid[:c.C], new_id=ws.new_id[:c.C])
        if rule.keys:
            blk._trace["keys"] = ws.keys[:c.C]
        return blk
