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
import contextlib
import ctypes as C
import os

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

    def __init__(self, g: Graph):
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
        self.exact_k = False                # device-drawn multinomial layers keep at most fanout + S nodes: K capacities are that bound
        self.exact_b = False                # neighbor layers keep at most fanout edges per seed: B capacities are that bound
        self.nb_replace = False             # neighbor layers drawn WITH replacement hold exactly fanout edges per non-empty column: B <= S * fanout, not |E|
        self._nr_scr = None                 # csrc/replace_draw.hip's node-wise draw: csrc/neighbor.hip's words
        self._nb_scr = None                 # csrc/neighbor.hip: tickets + node bitmap (zero once, left zero by every call)
        self._wn_scr = None                 # csrc/neighbor_w.hip: the same words + a record per seed and a staged key per CSC position
        self._lb_scr = None                 # csrc/labor.hip: the same words + one kept count per seed column; (cap_s, tensor)
        self.labor_is = False               # LABOR layers run csrc/labor_is.hip also with 0 iterations (fit.ImportanceLaborSampler)
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
    def _init_caps(self, S0, fanouts_sampling_order):
        caps, s = [], int(S0)
        for f in fanouts_sampling_order:
            k = min(self.V, int(1.25 * (f + s)) + 64)
            caps.append(dict(S=s, C=self.V, K=k, B=int(min(self.Eg, max(1 << 16, 48 * k)))))
            s = k
        return caps

    def _ensure(self, S0, fan):
        if self.caps is None or len(self.caps) != len(fan):
            self.caps = self._init_caps(S0, fan)
            self.ws = None
        elif self.caps[0]["S"] < S0:
            fresh = self._init_caps(S0, fan)
            self.caps = [{k: max(a[k], b[k]) for k in a} for a, b in zip(self.caps, fresh)]
            self.ws = None
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

    # ------------------------------------------------------------------ one sample_blocks call
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
        seeds = seeds.to(torch.int32).contiguous()
        L = len(fanouts)
        self._ensure(int(seeds.numel()), fanouts)
        snapshot = torch.get_rng_state() if uniforms is None and draw_state is None else None
        while True:
            out = self._enqueue(w_rows, seeds, fanouts, mode, eta, eps, uniforms, snapshot, draw_state=draw_state,
                                poisson=draw_state is not None, layer_dependency=layer_dependency)
            counts_dev = out[0]
            self.counts_host.copy_(counts_dev, non_blocking=True)
            if snapshot is not None:
                self.mt_back.copy_(self.mt_dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()                 # the ONE sync of the step's sampling
            raw = self.counts_host.numpy().tobytes()
            cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
            errs = [c.err for c in cnts]
            bad = 0
            for e in errs:
                bad |= e
            if bad & ~_CAP_ERRS:
                raise RuntimeError(f"sampler kernel error 0x{bad:x}: {_lib.err_string(bad)}")
            if bad & 1:
                raise RuntimeError("frontier longer than the graph has edges (repeated seeds?) or >= 2^31 positions")
            if bad & 2 and not self.n_bins:
                raise RuntimeError("candidate capacity exceeded / seed id out of range")
            if bad == 0:
                break
            if draw_state is not None:
                draw_state.step_dev.sub_(1)                            # the repeated call is the same draw step
            self._grow(errs)
            self._ensure(int(seeds.numel()), fanouts)
        if snapshot is not None:
            self._commit_rng(snapshot)
        return self._finish(out, cnts)

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
            return self._sample_blocks_mn_device(w_rows, seeds, fanouts, mode, eta, draw_state, replace=bool(replace))
        if draw != "host":
            raise ValueError("draw must be 'host' or 'device', not %r" % (draw,))
        seeds = seeds.to(torch.int32).contiguous()
        L = len(fanouts)
        self._ensure(int(seeds.numel()), fanouts)
        # a multinomial draw keeps min(num, C) nodes plus the seeds: make room
        for n in range(L):
            need = min(self.V, fanouts[n] + self.caps[n]["S"] + 64)
            if self.caps[n]["K"] < need:
                self.caps[n]["K"] = need
            if n + 1 < L and self.caps[n + 1]["S"] < self.caps[n]["K"]:
                self.caps[n + 1]["S"] = self.caps[n]["K"]
                self.ws = None
        self._ensure(int(seeds.numel()), fanouts)
        while True:
            dev, st = self.g.device, _stream()
            counts = torch.empty(L * 10, dtype=torch.int32, device=dev)
            eta_f, ome_f = float(np.float32(eta)), float(np.float32(1.0 - eta))
            layers, state = [], (seeds, int(seeds.numel()), 0)
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
            raw = self.counts_host.numpy().tobytes()
            cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
            bad = 0
            for c in cnts:
                bad |= c.err
            if bad & ~_CAP_ERRS or bad & 2:
                raise RuntimeError(f"sampler kernel error 0x{bad:x}: {_lib.err_string(bad)}")
            if bad == 0:
                return self._finish((counts, layers), cnts)
            self._grow([c.err for c in cnts])
            self._ensure(int(seeds.numel()), fanouts)

    def _mn_exact_caps(self, fanouts):
        """A device-drawn layer keeps union(drawn, seeds): at most fanout + S nodes, so that is its K capacity."""
        for n in range(len(fanouts)):
            need = min(self.V, int(fanouts[n]) + self.caps[n]["S"])
            if self.caps[n]["K"] < need:
                self.caps[n]["K"] = need
            if n + 1 < len(fanouts) and self.caps[n + 1]["S"] < self.caps[n]["K"]:
                self.caps[n + 1]["S"] = self.caps[n]["K"]
                self.ws = None

    def _sample_blocks_mn_device(self, w_rows, seeds, fanouts, mode, eta, draw_state, replace=False):
        if draw_state is None:
            raise ValueError("draw='device' needs a draw_state")
        seeds = seeds.to(torch.int32).contiguous()
        L = len(fanouts)
        self._ensure(int(seeds.numel()), fanouts)
        self._mn_exact_caps(fanouts)
        self._ensure(int(seeds.numel()), fanouts)
        while True:
            out = self._enqueue(w_rows, seeds, fanouts, mode, eta, 0.0, None, None, draw_state=draw_state, replace=replace)
            self.counts_host.copy_(out[0], non_blocking=True)
            torch.cuda.current_stream().synchronize()                 # the one sync of the call
            raw = self.counts_host.numpy().tobytes()
            cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
            bad = 0
            for c in cnts:
                bad |= c.err
            if bad & ~_CAP_ERRS or bad & 1 or (bad & 2 and not self.n_bins):
                raise RuntimeError(f"sampler kernel error 0x{bad:x}: {_lib.err_string(bad)}")
            if bad == 0:
                return self._finish(out, cnts, keys=not replace)
            draw_state.step_dev.sub_(1)                                # the repeated call is the same draw step
            self._grow([c.err for c in cnts])
            self._ensure(int(seeds.numel()), fanouts)
            self._mn_exact_caps(fanouts)
            self._ensure(int(seeds.numel()), fanouts)

    # ------------------------------------------------------------------ neighbor sampler (keyed per-column draw)
    def _nb_caps(self, S0, fanouts):
        """Capacities of neighbor layers from their bounds: a layer keeps at most ``fanout`` edges per seed (B exactly bounded
        when fanout >= 0) and, besides its seeds, at most one new source per kept edge."""
        caps, s = [], int(S0)
        for f in fanouts:
            f = int(f)
            b = int(min(self.Eg, s * f)) if f >= 0 else int(min(self.Eg, max(1 << 16, 48 * s)))
            if self.nb_replace and f >= 0:      # (a column of fewer than f edges holds f block edges: |E| is no bound)
                b = int(min(2 ** 31 - 1, s * f))
            k = int(min(self.V, s + min(b, self.Eg))) if f >= 0 else self.V
            caps.append(dict(S=s, C=self.V, K=k, B=b))
            s = k
        return caps

    def _ensure_neighbor(self, S0, fan):
        if self.caps is None or len(self.caps) != len(fan) or self.caps[0]["S"] < S0:
            fresh = self._nb_caps(S0, fan)
            if self.caps is not None and len(self.caps) == len(fan):
                fresh = [{k: max(a.get(k, 0), b[k]) for k in b} for a, b in zip(self.caps, fresh)]
            self.caps, self.ws = fresh, None
        self._ensure(S0, fan)

    def sample_blocks_neighbor(self, seeds, fanouts, draw_state, nb_prob=None, replace=False):
        """fit.NeighborSampler with ``draw="device"`` (csrc/neighbor.hip): the L layers (``fanouts`` in
        SAMPLING order) are only enqueued and the call synchronises once, at the end; torch's generators are not touched.
        ``nb_prob``: the weighted draw of csrc/neighbor_w.hip -- ``neighbor_prob(...)``'s record.
        ``replace``: the draw WITH replacement of csrc/replace_draw.hip, uniform or over a raw-mode
        ``nb_prob``."""
        if draw_state is None:
            raise ValueError("draw='device' needs a draw_state")
        seeds = seeds.to(torch.int32).contiguous()
        L = len(fanouts)
        if bool(replace) != self.nb_replace:
            self.nb_replace, self.caps, self.ws = bool(replace), None, None
        self._ensure_neighbor(int(seeds.numel()), fanouts)
        while True:
            out = self._enqueue(None, seeds, fanouts, 0, 0.0, 0.0, None, None, draw_state=draw_state, neighbor=True, nb_prob=nb_prob,
                                nb_replace=bool(replace))
            self.counts_host.copy_(out[0], non_blocking=True)
            torch.cuda.current_stream().synchronize()                 # the one sync of the call
            raw = self.counts_host.numpy().tobytes()
            cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
            bad = 0
            for c in cnts:
                bad |= c.err
            if bad & ~_CAP_ERRS or bad & 3:
                raise RuntimeError(f"sampler kernel error 0x{bad:x}: {_lib.err_string(bad)}")
            if bad == 0:
                return self._finish(out, cnts)
            draw_state.step_dev.sub_(1)                                # the repeated call is the same draw step
            self._grow([c.err for c in cnts])
            self._ensure_neighbor(int(seeds.numel()), fanouts)

    # ------------------------------------------------------------------ LABOR-0 sampler (keyed per-source draw)
    def _lb_caps(self, S0, fanouts):
        """Starting capacities of LABOR layers.  A column keeps ``fanout`` edges in expectation, not at most: B is NOT exactly
        bounded, so it starts at twice the expectation (the neighbor rule for fanout < 0) and the regrow loop covers the rest."""
        caps, s = [], int(S0)
        for f in fanouts:
            f = int(f)
            b = int(min(self.Eg, 2 * s * f + 4096)) if f >= 0 else int(min(self.Eg, max(1 << 16, 48 * s)))
            k = int(min(self.V, s + b)) if f >= 0 else self.V
            caps.append(dict(S=s, C=self.V, K=k, B=b))
            s = k
        return caps

    def _ensure_labor(self, S0, fan):
        if self.caps is None or len(self.caps) != len(fan) or self.caps[0]["S"] < S0:
            fresh = self._lb_caps(S0, fan)
            if self.caps is not None and len(self.caps) == len(fan):
                fresh = [{k: max(a.get(k, 0), b[k]) for k in b} for a, b in zip(self.caps, fresh)]
            self.caps, self.ws = fresh, None
        self._ensure(S0, fan)

    def sample_blocks_labor(self, seeds, fanouts, draw_state, layer_dependency=False, iterations=0, lb_prob=None):
        """fit.LaborSampler (csrc/labor.hip): the L layers (``fanouts`` in SAMPLING order) are only enqueued
        and the call synchronises once, at the end; torch's generators are not touched.  ``layer_dependency``: one variate per
        vertex for all layers of a step.  ``iterations`` > 0: LABOR-i layers (fit.ImportanceLaborSampler, csrc/labor_is.hip,
        DESIGN.md section 16).  ``lb_prob``: LABOR layers with edge probabilities (csrc/labor_w.hip) --
        ``neighbor_prob(...)``'s record; the blocks then carry ``_p``, the inclusion probabilities."""
        if draw_state is None:
            raise ValueError("the LABOR sampler needs a draw_state")
        seeds = seeds.to(torch.int32).contiguous()
        L = len(fanouts)
        self._ensure_labor(int(seeds.numel()), fanouts)
        while True:
            out = self._enqueue(None, seeds, fanouts, 0, 0.0, 0.0, None, None, draw_state=draw_state, labor=True,
                                layer_dependency=layer_dependency, labor_iterations=iterations, lb_prob=lb_prob)
            self.counts_host.copy_(out[0], non_blocking=True)
            torch.cuda.current_stream().synchronize()                 # the one sync of the call
            raw = self.counts_host.numpy().tobytes()
            cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
            bad = 0
            for c in cnts:
                bad |= c.err
            if bad & ~_CAP_ERRS or bad & 3:
                raise RuntimeError(f"sampler kernel error 0x{bad:x}: {_lib.err_string(bad)}")
            if bad == 0:
                blocks = self._finish(out, cnts)
                for blk, c, p in zip(blocks, cnts, self._wl_out if lb_prob is not None else ()):
                    blk._p = p[:c.B]
                return blocks
            draw_state.step_dev.sub_(1)                                # the repeated call is the same draw step
            self._grow([c.err for c in cnts])
            self._ensure_labor(int(seeds.numel()), fanouts)

    def _labor_scratch(self, cap_s):
        if self._lb_scr is None or self._lb_scr[0] < cap_s:           # (sized once for any seed capacity up to |V|)
            rows = max(self.V, int(cap_s))
            nbytes = int(_lib.lib.bliss_labor_scratch_bytes(self.V, rows))
            self._lb_scr = (rows, torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device))
        return self._lb_scr[1]

    def _labor_is_scratch(self, cap_s, cap_b):
        """Sized once for any seed capacity up to |V| and the largest edge capacity of the layers; regrows with B."""
        if self._li_scr is None or self._li_scr[0] < cap_s or self._li_scr[1] < cap_b:
            rows, edges = max(self.V, int(cap_s)), max(int(cap_b), max(c["B"] for c in self.caps))
            nbytes = int(_lib.lib.bliss_labor_is_scratch_bytes(self.V, rows, edges))
            if nbytes < 0:
                raise RuntimeError("bliss_labor_is_scratch_bytes failed")
            self._li_scr = (rows, edges, torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device))
        return self._li_scr[2]

    def _wlabor_scratch(self, cap_s, cap_b):
        """Sized once for any seed capacity up to |V| and the largest edge capacity of the layers; regrows with B."""
        if self._wl_scr is None or self._wl_scr[0] < cap_s or self._wl_scr[1] < cap_b:
            rows, edges = max(self.V, int(cap_s)), max(int(cap_b), max(c["B"] for c in self.caps))
            nbytes = int(_lib.lib.bliss_wlabor_scratch_bytes(self.V, rows, edges))
            if nbytes < 0:
                raise RuntimeError("bliss_wlabor_scratch_bytes failed")
            self._wl_scr = (rows, edges, torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device))
        return self._wl_scr[2]

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

    def _wneighbor_scratch(self):
        if self._wn_scr is None:                                      # (sized once for any seed capacity up to |V|)
            nbytes = int(_lib.lib.bliss_wneighbor_scratch_bytes(self.V, self.V, self.Eg))
            if nbytes < 0:
                raise RuntimeError("bliss_wneighbor_scratch_bytes failed")
            self._wn_scr = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device)
        return self._wn_scr

    def _enqueue_neighbor_layer(self, n, fanout, cur_seeds, n_seeds, n_seeds_dev, draw_state, last, c_ws, c_out, lay, cnt_ptr, st,
                                labor=False, layer_dependency=False, labor_iterations=0, nb_prob=None, lb_prob=None, p_out=None,
                                nb_replace=False):
        """One bliss_neighbor_layer (``labor``: one bliss_labor_layer, or one bliss_labor_is_layer when ``labor_iterations`` > 0, or
        one bliss_wlabor_layer with ``lb_prob``, its p_ij into ``p_out``; ``nb_prob``: one bliss_wneighbor_layer) + the by-source
        index of its block (bliss_block_transpose on the device-resident B).  ``nb_replace``: one bliss_neighbor_replace_layer,
        uniform or over the raw-mode ``nb_prob``."""
        cap, ws = self.caps[n], self.ws[n]
        if nb_replace:
            if labor or (nb_prob is not None and nb_prob["mode"] != _lib.WN_RAW):
                raise NotImplementedError("the draw with replacement is the neighbor layers', uniform or over raw probabilities")
            f = int(fanout)
            if f == 0 or f > _lib.NR_MAX_FANOUT:
                raise ValueError("the draw with replacement takes fanouts of 1 .. %d (or negative: whole columns), not %d"
                                 % (_lib.NR_MAX_FANOUT, f))
            if self._nr_scr is None:
                nbytes = int(_lib.lib.bliss_neighbor_replace_scratch_bytes(self.V, 1))
                self._nr_scr = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device)
            row = None if nb_prob is None else nb_prob["rows"][n if len(nb_prob["rows"]) > 1 else 0]
            _lib.check(_lib.lib.bliss_neighbor_replace_layer(C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"],
                                                             f, 0, draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                             _ptr(row), 0, C.byref(c_ws), C.byref(c_out), self._nr_scr.data_ptr(), st),
                       "bliss_neighbor_replace_layer")
        elif labor and lb_prob is not None:
            row = lb_prob["rows"][n if len(lb_prob["rows"]) > 1 else 0]
            _lib.check(_lib.lib.bliss_wlabor_layer(C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"],
                                                   int(fanout), 0, draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                   int(bool(layer_dependency)), lb_prob["mode"], row.data_ptr(), lb_prob["eta_f"],
                                                   lb_prob["ome_f"], C.byref(c_ws), C.byref(c_out), p_out.data_ptr(),
                                                   self._wlabor_scratch(cap["S"], c_out.cap_b).data_ptr(), st), "bliss_wlabor_layer")
        elif nb_prob is not None:
            row = nb_prob["rows"][n if len(nb_prob["rows"]) > 1 else 0]
            _lib.check(_lib.lib.bliss_wneighbor_layer(C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"],
                                                      int(fanout), 0, draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                      nb_prob["mode"], row.data_ptr(), nb_prob["eta_f"], nb_prob["ome_f"], 0,
                                                      C.byref(c_ws), C.byref(c_out), self._wneighbor_scratch().data_ptr(), st),
                       "bliss_wneighbor_layer")
        elif labor and (labor_iterations > 0 or self.labor_is):
            _lib.check(_lib.lib.bliss_labor_is_layer(C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"],
                                                     int(fanout), 0, draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                     int(bool(layer_dependency)), int(labor_iterations), C.byref(c_ws), C.byref(c_out),
                                                     self._labor_is_scratch(cap["S"], c_out.cap_b).data_ptr(), st),
                       "bliss_labor_is_layer")
        elif labor:
            _lib.check(_lib.lib.bliss_labor_layer(C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"], int(fanout),
                                                  0, draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                  int(bool(layer_dependency)), C.byref(c_ws), C.byref(c_out),
                                                  self._labor_scratch(cap["S"]).data_ptr(), st), "bliss_labor_layer")
        else:
            if self._nb_scr is None:
                nbytes = int(_lib.lib.bliss_neighbor_scratch_bytes(self.V, 1))
                self._nb_scr = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.g.device)
            _lib.check(_lib.lib.bliss_neighbor_layer(C.byref(self.c_graph), cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cap["S"], int(fanout),
                                                     0, draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last), C.byref(c_ws),
                                                     C.byref(c_out), self._nb_scr.data_ptr(), st), "bliss_neighbor_layer")
        b_src, t_indptr, t_edge = lay[1], lay[10], lay[11]
        if t_indptr is None:
            return                                                     # (Block.transposed builds it on demand)
        ck, cb = cap["K"], cap["B"]
        if ws.tr_temp is None or ws.tr_temp[0] != (cb, ck):
            nbytes = int(_lib.lib.bliss_block_transpose_temp_bytes(cb, ck)) if cb else 0
            if nbytes < 0:
                raise RuntimeError("bliss_block_transpose_temp_bytes failed")
            ws.tr_temp = ((cb, ck), nbytes, torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.g.device))
        _, nbytes, temp = ws.tr_temp
        _lib.check(_lib.lib.bliss_block_transpose(b_src.data_ptr(), cnt_ptr + 16, cb, cb, ck, t_indptr.data_ptr(), t_edge.data_ptr(),
                                                  temp.data_ptr(), nbytes, st), "bliss_block_transpose")

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
        lay = (b_indptr, b_src, b_dst, b_pos, b_eid, b_w, b_q, kept_nid, node_prob, counts[10 * n:10 * n + 10], t_indptr, t_edge)
        return c_ws, c_out, lay, cnt_ptr, kept_nid

    # ------------------------------------------------------------------ static-shape (graph-capturable) variant
    def set_static_caps(self, S0, fanouts, max_sizes, k_margin=1.5, b_margin=3.0):
        """Fix the capacities from sizes observed in exact mode (``max_sizes[n] = dict(K=, B=)`` in sampling
        order).  Static shapes mean no host round trip inside a step and a step that can be captured in a HIP graph;
        the price is that a step whose true sizes exceed these capacities is detected only afterwards."""
        caps, s = [], int(S0)
        for n, f in enumerate(fanouts):
            k = min(self.V, int(k_margin * max_sizes[n]["K"]) + 256)
            if self.exact_k:                # (device-drawn multinomial layer: the exact bound, such a step cannot overflow K)
                k = min(self.V, int(f) + s)
            b = int(min(self.Eg, int(b_margin * max_sizes[n]["B"]) + 4096))
            if self.exact_b and int(f) >= 0:    # (neighbor layer: the exact bound, such a step cannot overflow B)
                b = int(min(2 ** 31 - 1, s * int(f))) if self.nb_replace else int(min(self.Eg, s * int(f)))
            # E only sizes launch grids (every kernel strides over the true count): a tight bound lets the hardware balance
            # the workgroups instead of a capped grid looping unevenly
            e = int(min(self.Eg, int(1.5 * max_sizes[n].get("E", self.Eg)) + 65536))
            # X: how many block edges a multi-GPU step EXCHANGES per block (update lists are sent capacity-sized; B's margin
            # is for memory that costs nothing, X's for bytes that cross xGMI every step); a longer list is flagged
            x = int(min(b, int(1.5 * max_sizes[n]["B"]) + 2048))
            caps.append(dict(S=s, C=self.V, K=k, B=b, E=e, X=x))
            s = k
        self.caps, self.ws = caps, None
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
                       last_block=True, ready_flag=0, draw_state=None, neighbor=False, labor=False, layer_dependency=False,
                       labor_iterations=0, nb_prob=None, lb_prob=None, n_live_dev=None, poisson=False, replace=False,
                       nb_replace=False):
        """Enqueue one sample_blocks on the current stream with capacity-padded outputs and NO sync.  Returns the
        blocks (sampling order); sizes, errors and the generator state are read back by finish().

        ``slot``: which persistent set of output buffers to fill.  ``chain_rng``: continue from the generator state the
        previous enqueue left on the device instead of the host-staged one (several batches sampled per host round trip).
        ``part``: None = the whole call.  "main" = everything except the blocks of all but the last-sampled layer, and layer
        n raises ``flags[n]`` when it starts; "early_blocks" = only those blocks, each behind a bliss_flag_wait on
        ``flags[n + 1]`` -- to be enqueued on ANOTHER stream, with ``scratch_sets`` >= the number of layers (block n then shares
        no scratch with any later layer) and external_rng.  The caller orders the next "main" after both parts.
        ``last_block=False`` with "main": the last-sampled layer's block is left out as well and ``flags[L]`` is raised at the end
        (its draw is done); part "last_block" = only that block, behind a bliss_flag_wait on ``flags[L]``; ``ready_flag``
        (address of a device flag) is raised as soon as the block's forward arrays are final, before its by-source index.
        ``draw_state`` (a DrawState): the layers draw with the device-side multinomial draw instead of the Poisson chain
        (whole calls only; no generator is involved); with ``poisson``: the Poisson chain itself with the keyed draw of
        bliss_poisson_select_keyed (whole calls only, no generator, no staging; ``layer_dependency``: one
        variate per node for all layers).  ``neighbor``: the layers are neighbor layers (csrc/neighbor.hip; needs
        ``draw_state``, whole calls only; ``w_rows`` / ``mode`` / ``eta`` / ``eps`` are ignored).  ``labor``: the layers are LABOR-0
        layers (csrc/labor.hip; the same conditions), with one variate per vertex for all layers when ``layer_dependency``; ``labor_iterations`` > 0:
        LABOR-i layers (csrc/labor_is.hip).  ``nb_prob`` (with ``neighbor``): the weighted draw of csrc/neighbor_w.hip, from
        ``neighbor_prob(...)``.  ``lb_prob`` (with ``labor``, ``labor_iterations`` = 0): LABOR layers with edge probabilities
        (csrc/labor_w.hip), from the same record; the blocks then carry ``_p``, the inclusion probabilities.
        ``n_live_dev`` (an int32 word on the device): ``seeds`` is a buffer of CAPACITY length -- the
        capacity the static shapes were fixed for -- of which only the first ``n_live_dev[0]`` slots are this batch's seeds.
        The first-sampled layer is then launched like every later one, with its seed count read on the device, so a captured
        call serves every batch size up to the capacity; the output block's counts record holds the live S.  Slots past the
        live count are read for no result (they hold valid node ids: zero, or an earlier batch's).  Whole calls only.
        ``replace`` (with ``draw_state``, the multinomial layers) / ``nb_replace`` (with ``neighbor``): the draws WITH replacement of
        csrc/replace_draw.hip in place of bliss_multinomial_draw / bliss_neighbor_layer."""
        if replace and (draw_state is None or poisson or neighbor or labor):
            raise ValueError("replace=True selects the multinomial layers' keyed draw with replacement: it needs a draw_state")
        if nb_replace and not neighbor:
            raise ValueError("nb_replace belongs to the neighbor layers")
        if neighbor and bool(nb_replace) != self.nb_replace:
            raise ValueError("the capacities of this engine were fixed %s replacement (LayerEngine.nb_replace)"
                             % ("with" if self.nb_replace else "without"))
        if n_live_dev is not None:
            if part is not None or external_rng or chain_rng:
                raise NotImplementedError("a live seed count has no split / external-generator enqueue (the pipelined two-stream "
                                          "loop is out of scope)")
            if not (torch.is_tensor(n_live_dev) and n_live_dev.dtype == torch.int32 and n_live_dev.numel() == 1
                    and n_live_dev.device == self.g.device):
                raise ValueError("n_live_dev: one int32 word on the graph's device")
            if self.caps is None or int(seeds.numel()) != self.caps[0]["S"] or seeds.dtype != torch.int32 or not seeds.is_contiguous():
                raise ValueError("a live seed count needs a contiguous int32 seed buffer of exactly the static seed capacity (%s), "
                                 "got %d slots" % (None if self.caps is None else self.caps[0]["S"], int(seeds.numel())))
        if nb_prob is not None and not neighbor:
            raise ValueError("nb_prob belongs to the neighbor layers")
        if lb_prob is not None and not labor:
            raise ValueError("lb_prob belongs to the LABOR layers")
        if labor and (neighbor or draw_state is None or part is not None or external_rng or chain_rng):
            raise NotImplementedError("the LABOR sampler needs a draw_state and has no split / external-generator enqueue "
                                      "(the pipelined two-stream loop is out of scope)")
        if neighbor and (draw_state is None or part is not None or external_rng or chain_rng):
            raise NotImplementedError("the device-side neighbor sampler needs a draw_state and has no split / external-generator "
                                      "enqueue (the pipelined two-stream loop is out of scope)")
        if poisson and (neighbor or labor or draw_state is None):
            raise ValueError("poisson=True selects the keyed Poisson draw of the layer-wise samplers: it needs a draw_state")
        if draw_state is not None and (part is not None or external_rng or chain_rng):
            raise NotImplementedError("the device-side draws (multinomial, keyed Poisson) have no split / external-generator "
                                      "enqueue (the pipelined two-stream loop is out of scope)")
        if part is not None and (self.scratch_sets < len(fanouts) or not external_rng):
            raise ValueError("split enqueue needs one scratch set per layer and an external generator")
        L = len(fanouts)
        out = self._enqueue(w_rows, seeds, fanouts, mode, eta, eps, None, True, slot=slot, chain_rng=chain_rng,
                            external_rng=external_rng, part=part, last_block=last_block, ready_flag=ready_flag, draw_state=draw_state,
                            neighbor=neighbor, labor=labor, layer_dependency=layer_dependency, labor_iterations=labor_iterations,
                            nb_prob=nb_prob, lb_prob=lb_prob, n_live_dev=n_live_dev, poisson=poisson, replace=replace,
                            nb_replace=nb_replace)
        self._static_draw[slot] = draw_state is not None
        counts_dev, layers = out
        if slot not in self._slot_counts_host:
            self._slot_counts_host[slot] = torch.empty(L * 10, dtype=torch.int32).pin_memory()
        if not external_rng:                     # (external: static_rng_end copies both, off the consumer's critical path)
            self._slot_counts_host[slot].copy_(counts_dev, non_blocking=True)
            if draw_state is None:
                self.mt_back.copy_(self.mt_dev, non_blocking=True)
        blocks = []
        for n, lay in enumerate(layers):
            b_indptr, b_src, b_dst, b_pos, b_eid, b_w, b_q, kept_nid, node_prob, cdev, t_indptr, t_edge = lay
            cap = self.caps[n]
            blk = Block(self.g, cap["K"], cap["S"], b_indptr, b_src, b_dst, b_pos, b_eid, kept_nid)
            blk._edge_weights, blk._q, blk._node_prob = b_w, b_q, node_prob
            if lb_prob is not None:
                blk._p = self._wl_out[n][:cap["B"]]
            blk._counts, blk._counts_dev = None, cdev
            blk._nnz_ptr = counts_dev.data_ptr() + 40 * n + 16
            blk._xcap = int(cap.get("X", cap["B"]))
            if t_indptr is not None:
                blk._transposed = (t_indptr, t_edge)
            blk._trace = {}
            blocks.append(blk)
        self._static[slot] = (blocks, L)    # kept: a captured graph replays this enqueue without re-running it
        return blocks

    def finish(self, slot=0, commit=True):
        """After the stream has been synchronised: true sizes, error check, generator hand-back."""
        blocks, L = self._static[slot]
        raw = self._slot_counts_host[slot].numpy().tobytes()
        cnts = [_lib.LayerCounts.from_buffer_copy(raw[40 * n: 40 * n + 40]) for n in range(L)]
        bad = 0
        for c in cnts:
            bad |= c.err
        for b, c in zip(blocks, cnts):
            b._counts = c
        if commit and not self._static_draw.get(slot):       # (the device draw consumed nothing from torch's generator)
            self._commit_rng(self._static_snapshot)
        if bad:
            raise RuntimeError(f"static-shape step exceeded its capacities or hit a kernel error 0x{bad:x} "
                               f"({_lib.err_string(bad)}); the step's results are invalid -- raise the margins")
        return cnts

    def _enqueue(self, w_rows, seeds, fanouts, mode, eta, eps, uniforms, snapshot, slot=None, chain_rng=False, external_rng=False,
                 part=None, last_block=True, ready_flag=0, draw_state=None, neighbor=False, labor=False, layer_dependency=False,
                 labor_iterations=0, nb_prob=None, lb_prob=None, n_live_dev=None, poisson=False, replace=False, nb_replace=False):
        if lb_prob is not None and (labor_iterations > 0 or self.labor_is):
            raise NotImplementedError("LABOR-i with edge probabilities is out of scope")
        dev, st = self.g.device, _stream()
        L = len(fanouts)
        if draw_state is None and snapshot is not None and not chain_rng and not external_rng:
            if snapshot is not True:
                self._stage_rng(snapshot)
            self.mt_dev.copy_(self.mt_host, non_blocking=True)
        if slot is None:
            counts = torch.empty(L * 10, dtype=torch.int32, device=dev)
        else:
            if slot not in self._slot_counts or self._slot_counts[slot].numel() != L * 10:
                self._slot_counts[slot] = torch.empty(L * 10, dtype=torch.int32, device=dev)
            counts = self._slot_counts[slot]
        use_rng = uniforms is None and draw_state is None
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
            if neighbor or labor:               # neighbor / LABOR layer: 6 / 7 launches and the by-source index, nothing else
                p_out = None
                if labor and lb_prob is not None:
                    p_out = self._wlabor_p(n, slot, cap["B"])
                    self._wl_out.append(p_out)
                self._enqueue_neighbor_layer(n, fanouts[n], cur_seeds, n_seeds, n_seeds_dev, draw_state, last, c_ws, c_out, lay,
                                             cnt_ptr, st, labor=labor, layer_dependency=layer_dependency,
                                             labor_iterations=labor_iterations, nb_prob=nb_prob if neighbor else None,
                                             lb_prob=lb_prob if labor else None, p_out=p_out, nb_replace=nb_replace and neighbor)
                layers.append(lay)
                cur_seeds, n_seeds, n_seeds_dev = kept_nid, -1, cnt_ptr + 12
                continue
            w_pos = w_rows[n]
            if part == "main":                  # layer n raises flag n when it starts (= everything before it has completed)
                c_ws.entry_flag = self.flags.data_ptr() + 4 * n
            if draw_state is not None and not poisson:   # multinomial samplers, keyed draw: 1 + 5 + 4 launches, then the block
                _lib.check(_lib.lib.bliss_frontier_prob(C.byref(self.c_graph), C.byref(self._set(n)["c_maps"]), w_pos.data_ptr(),
                                                        cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cs, mode, eta_f, ome_f,
                                                        cap.get("E", self.Eg), C.byref(c_ws), st), "bliss_frontier_prob")
                if replace:                     # the keyed categorical draw with replacement: 3 launches, the same mark format
                    if ws.rdraw_scr is None:
                        nbytes = int(_lib.lib.bliss_multinomial_draw_replace_scratch_bytes(cap["C"]))
                        ws.rdraw_scr = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
                    _lib.check(_lib.lib.bliss_multinomial_draw_replace(ws.p.data_ptr(), cnt_ptr, cap["C"], int(fanouts[n]), 0,
                                                                       draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                                       ws.rdraw_scr.data_ptr(), ws.new_id.data_ptr(), 0, st),
                               "bliss_multinomial_draw_replace")
                else:
                    _lib.check(_lib.lib.bliss_multinomial_draw(ws.cand_nid.data_ptr(), ws.p.data_ptr(), cnt_ptr, cap["C"], int(fanouts[n]), 0,
                                                               draw_state.seed, draw_state.step_dev.data_ptr(), n, int(last),
                                                               ws.draw_scr.data_ptr(), ws.keys.data_ptr(), ws.new_id.data_ptr(), st),
                               "bliss_multinomial_draw")
                _lib.check(_lib.lib.bliss_multinomial_select_marked(C.byref(c_ws), st), "bliss_multinomial_select_marked")
            elif part in (None, "main"):        # candidates, probabilities, draw: all the next layer needs (its seeds = kept_nid)
                if self.n_bins and self.fuse_scale:
                    # the Poisson scale rides in the last workgroup of the candidate numbering (one launch less per layer)
                    c_ws.fs_ticket = self.fs_ticket.data_ptr()
                    c_ws.fs_fanout, c_ws.fs_eps = int(fanouts[n]), float(eps)
                    if use_rng:
                        c_ws.fs_rng_ctl, c_ws.fs_layer_off = self.rng_ctl.data_ptr(), self.rng_ctl.data_ptr() + 4 * (8 + n)
                        c_ws.fs_is_last, c_ws.fs_rng_cap = int(n == L - 1), self.rng_cap
                _lib.check(_lib.lib.bliss_frontier_prob(C.byref(self.c_graph), C.byref(self._set(n)["c_maps"]), w_pos.data_ptr(),
                                                        cur_seeds.data_ptr(), n_seeds, n_seeds_dev, cs, mode, eta_f, ome_f,
                                                        cap.get("E", self.Eg), C.byref(c_ws), st), "bliss_frontier_prob")
                if poisson:                     # keyed Poisson draw: no generator, no uniforms buffer; the last select bumps the step
                    _lib.check(_lib.lib.bliss_poisson_select_keyed(C.byref(c_ws), int(fanouts[n]), float(eps), draw_state.seed,
                                                                   draw_state.step_dev.data_ptr(), 0 if layer_dependency else n,
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

    def _finish(self, out, cnts, keys=False):
        _, layers = out
        blocks = []
        for n, (lay, c) in enumerate(zip(layers, cnts)):
            b_indptr, b_src, b_dst, b_pos, b_eid, b_w, b_q, kept_nid, node_prob, cdev, t_indptr, t_edge = lay
            S, K, B = c.S, c.K, c.B
            blk = Block(self.g, K, S, b_indptr[:S + 1], b_src[:B], b_dst[:B], b_pos[:B], b_eid[:B], kept_nid[:K])
            blk._edge_weights, blk._q, blk._node_prob = b_w[:B], b_q[:B], node_prob[:K]
            blk._counts, blk._counts_dev = c, cdev
            if t_indptr is not None:
                blk._transposed = (t_indptr[:K + 1], t_edge[:max(B, 1)])
            ws = self.ws[n]
            blk._trace = dict(p=ws.p[:c.C], P=ws.P[:c.C], cand_nid=ws.cand_nid[:c.C], new_id=ws.new_id[:c.C])
            if keys:
                blk._trace["keys"] = ws.keys[:c.C]
            blocks.append(blk)
        return blocks
