"""A lean training loop that reproduces the reference's call sites around the hot path.

pytorch_lightning / dgl.dataloading.DataLoader are not available on this platform, so this module
replays, in order, exactly what they do to the sampler and the model each step
(train_lightning.py:100-168 training_step, :205-216 optimiser, :396-408 loader, :463-471 callback):

    seeds  = next batch of train ids (shuffled per epoch, drop_last)           DataLoader
    input_nodes, output_nodes, mfgs = sampler.sample(g, seeds)                 BlockSampler.sample
    x = mfgs[0].srcdata['features'];  y = mfgs[-1].dstdata['labels']          training_step :138-139
    loss = loss_fn(model(mfgs, x), y);  loss.backward();  optimiser.step()     :141-142 + Lightning
    sampler.exp3(mfgs, g)                                                      BatchSizeCallback :469-471
"""
import contextlib
import ctypes as C
import os
import time

import torch
import torch.nn as nn

from . import _lib


class BatchLoader:
    """dgl.dataloading.DataLoader(g, train_nid, sampler, batch_size, shuffle=True, drop_last=True)
    reduced to its id stream (train_lightning.py:396-408).  Shuffles on the ids' device with its own
    generator so that the sampler's CPU random stream is untouched."""

    def __init__(self, ids, batch_size, shuffle=True, drop_last=True, seed=2):
        self.ids, self.bs, self.shuffle, self.drop_last = ids, int(batch_size), shuffle, drop_last
        self._next_bs = None
        self.gen = torch.Generator(device=ids.device)
        self.gen.manual_seed(seed)

    def set_batch_size(self, bs):
        """``datamodule.batch_size = bs`` + ``loop.setup_data()`` (train_lightning.py:478-485): the size of the batches from the
        next ``__iter__`` on.  A pass in progress keeps its slices, and ``len`` the count of the pass last started."""
        bs = int(bs)
        if bs < 1:
            raise ValueError("batch size must be at least 1, got %d" % bs)
        self._next_bs = bs

    def __len__(self):
        n = self.ids.numel()
        return n // self.bs if self.drop_last else (n + self.bs - 1) // self.bs

    def __iter__(self):
        if self._next_bs is not None:
            self.bs, self._next_bs = self._next_bs, None
        return self._batches(self.bs, len(self))

    def _batches(self, bs, count):
        ids = self.ids
        if self.shuffle:
            ids = ids[torch.randperm(ids.numel(), generator=self.gen, device=ids.device)]
        for i in range(count):
            yield ids[i * bs:(i + 1) * bs]

    def forever(self):
        while True:
            yield from iter(self)


def _cap_kw():
    """Keyword arguments of every ``torch.cuda.graph`` capture here: with a process group alive, ProcessGroupNCCL's watchdog thread
    queries its events at any time, and a capture in the default "global" error mode turns such a query from ANOTHER thread into
    "operation not permitted when stream is capturing" (seen once captures became frequent: bench.py --dist shards aborted)."""
    try:
        import torch.distributed as _d
        return {"capture_error_mode": "thread_local"} if _d.is_available() and _d.is_initialized() else {}
    except Exception:                                            # noqa: BLE001
        return {}


def _inputs(model, mfgs):
    """``mfgs[0].srcdata['features']`` (train_lightning.py:138); for a model whose first layer gathers the rows as its operand
    load (model.SAGE on the MFMA path) the not-yet-gathered (table, ids) pair instead."""
    if getattr(model, "accepts_lazy_rows", False):
        return mfgs[0].srcdata.lazy("features")
    return mfgs[0].srcdata["features"]


def _ce_loss():
    if os.environ.get("BLISS_FUSED_CE", "1") == "0":
        return nn.CrossEntropyLoss()
    from .nn import CrossEntropyLoss
    return CrossEntropyLoss()


def _bce_loss():
    if os.environ.get("BLISS_FUSED_BCE", "1") == "0":
        return nn.BCEWithLogitsLoss()
    from .nn import BCEWithLogitsLoss
    return BCEWithLogitsLoss()


def _loss_backward(loss_fn, pred, labels, opt, n_rows_dev=None):
    """loss = loss_fn(pred, labels); opt.zero_grad(); loss.backward() (train_lightning.py:142 + Lightning).  The one-launch
    losses of csrc/loss.hip hand d loss / d pred over with the loss, so their route skips the loss node.  Returns the detached loss.
    ``n_rows_dev``: the live row count of a capacity-padded batch (one-launch losses only)."""
    opt.zero_grad(set_to_none=True)
    if n_rows_dev is not None:
        if not hasattr(loss_fn, "backward_from"):
            raise NotImplementedError("a batch capacity needs the one-launch losses of csrc/loss.hip (BLISS_FUSED_CE / "
                                      "BLISS_FUSED_BCE are off): torch's losses have no live row count")
        return loss_fn.backward_from(pred, labels, n_rows_dev=n_rows_dev)
    if hasattr(loss_fn, "backward_from"):
        return loss_fn.backward_from(pred, labels)
    loss = loss_fn(pred, labels)
    loss.backward()
    return loss.detach()


def _update_metric(metric, pred, mfgs, n_rows_dev=None):
    """``metric.update`` for a batch: the output block's labels as (label table, destination ids) -- the pair the one-launch
    losses take, so nothing is gathered for the metric -- or, for a block without a parent table, its own labels.
    ``n_rows_dev``: the live row count of a capacity-padded batch."""
    lab = mfgs[-1].dstdata
    parent = getattr(lab, "_parent", None)
    if parent is not None and "labels" in parent:
        from .graph import NID
        metric.update(pred, label_table=parent["labels"], label_ids=lab[NID], n_rows_dev=n_rows_dev)
    else:
        metric.update(pred, lab["labels"], n_rows_dev=n_rows_dev)


def _live_refusal(model):
    """Why ``model`` cannot run on a capacity-padded OUTPUT block, or None if it can.  Rows past the live
    count hold whatever the buffers held: only a path whose every row loop is bounded by the block's device-side counts keeps
    them out of the weight gradients (0 * NaN is NaN)."""
    from .model import GATv2, GCN, SAGE
    from .nn import TILE_KINDS, _mfma_bwd_on
    if isinstance(model, GCN):
        if model.transforms not in TILE_KINDS:
            return ('GCN runs live on its bounded kernels only: with transforms="library" its layers run over all capacity rows of '
                    'the output block; build it with GCN(..., transforms="tile") (DESIGN.md section 26)')
        return model.tile_refusal()
    if isinstance(model, GATv2):
        if model.transforms not in TILE_KINDS:
            return ('GATv2 runs live on its bounded kernels only: with transforms="library" its layers run over all capacity rows of '
                    'the output block; build it with GATv2(..., transforms="tile") (DESIGN.md section 22)')
        ps = list(model.parameters())
        if not ps or not all(p.is_cuda and p.dtype == torch.bfloat16 for p in ps):
            return 'GATv2(transforms="%s") takes bf16 parameters on the GPU' % model.transforms
        return model.tile_refusal()
    if not isinstance(model, SAGE):
        return ("%s has no live path: its layers run over all capacity rows of the output block (only SAGE on its MFMA path, "
                'GATv2(transforms="tile") and GCN(transforms="tile") bound every row loop by the block\'s device-side counts)' % type(model).__name__)
    ps = list(model.parameters())
    if ps and model._pool_tile:                  # 'pool' on the tile kernels: bounded like the MFMA path
        return model.tile_refusal(ps[0])
    if ps and model._gcn_tile:                   # 'gcn' on the tile kernels: every row and edge loop bounded
        return model.tile_refusal(ps[0])
    if not ps or not model._mfma_ok(ps[0]) or not _mfma_bwd_on():
        return ("SAGE runs live on its MFMA path only (bf16 on the GPU, ReLU, layers within the tile kernel's limits, "
                "BLISS_SAGE_MFMA / BLISS_SAGE_MFMA_BWD not 0): the library-GEMM path multiplies stale capacity rows into the "
                "weight gradients")
    return None


def _check_capacity(batch_size, batch_capacity, model, what):
    cap = int(batch_capacity)
    if cap < int(batch_size) or int(batch_size) < 1:
        raise ValueError("%s: batch_capacity (%d) must be at least the batch size (%d)" % (what, cap, int(batch_size)))
    why = _live_refusal(model)
    if why is not None:
        raise NotImplementedError("%s(batch_capacity=...): %s" % (what, why))
    return cap


def _train_metric(train_metric, multilabel):
    if not train_metric:
        return None
    from .metrics import MicroF1
    return MicroF1(multilabel)


def make_adam(model, lr, capturable=False):
    """th.optim.Adam(self.parameters(), lr) (train_lightning.py:206).  For the reference's precision (bf16 module on the GPU,
    :596-618) this is the one-launch gfx950 Adam of csrc/optim.hip; anything else gets torch's own."""
    ps = list(model.parameters())
    if ps and all(p.is_cuda and p.dtype == torch.bfloat16 and p.is_contiguous() for p in ps) and len(ps) <= _lib.ADAM_MAX_TENSORS:
        from .optim import Adam
        return Adam(ps, lr=lr)
    if capturable:
        return torch.optim.Adam(ps, lr=lr, capturable=True, fused=True)
    return torch.optim.Adam(ps, lr=lr)


class TrainStep:
    """One optimiser step of ModelLightning (train_lightning.py:50-216) with the bandit callback."""

    def __init__(self, g, sampler, model, lr=0.002, multilabel=False, bandit=True, grad_sync=None, exp3_sync=None, train_metric=False):
        self.g, self.sampler, self.model = g, sampler, model
        self.loss_fn = _bce_loss() if multilabel else _ce_loss()                        # :77-79
        # train_acc (:68-70, updated per step at :143): counts on the device, one launch per step and no read-back until
        # ``train_acc.compute()`` (metrics.MicroF1); None unless asked for
        self.train_acc = _train_metric(train_metric, multilabel)
        self.opt = make_adam(model, lr)                                                  # :206
        self.bandit = bandit and hasattr(sampler, "exp3")          # train_lightning.py:469: only for the bandit samplers
        self.grad_sync, self.exp3_sync = grad_sync, exp3_sync
        self.num_steps = 0
        self.w = 0.99                                                                    # :76
        n_layers = len(sampler.nodes_per_layer)
        self.cum_sampled_nodes = [0.0] * (n_layers + 1)
        self.cum_sampled_edges = [0.0] * n_layers
        self.last = {}

    def _ema(self, mfgs):
        self.num_steps += 1                                                              # :103
        for i, mfg in enumerate(mfgs):                                                   # :104-110
            self.cum_sampled_nodes[i] = self.cum_sampled_nodes[i] * self.w + mfg.num_src_nodes()
            self.cum_sampled_edges[i] = self.cum_sampled_edges[i] * self.w + mfg.num_edges()
        i = len(mfgs)
        self.cum_sampled_nodes[i] = self.cum_sampled_nodes[i] * self.w + mfgs[-1].num_dst_nodes()   # :127-129

    def num_sampled_edges(self, i):                                                      # :91-98
        return self.cum_sampled_edges[i] * (1 - self.w) / (1 - self.w ** self.num_steps)

    def num_sampled_nodes(self, i):                                                      # :82-89
        return self.cum_sampled_nodes[i] * (1 - self.w) / (1 - self.w ** self.num_steps)

    def __call__(self, seeds):
        input_nodes, output_nodes, mfgs = self.sampler.sample(self.g, seeds)
        self._ema(mfgs)
        batch_inputs = _inputs(self.model, mfgs)                                         # :138
        batch_labels = mfgs[-1].dstdata["labels"]                                        # :139
        batch_pred = self.model(mfgs, batch_inputs)                                      # :141
        if self.train_acc is not None:
            _update_metric(self.train_acc, batch_pred, mfgs)                             # :143
        loss = _loss_backward(self.loss_fn, batch_pred, batch_labels, self.opt)          # :142
        if self.grad_sync is not None:
            self.grad_sync(self.model)
        self.opt.step()
        if self.bandit:
            if self.exp3_sync is not None:
                self.exp3_sync(self.sampler, mfgs, self.g)
            else:
                self.sampler.exp3(mfgs, self.g)                                          # :469-471
        self.last = dict(loss=loss, mfgs=mfgs, pred=batch_pred, labels=batch_labels)
        return loss

    def last_batch_counts(self):
        """(tp, fp, fn, n) added to ``train_acc`` since the previous call (one read-back): the last batch's, when called after
        every step."""
        return self.train_acc.delta()


def _enable_gemm_tuning():
    """Let PyTorch's TunableOp measure the rocBLAS / hipBLASLt solutions of every GEMM shape it meets from now on.  Returns
    False (and leaves the library defaults in place) if this PyTorch build cannot."""
    try:
        tn = torch.cuda.tunable
        tn.enable(True)
        tn.tuning_enable(True)
        tn.set_max_tuning_duration(30)
        tn.set_max_tuning_iterations(20)
        tn.set_filename(os.path.join(os.environ.get("TMPDIR", "/tmp"), "bliss_tunableop_%d.csv" % os.getpid()))
        return True
    except Exception as e:                                   # noqa: BLE001 -- tuning is an optimisation, never a requirement
        import warnings
        warnings.warn("GEMM tuning unavailable (%r); using the library defaults" % (e,))
        return False


class GraphedTrainStep:
    """The same step as TrainStep, recorded ONCE into a HIP graph and replayed: sampler kernels, feature gather,
    SAGE forward / backward, Adam and the EXP3 update with no host work in between.

    The reference launches ~350 kernels and syncs >= 24 times per step from Python; the
    eager TrainStep above still pays ~150 launches and one mid-step sync.  Replay needs static shapes, so the
    blocks are padded to capacities learned from a few eager steps (``calibrate``); true sizes stay on the device
    and come back with the step's single end-of-step sync.  Results are bit-identical to the eager path."""

    def __init__(self, g, sampler, model, batch_size, lr=0.002, multilabel=False, distributed=False, train_metric=False, ledger=False,
                 batch_capacity=None):
        self.g, self.sampler, self.model, self.bs = g, sampler, model, int(batch_size)
        self.distributed = distributed          # replicas: gradient all-reduce + EXP3 exchange recorded in the graph too
        # batch_capacity: the seed buffer has that many slots and a device word says how many are live, so
        # ONE captured graph serves every batch size 1 .. capacity; None: the step and its graph are exactly the ones without it
        self.capacity = None
        if batch_capacity is not None:
            if distributed:
                raise NotImplementedError("batch_capacity is the single-process step's (every rank would need the same live count)")
            self.capacity = _check_capacity(batch_size, batch_capacity, model, type(self).__name__)
        # ledger: one more launch at the end of the step (csrc/ledger.hip) folds it into a device-resident record -- what ``run``
        # needs to leave the host out of the loop; False: the step and its graph are exactly the ones without it
        self._ledger_on, self._ledger, self.w = bool(ledger), None, 0.99
        self.regrows, self._want_regrow, self._ledger_regrow_at = 0, False, None
        if self._ledger_on:
            rec = _lib.ledger_new(len(sampler.nodes_per_layer))
            # (with a capacity the 32-byte batch statistics record of bliss_batch_stats follows the ledger's: one read-back has both)
            raw = bytearray(bytes(rec)) + (bytearray(C.sizeof(_lib.BatchStats)) if self.capacity is not None else bytearray())
            self._ledger = torch.frombuffer(raw, dtype=torch.int64).to(g.device)
        self.loss_fn = _bce_loss() if multilabel else _ce_loss()
        # train_acc: one more launch inside the captured graph (metrics.MicroF1: counts stay on the device); None unless asked
        # for, and the graph is then exactly the one without it
        self.train_acc = _train_metric(train_metric, multilabel)
        # ONE launch for all parameter tensors (csrc/optim.hip; torch's foreach path is ~40 launches of >= 5 us inside a graph,
        # its fused multi-tensor kernel ~50 us)
        self.opt = make_adam(model, lr, capturable=True)
        self._cap_s = self.bs if self.capacity is None else self.capacity        # slots of the seed buffer = the static seed capacity
        self.seeds = torch.zeros(self._cap_s, dtype=torch.int32, device=g.device)
        self.n_live, self._n_enqueued = None, None
        if self.capacity is not None:
            self.n_live = torch.full((1,), self.bs, dtype=torch.int32, device=g.device)
            self._n_enqueued = self.bs
        self.graph = None
        self.num_steps = 0
        self.last_counts = None
        self.loss = None

    def _load_batch(self, seeds):
        """Enqueue the batch: the seed copy and, with a capacity, the live count -- the latter only when it changed.  No sync.
        Sizes outside 1 .. capacity are refused here, on the host, before anything is enqueued."""
        if self.capacity is None:
            self.seeds.copy_(seeds)
            return
        n = int(seeds.numel())
        if not 1 <= n <= self.capacity:
            raise ValueError("a batch of %d seeds does not fit this step: 1 .. %d (batch_capacity)" % (n, self.capacity))
        self.seeds[:n].copy_(seeds)
        if n != self._n_enqueued:
            self.n_live.fill_(n)
            self._n_enqueued = n

    def calibrate(self, loader, steps=8, k_margin=1.5, b_margin=3.0):
        """Run eager sampling to learn per-layer sizes, then fix the static capacities.  With a batch capacity ``loader`` yields
        batches of ``batch_capacity`` seeds: the capacities are those of the largest batch the step serves."""
        L = len(self.sampler.nodes_per_layer)
        mx = [dict(K=0, B=0, E=0) for _ in range(L)]
        for _ in range(steps):
            seeds = next(loader)
            if self.capacity is not None and int(seeds.numel()) != self.capacity:
                raise ValueError("calibrate: with batch_capacity=%d the loader must yield batches of that many seeds, got %d"
                                 % (self.capacity, int(seeds.numel())))
            _, _, blocks = self.sampler.sample_blocks(self.g, seeds)
            for n, b in enumerate(reversed(blocks)):                      # sampling order
                mx[n]["K"] = max(mx[n]["K"], b.num_src_nodes())
                mx[n]["B"] = max(mx[n]["B"], b.num_edges())
                mx[n]["E"] = max(mx[n]["E"], b._counts.E)
        if self.distributed:                       # the exchanged lists are capacity-sized: every rank needs the same capacities
            import torch.distributed as dist
            t = torch.tensor([[m["K"], m["B"], m["E"]] for m in mx], dtype=torch.int64, device=self.g.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            mx = [dict(K=int(k), B=int(b), E=int(e)) for k, b, e in t.tolist()]
        fan = [self.sampler.nodes_per_layer[b] for b in reversed(range(L))]
        self._margins, self._hw = (k_margin, b_margin), [dict(m) for m in mx]
        self.sampler._engine.set_static_caps(self._cap_s, fan, mx, k_margin, b_margin)

    def _body(self):
        live = {} if self.capacity is None else dict(n_live_dev=self.n_live)
        input_nodes, output_nodes, mfgs = self.sampler.sample_blocks_static(self.g, self.seeds, **live)
        x = _inputs(self.model, mfgs)
        y = mfgs[-1].dstdata["labels"]
        pred = self.model(mfgs, x)
        if self.train_acc is not None:
            _update_metric(self.train_acc, pred, mfgs, self.n_live)    # train_lightning.py:143
        loss = _loss_backward(self.loss_fn, pred, y, self.opt, self.n_live)
        bandit = hasattr(self.sampler, "exp3")                     # train_lightning.py:469: only for the bandit samplers
        if self.distributed:
            from . import dist as bdist
            bdist.allreduce_gradients(self.model)
            self.opt.step()
            if bandit:
                bdist.exp3_all_ranks_static(self.sampler, mfgs, self.g)
        else:
            self.opt.step()
            if bandit:
                self.sampler.exp3(mfgs, self.g)
        # detach: a live autograd graph would pin the warm-up stream's AccumulateGrad nodes into the capture
        loss = loss.detach()
        if self._ledger_on:
            self._ledger_step(loss)
        return loss

    def _finish(self):
        torch.cuda.current_stream().synchronize()
        self.last_counts = self.sampler.finish_static()
        self.num_steps += 1

    def capture(self, loader, warmup=3, tune_gemm=False):
        """Eager static-shape warm-up steps on a side stream (allocator + autograd warm), then capture.

        ``tune_gemm``: let PyTorch's TunableOp pick the rocBLAS / hipBLASLt solution for every dense transform during
        the warm-up (the shapes are static, so each is tuned once); the tall-skinny weight-gradient GEMMs otherwise get
        a default tile that fills only a fraction of the 256 CUs."""
        eng = self.sampler._engine
        tune_gemm = tune_gemm and _enable_gemm_tuning()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._load_batch(next(loader))
                eng.stage_rng_from_torch()
                self.loss = self._body()
                self._finish()
        torch.cuda.current_stream().wait_stream(side)
        if tune_gemm:
            torch.cuda.tunable.tuning_enable(False)        # keep using the tuned solutions, stop measuring
        self._capture_graph(loader)

    def _capture_graph(self, loader):
        """Record the step on the next batch of ``loader`` and replay it once: that batch is a real step."""
        self.loss = None
        import gc
        gc.collect()
        torch.cuda.synchronize()
        self._load_batch(next(loader))
        self.sampler._engine.stage_rng_from_torch()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, **_cap_kw()):
            self.loss = self._body()
        # the capture itself executed nothing: replay once so that this batch is a real step
        self.graph.replay()
        self._finish()

    def __call__(self, seeds):
        self._load_batch(seeds)
        self.sampler._engine.stage_rng_from_torch()
        self.graph.replay()
        self._finish()
        return self.loss

    def eager_step(self, seeds):
        """The same static-shape step launched kernel by kernel (used to time individual kernels)."""
        self._load_batch(seeds)
        self.sampler._engine.stage_rng_from_torch()
        loss = self._body()
        self._finish()
        return loss

    # -- the step ledger (ledger=True): epoch statistics on the device, a loop without the host ---------------------------
    # Capacities come from a few steps taken while a bandit sampler's weights are uniform; the kept sets drift as they move.  A
    # step over a capacity is clamped and flagged only afterwards (its update is invalid), so the ledger raises ``near`` once a
    # size passes ``regrow_at`` of its capacity and ``run`` acts BEFORE the overflow: it finishes what is enqueued, re-fixes the
    # capacities from the high-water marks, re-captures and carries on.
    regrow_at = 0.85
    capture_warmup = 3                                   # warm-up steps of the capture ``run`` makes when there is no graph yet

    def _n_layers(self):
        return len(self.sampler.nodes_per_layer)

    def _ledger_caps(self):
        """{cap_K, cap_B, cap_E} per layer (sampling order) for the ledger's early warning.  A dimension whose capacity is an
        exact bound (the engine's ``exact_k`` / ``exact_b``) cannot overflow: it is passed as INT32_MAX and never raises ``near``."""
        eng, L, big = self.sampler._engine, self._n_layers(), 2 ** 31 - 1
        fan = [self.sampler.nodes_per_layer[b] for b in reversed(range(L))]
        arr = (C.c_int32 * (3 * L))()
        for n, c in enumerate(eng.caps):
            arr[3 * n] = big if eng.exact_k else c["K"]
            arr[3 * n + 1] = big if (eng.exact_b and int(fan[n]) >= 0) else c["B"]
            arr[3 * n + 2] = c["E"]
        return arr

    def _ledger_step(self, loss):
        if loss.numel() != 1 or loss.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("the step ledger takes a bf16 or fp32 scalar loss, not %s %s" % (loss.dtype, tuple(loss.shape)))
        code = _lib.LEDGER_LOSS_BF16 if loss.dtype == torch.bfloat16 else _lib.LEDGER_LOSS_F32
        self._ledger_regrow_at = float(self.regrow_at)             # (a launch argument: fixed in a captured graph)
        _lib.check(_lib.lib.bliss_step_ledger(_lib.LEDGER_STEP, loss.data_ptr(), code, self.sampler._engine._slot_counts[0].data_ptr(),
                                              self._n_layers(), self._ledger_caps(), self.w, self._ledger_regrow_at,
                                              self._ledger.data_ptr(), torch.cuda.current_stream().cuda_stream), "bliss_step_ledger")
        if self.capacity is not None:              # the input layer (the LAST-sampled one) into the running mean / variance
            _lib.check(_lib.lib.bliss_batch_stats(_lib.BATCH_STATS_PUSH, self.sampler._engine._slot_counts[0].data_ptr(),
                                                  self._n_layers() - 1, self._stats_ptr(), torch.cuda.current_stream().cuda_stream),
                       "bliss_batch_stats")

    def _stats_ptr(self):
        return self._ledger.data_ptr() + int(_lib.lib.bliss_step_ledger_bytes(self._n_layers()))

    def batch_stats(self, rec=None):
        """The running statistics of the input layer's size, ``dict(n=, m=, s=)`` -- what ``fit.BatchSizeController.load`` takes
        (``rec``: a ledger record read already; else one read-back behind everything enqueued)."""
        if not self._ledger_on or self.capacity is None:
            raise RuntimeError("this step keeps no batch statistics (ledger=True and a batch_capacity)")
        return dict((rec if rec is not None else self.ledger())["batch_stats"])

    def clear_batch_stats(self):
        """Enqueue the clear of the batch statistics (after a change of the batch size: train_lightning.py:486)."""
        if not self._ledger_on or self.capacity is None:
            raise RuntimeError("this step keeps no batch statistics (ledger=True and a batch_capacity)")
        _lib.check(_lib.lib.bliss_batch_stats(_lib.BATCH_STATS_CLEAR, None, 0, self._stats_ptr(), torch.cuda.current_stream().cuda_stream),
                   "bliss_batch_stats")

    def _ledger_mode(self, mode):
        _lib.check(_lib.lib.bliss_step_ledger(mode, None, 0, None, self._n_layers(), None, 0.0, 0.0, self._ledger.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "bliss_step_ledger")

    def _parse(self, buf):
        """A host copy of the record (an int64 tensor) as a dict."""
        raw = buf.numpy().tobytes()
        out = _lib.ledger_dict(_lib.ledger_struct(self._n_layers()).from_buffer_copy(raw))
        if self.capacity is not None:
            st = _lib.BatchStats.from_buffer_copy(raw[int(_lib.lib.bliss_step_ledger_bytes(self._n_layers())):])
            out["batch_stats"] = dict(n=int(st.n), m=float(st.m), s=float(st.s))
        return out

    def ledger(self):
        """The record as a dict, behind everything enqueued on the current stream (one read-back)."""
        if not self._ledger_on:
            raise RuntimeError("this step keeps no ledger (ledger=True)")
        return self._parse(self._ledger.cpu())

    def reset_epoch(self):
        """Enqueue the epoch reset: steps_epoch, loss_sum and nonfinite start again, everything else carries on."""
        self._ledger_mode(_lib.LEDGER_RESET_EPOCH)

    def num_sampled_edges(self, i, rec=None):
        """TrainStep.num_sampled_edges (train_lightning.py:91-98) from the ledger (``rec``: a record read already)."""
        rec = rec if rec is not None else self.ledger()
        return rec["cum_edges"][self._n_layers() - 1 - i] * (1 - self.w) / (1 - self.w ** rec["steps_total"])

    def num_sampled_nodes(self, i, rec=None):
        """TrainStep.num_sampled_nodes (:82-89) from the ledger; ``i == n_layers``: the output nodes."""
        rec = rec if rec is not None else self.ledger()
        L = self._n_layers()
        cum = rec["cum_out"] if i == L else rec["cum_nodes"][L - 1 - i]
        return cum * (1 - self.w) / (1 - self.w ** rec["steps_total"])

    def regrow(self):
        """Have the next ``run`` re-fix the capacities from the ledger's high-water marks and re-capture before it goes on."""
        self._want_regrow = True

    def _ledger_error(self, rec, where=""):
        bad = rec["err"]
        return RuntimeError(f"static-shape step exceeded its capacities or hit a kernel error 0x{bad:x} ({_lib.err_string(bad)}) "
                            f"at step {rec['first_bad_step']} of the ledger's count{where}; the results are invalid from that step "
                            f"on -- raise the margins or lower regrow_at")

    def _regrow_now(self, loader, refix=True):
        """Finish what is enqueued, enlarge the capacities to the high-water marks (x the calibration margins), re-capture.  The
        capture replays once: one real step on the next batch of ``loader``.  ``refix=False``: only the re-capture (a launch
        argument of the recorded ledger launch changed, ``regrow_at``)."""
        import gc
        eng, L = self.sampler._engine, self._n_layers()
        torch.cuda.current_stream().synchronize()
        rec = self.ledger()
        if rec["err"]:
            raise self._ledger_error(rec)
        self.graph, self.loss = None, None                 # quiesced above: drop the graph recorded for the old shapes
        gc.collect()
        torch.cuda.synchronize()
        if refix:
            mx = [dict(K=max(h.get("K", 0), rec["hw_K"][n]), B=max(h.get("B", 0), rec["hw_B"][n]), E=max(h.get("E", 0), rec["hw_E"][n]))
                  for n, h in enumerate(self._hw)]
            fan = [self.sampler.nodes_per_layer[b] for b in reversed(range(L))]
            eng.set_static_caps(self._cap_s, fan, mx, *self._margins)
            self._hw = mx
            self._ledger_mode(_lib.LEDGER_REARM)
            self._want_regrow = False
            self.regrows += 1
        self._capture_graph(loader)

    def _check_errors_once(self):
        """The error words nothing reads per step (one small read-back each, once per ``run``)."""
        if hasattr(self.sampler, "check_errors"):
            self.sampler.check_errors()
        if hasattr(self.loss_fn, "check_errors"):
            self.loss_fn.check_errors()                  # a label out of range trains silently otherwise
        for m in self.model.modules():
            if m is not self.model and hasattr(m, "check_errors"):
                m.check_errors()                         # (GATv2Conv's fused kernels)

    def run(self, loader, n_steps, poll=16, ring=8):
        """``n_steps`` train steps on the next batches of ``loader`` (an iterator); returns nothing per step: the ledger has the
        loss sum and the size averages, and ``sizes()`` / ``last_counts`` / the blocks' ``_counts`` describe the last step.

        A sampler that draws on the device (``draw == "device"``) runs FREE: per step the host enqueues the seed copy and the
        graph replay, nothing else.  Every ``poll`` steps it enqueues a non-blocking copy of the ledger into a ring of ``ring``
        pinned buffers, each with an event, after looking at the copies that have landed (never the one just enqueued; a buffer
        about to be reused is waited for, so the host stays at most ``ring`` polls ahead).  The stream is synchronised once, at
        the end.  The Poisson samplers draw from torch's CPU generator, which the host stages per step and takes back after it:
        they keep the per-step protocol (stage, replay, one sync, ``finish_static``) and use the ledger for everything else
        -- unless they too draw on the device (``draw="device"``, the keyed Poisson draw of DESIGN.md section 21).

        A record with an error word stops the enqueueing: the device finishes and RuntimeError names ``first_bad_step``.  A
        record with ``near`` set (or ``regrow()``) makes the loop finish what is enqueued, re-fix the capacities, re-capture
        (that replay is one of the ``n_steps``) and carry on: batches, their order, the draw step, torch's generator and the
        number of optimiser steps are those of the plain loop.  Without a graph yet, the first ``capture_warmup`` + 1 steps
        are the capture's (fewer steps than that run kernel by kernel)."""
        if not self._ledger_on:
            raise RuntimeError("run() needs the step ledger: GraphedTrainStep(..., ledger=True)")
        if self.distributed:
            raise NotImplementedError("run() is the single-process loop (every rank would have to take the same regrow decision)")
        if getattr(self, "_hw", None) is None:
            raise RuntimeError("calibrate() first: run() needs the static capacities")
        # (a generation-2 garbage collection in the middle of the loop can take longer than the host's lead: not during the loop)
        import gc
        was_enabled = gc.isenabled()
        if was_enabled:
            gc.disable()
        try:
            self._run(loader, int(n_steps), max(int(poll), 1), max(int(ring), 1))
        finally:
            if was_enabled:
                gc.enable()

    def _run(self, loader, n_steps, poll, ring):
        eng = self.sampler._engine
        free = getattr(self.sampler, "draw", "host") == "device"
        done = 0
        if self.graph is None and n_steps > 0:
            if n_steps < self.capture_warmup + 1:
                for _ in range(n_steps):
                    self.loss = self.eager_step(next(loader))
                done = n_steps
            else:
                self.capture(loader, warmup=self.capture_warmup)
                done = self.capture_warmup + 1
        if getattr(self, "_ring", None) is None or len(self._ring) != ring:
            self._ring = [torch.empty(self._ledger.numel(), dtype=torch.int64).pin_memory() for _ in range(ring)]
            self._ring_ev = [torch.cuda.Event() for _ in range(ring)]
        pending, polls, bad = [], 0, None                # ring slots in flight, oldest first
        while done < n_steps:
            if self._want_regrow or self._ledger_regrow_at != float(self.regrow_at):
                pending.clear()                          # (copies from before the regrow carry the old warning)
                self._regrow_now(loader, refix=self._want_regrow)
                done += 1
                continue
            self._load_batch(next(loader))
            if free:
                self.graph.replay()
                self.num_steps += 1
            else:
                eng.stage_rng_from_torch()
                self.graph.replay()
                self._finish()
            done += 1
            if done % poll or done >= n_steps:
                continue
            slot, rec = polls % ring, None
            while pending and (pending[0] == slot or self._ring_ev[pending[0]].query()):
                i = pending.pop(0)
                if not self._ring_ev[i].query():
                    self._ring_ev[i].synchronize()       # the ring is full: the host is `ring` polls ahead of the device
                rec = self._parse(self._ring[i])         # (err, near and the marks are cumulative: the newest record says it all)
                if rec["err"]:
                    break
            if rec is not None and rec["err"]:
                bad = rec                                # every later step builds on invalid blocks: stop enqueueing
                break
            if rec is not None and rec["near"]:
                self._want_regrow = True
                continue
            self._ring[slot].copy_(self._ledger, non_blocking=True)
            self._ring_ev[slot].record()
            pending.append(slot)
            polls += 1
        torch.cuda.current_stream().synchronize()        # let the device finish: THE sync of a free-running run
        rec = self.ledger()
        if bad is not None and not rec["err"]:
            rec = bad
        if free and done:
            try:
                self.last_counts = self.sampler.finish_static()
            except RuntimeError:
                if not rec["err"]:
                    raise
        if rec["err"]:
            raise self._ledger_error(rec, f" ({done} of this run's {n_steps} steps were enqueued)")
        if rec["near"]:
            self._want_regrow = True                     # seen too late for this run: the next one starts with the regrow
        self._check_errors_once()

    def last_batch_counts(self):
        """(tp, fp, fn, n) added to ``train_acc`` since the previous call (one read-back): the last batch's, when called after
        every step."""
        return self.train_acc.delta()

    def sizes(self):
        """Per block (input-most first): the true S, E, C, K, B of the last step."""
        return [dict(S=c.S, E=c.E, C=c.C, K=c.K, B=c.B) for c in reversed(self.last_counts)]

    def _graph_attrs(self):
        return ("graph",)

    def close(self):
        """Quiesce the device and destroy the captured graphs NOW.  A distributed run must call this before
        ``destroy_process_group()``: the graphs hold RCCL nodes, and graphs that outlive their communicator (destroyed at
        interpreter exit, after the process group) abort the process."""
        import gc
        torch.cuda.synchronize()
        for name in self._graph_attrs():
            v = getattr(self, name, None)
            if isinstance(v, list):
                setattr(self, name, [None] * len(v))
            elif v is not None:
                setattr(self, name, None)
        self.loss = None
        if hasattr(self, "losses"):
            self.losses = None
        gc.collect()
        torch.cuda.synchronize()


class PipelinedTrainStep(GraphedTrainStep):
    """Two train steps per call, software-pipelined: while the backward pass and Adam of batch ``a`` run on one stream,
    the sampler already builds the blocks of batch ``b`` on another (and vice versa); every piece is a replayed HIP graph.

        F(a) X(a) [ S(b) || B(a) ]  F(b) X(b) [ S(a') || B(b) ]          F forward+loss, X exp3 update, B backward+Adam, S sample

    The sampler is a long chain of small latency- and atomic-bound kernels that leaves most of the chip idle; the
    dense backward fills that idle capacity.  Nothing is reordered that depends on anything else: S(b) needs the EXP3
    weights after X(a) (it comes after it) and not the parameters; X reads only what the forward left on the blocks
    (embed_norm, q_ij), so running it before B changes no value -- every step computes exactly what the sequential
    loop computes, bit for bit, and torch's CPU generator is consumed in the same order (S(b) then S(a')).

    How the pieces are ordered (``use_flags``, the default): every graph launch costs ~20 us on the stream it is launched
    on, and an event between two kernels cuts a graph in two.  So the critical chain F X S of one step is ONE graph on the
    main stream, and the work beside it is handed off through device flags instead of events (bliss_flag_wait): the
    backward graph (second stream) starts with a wait for the flag the sampler's first kernel raises (= X has finished);
    the blocks of all but the last-sampled layer are a third graph on a third stream, each behind a wait for the flag the
    NEXT layer's first kernel raises (= this layer's draw has finished) -- block n shares no scratch with the later layers
    (one scratch set per layer in the engine), so the critical path loses those block passes.  Inside ONE graph parallel
    branches would share a hardware queue on ROCm 7.2, hence three graphs on three real streams.  ``capture`` checks that
    the flags arrive (streams that happen to share a hardware queue would make a waiting kernel block its producer) and
    otherwise falls back to event ordering: F+X, S and B as separate graphs (BLISS_PIPELINE_FLAGS=0 forces that).
    F.normalize's pass over the bandit rows stays inside X, in place (taken off the critical stream
    it was no faster).

    One call = two optimiser steps on two batches; the batch sampled last is trained by the next call (``drain``
    trains the final one)."""

    def __init__(self, g, sampler, model, batch_size, lr=0.002, multilabel=False, distributed=False, train_metric=False,
                 batch_capacity=None):
        if batch_capacity is not None:
            raise NotImplementedError("PipelinedTrainStep has no batch_capacity: its sampler is split over streams around a "
                                      "host-known seed count (use GraphedTrainStep)")
        if train_metric:
            raise NotImplementedError("PipelinedTrainStep keeps no train_acc (its forward pass is split over two graphs and two "
                                      "streams): use TrainStep or GraphedTrainStep with train_metric=True")
        if getattr(sampler, "draw", "host") == "device":
            raise NotImplementedError("PipelinedTrainStep splits the sampler over streams and runs its generator beside it; the "
                                      "device-side draws (multinomial, neighbor) have neither: use GraphedTrainStep with draw='device'")
        super().__init__(g, sampler, model, batch_size, lr, multilabel, distributed)
        self.seeds2 = [torch.zeros(self.bs, dtype=torch.int32, device=g.device) for _ in range(2)]
        self.mfgs = [None, None]
        # backward pass + Adam.  Measured and dropped: a high-priority stream (round 2: no different), a LOWEST-priority stream made
        # through the HIP runtime (round 3: 1490.1 vs 1490.0 steps/s) and a CU-masked stream (hipExtStreamCreateWithCUMask, so that
        # the backward pass leaves CUs to the sampler's latency-bound chain: 2.09 ms per step even with the full mask)
        self.side = torch.cuda.Stream()
        self.third = torch.cuda.Stream()         # blocks of all but the last-sampled layer (flag mode)
        self._fwd_done, self._bwd_done, self._blk_done = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        self._seed_ev = torch.cuda.Event()
        self.use_flags = os.environ.get("BLISS_PIPELINE_FLAGS", "1") != "0"
        self.losses = None
        self.last_counts2 = None
        self._flag_boundary = os.environ.get("BLISS_FLAG_BOUNDARY", "1") != "0"
        # The input layer's block (the LAST one the sampler builds: ~90 us at the end of its chain) built on the third stream
        # beside the next step's first transform, which needs the kept-node list only; the first aggregation waits for a
        # flag (nn._wait_block).  SAGE only: its first reader of the block's arrays is that aggregation.
        self._defer_block0 = False
        self.g_blk0 = [None, None]
        self._blk0_done = torch.cuda.Event()

    def _sample(self, slot, chain, external_rng=False, part=None, last_block=True, ready_flag=0):
        return self.sampler.sample_blocks_static(self.g, self.seeds2[slot], slot=slot, chain_rng=chain, external_rng=external_rng,
                                                 part=part, last_block=last_block, ready_flag=ready_flag)[2]

    def _split_forward(self):
        # BLISS_SPLIT_FORWARD=0 keeps the whole forward pass ahead of the bandit update (the round-1 order)
        return (hasattr(self.model, "forward_hidden") and len(getattr(self.model, "layers", ())) > 1 and hasattr(self.sampler, "exp3")
                and os.environ.get("BLISS_SPLIT_FORWARD", "1") != "0")

    FLAG_BLOCK0, FLAG_B_DONE = 10, 11                     # engine.flags slots (0..L: the sampler's layers; 14: the probe)

    def _forward(self, mfgs):
        """The part of the step the NEXT batch's sampler waits for: the forward pass up to the output layer's input (every
        block's row norms exist from there on, train_lightning.py:232-238 reads nothing else) and the bandit update.  Returns
        what _backward needs to finish the step."""
        pending = self._forward_model(mfgs)
        if not hasattr(self.sampler, "exp3"):                      # LADIES samplers keep no bandit state
            return pending
        if self.distributed:
            from . import dist as bdist
            bdist.exp3_all_ranks_static(self.sampler, mfgs, self.g)
        else:
            self.sampler.exp3(mfgs, self.g)
        return pending

    def _forward_model(self, mfgs):
        if self._split_forward():
            pending = ("hidden", self.model.forward_hidden(mfgs, _inputs(self.model, mfgs)), mfgs)
        else:
            pred = self.model(mfgs, _inputs(self.model, mfgs))
            pending = ("pred", pred, mfgs)
        return pending

    def _backward(self, pending):
        """Output layer + loss (when _forward left them), backward, optimizer.  Returns the detached loss."""
        kind, val, mfgs = pending
        loss = None
        if kind == "hidden" and hasattr(self.model, "forward_last_parts") and hasattr(self.loss_fn, "backward_from_parts"):
            # output layer's sum and the label gather inside the loss kernel (two small launches less on the backward stream)
            lab = mfgs[-1].dstdata
            table = lab._parent["labels"] if getattr(lab, "_parent", None) is not None and "labels" in lab._parent else None
            parts = self.model.forward_last_parts(mfgs, val) if table is not None and not dict.__contains__(lab, "labels") else None
            if parts is not None:
                self.opt.zero_grad(set_to_none=True)
                loss = self.loss_fn.backward_from_parts(parts[0], parts[1], table, lab._index_fn())
        if loss is None:
            pred = self.model.forward_last(mfgs, val) if kind == "hidden" else val
            loss = _loss_backward(self.loss_fn, pred, mfgs[-1].dstdata["labels"], self.opt)
        if self.distributed:
            from . import dist as bdist
            bdist.allreduce_gradients(self.model)
        self.opt.step()
        return loss

    def _pair(self):
        # Eager version (warm-up, kernel-by-kernel timing).  The sampler stays on the origin stream (its random-number
        # generator forks from there); the model runs on the second stream, forward AND backward (autograd replays a node on
        # the stream of its forward).
        main, side = torch.cuda.current_stream(), self.side
        side.wait_stream(main)
        losses = []
        for cur, nxt, chain in ((0, 1, False), (1, 0, True)):
            with torch.cuda.stream(side):
                pending = self._forward(self.mfgs[cur])      # F + X
            main.wait_stream(side)                           # the sampler needs the EXP3 weights X just wrote
            self.mfgs[nxt] = self._sample(nxt, chain)        # S, beside ...
            with torch.cuda.stream(side):
                losses.append(self._backward(pending))       # ... B
                side.wait_stream(main)                       # the next forward needs the blocks S built
        main.wait_stream(side)
        return tuple(losses)

    def prime(self, seeds):
        """Sample the first batch (slot 0) so that the pipeline has something to train on."""
        self.seeds2[0].copy_(seeds)
        self.sampler._engine.stage_rng_from_torch()
        self.mfgs[0] = self._sample(0, False)
        torch.cuda.current_stream().synchronize()
        self.sampler.finish_static(0, commit=True)

    def _finish_pair(self, check_flags=True):
        torch.cuda.current_stream().synchronize()
        c1 = self.sampler.finish_static(1, commit=False)
        c0 = self.sampler.finish_static(0, commit=True)
        self.last_counts2 = [c1, c0]                     # the two batches sampled by this replay, in sampling order
        self.last_counts = c0
        self.num_steps += 2
        if check_flags and self.graph and self.use_flags and int(self.sampler._engine.flag_err.item()):
            raise RuntimeError("a cross-stream flag never arrived (bliss_flag_wait timed out): the pipelined results are invalid")

    def _load(self, loader):
        self.seeds2[1].copy_(next(loader))               # S(b) runs first, then S(a')
        self.seeds2[0].copy_(next(loader))
        self.sampler._engine.stage_rng_from_torch()

    def capture(self, loader, warmup=2, tune_gemm=False):
        eng = self.sampler._bind(self.g)
        L = len(self.sampler.nodes_per_layer)
        if torch.cuda.current_stream() != torch.cuda.default_stream():
            import warnings
            warnings.warn("PipelinedTrainStep: captured from a non-default stream; HIP maps streams onto a few hardware queues and the "
                          "critical chain then shares one with a side stream (measured 1.08 instead of 0.70 ms per step)")
        if self.use_flags and not self._flags_usable():       # (before the warm-up: autograd remembers the streams it ran on)
            import warnings
            warnings.warn("PipelinedTrainStep: streams do not run side by side here (a profiler serialising kernels?); "
                          "ordering the graphs with events instead of device flags")
            self.use_flags = False
        if self.use_flags:
            eng.scratch_sets = max(eng.scratch_sets, L)      # block n then shares no scratch with any later layer
        self._defer_block0 = (self.use_flags and self._flag_boundary and L > 1 and L < self.FLAG_BLOCK0 and type(self.model).__name__ == "SAGE"
                              and self._split_forward() and os.environ.get("BLISS_DEFER_BLOCK0", "1") != "0")
        tune_gemm = tune_gemm and _enable_gemm_tuning()
        warm = torch.cuda.Stream()
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            self.prime(next(loader))
            for _ in range(warmup):
                self._load(loader)
                self.losses = self._pair()
                self._finish_pair()
        torch.cuda.current_stream().wait_stream(warm)
        if tune_gemm:
            torch.cuda.tunable.tuning_enable(False)
        self.losses = None
        import gc
        gc.collect()
        torch.cuda.synchronize()
        self._capture_graphs(loader)
        if self.use_flags and int(eng.flag_err.item()):
            import warnings
            warnings.warn("PipelinedTrainStep: a cross-stream flag timed out (streams sharing a hardware queue?); "
                          "falling back to event-ordered graphs")
            eng.flag_err.zero_()
            eng.flags.zero_()
            self.use_flags = False
            self._capture_graphs(loader)

    def _probe(self, st, flag_index):
        """One wait on ``st`` enqueued FIRST, the raise on the main stream afterwards: completes without a timeout only if
        the two streams really run side by side."""
        eng = self.sampler._engine
        main = torch.cuda.current_stream()
        torch.cuda.synchronize()
        eng.flag_err.zero_()
        eng.flags.zero_()
        torch.cuda.synchronize()
        f = eng.flags.data_ptr() + 4 * flag_index
        _lib.check(_lib.lib.bliss_flag_wait(f, eng.flag_err.data_ptr(), st.cuda_stream), "bliss_flag_wait")
        _lib.check(_lib.lib.bliss_flag_raise(f, main.cuda_stream), "bliss_flag_raise")
        torch.cuda.synchronize()
        ok = int(eng.flag_err.item()) == 0
        eng.flag_err.zero_()
        eng.flags.zero_()
        torch.cuda.synchronize()
        return ok

    def _flags_usable(self, tries=4):
        """Probe with harmless kernels before relying on device flags for ordering: a flag that times out in the real loop
        would let a consumer run before its producer.  HIP multiplexes streams onto a few hardware queues (4 by default);
        a stream that shares the main stream's queue cannot wait for it, so such a stream is replaced by the next one of
        PyTorch's pool and probed again.  Under a profiler that serialises kernels (rocprofv3 --pmc) no stream passes."""
        for name in ("side", "third"):
            for _ in range(tries):
                if self._probe(getattr(self, name), 14):
                    break
                setattr(self, name, torch.cuda.Stream())
            else:
                return False
        return True

    def _capture_graphs(self, loader):
        # Several graphs, not one: a HIP graph with the sampler and the backward pass as parallel branches is executed with
        # both branches on one hardware queue (ROCm 7.2), i.e. not overlapped.  Replaying them from different real streams
        # gives the overlap (see _half).
        eng = self.sampler._engine
        L = len(self.sampler.nodes_per_layer)
        self._load(loader)
        side = self.side
        pool = torch.cuda.graph_pool_handle()
        self.graph = None
        self.g_main, self.g_fwd, self.g_bwd, self.g_smp, self.g_blk, self.g_blk0 = ([None, None] for _ in range(6))
        held, out = [None, None], [None, None]
        st_ = lambda: torch.cuda.current_stream().cuda_stream
        for cur, nxt, chain in ((0, 1, False), (1, 0, True)):
            # (the sampler is recorded without its generator: that one is launched ahead of time, see _replay / run)
            self.g_bwd[cur] = torch.cuda.CUDAGraph()
            if self.use_flags:
                self.g_main[cur] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.g_main[cur], pool=pool, stream=side, **_cap_kw()):
                    if self._flag_boundary:
                        # "the previous step's backward pass, Adam and early blocks are done", as a device flag: the graph is
                        # launched ahead and its first kernel waits ~3 us past the raise; a stream-event wait in front of the
                        # graph launch cost ~30 us from the end of B to the first kernel of F
                        _lib.check(_lib.lib.bliss_flag_wait(eng.flags.data_ptr() + 4 * self.FLAG_B_DONE, eng.flag_err.data_ptr(), st_()),
                                   "bliss_flag_wait")
                    if self._defer_block0:              # (the wait itself is recorded by the first aggregation over that block)
                        self.mfgs[cur][0]._ready = (eng.flags.data_ptr() + 4 * self.FLAG_BLOCK0, eng.flag_err.data_ptr())
                    held[cur] = self._forward(self.mfgs[cur])                                   # F + X
                    self.mfgs[cur][0]._ready = None
                    self.mfgs[nxt] = self._sample(nxt, chain, external_rng=True, part="main",   # S without the early blocks
                                                  last_block=not self._defer_block0)
                if L > 1:
                    self.g_blk[nxt] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.g_blk[nxt], **_cap_kw()):
                        self._sample(nxt, chain, external_rng=True, part="early_blocks")
                if self._defer_block0:
                    self.g_blk0[nxt] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.g_blk0[nxt], **_cap_kw()):
                        # (raises FLAG_BLOCK0 itself, before it sorts the by-source index the backward pass will read)
                        self._sample(nxt, chain, external_rng=True, part="last_block", ready_flag=eng.flags.data_ptr() + 4 * self.FLAG_BLOCK0)
                with torch.cuda.graph(self.g_bwd[cur], pool=pool, stream=side, **_cap_kw()):
                    # B may start once S has (flag 0 is raised by the sampler's first kernel: F and X have completed)
                    _lib.check(_lib.lib.bliss_flag_wait(eng.flags.data_ptr(), eng.flag_err.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream), "bliss_flag_wait")
                    out[cur] = self._backward(held[cur])
            else:
                self.g_fwd[cur], self.g_smp[nxt] = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.g_fwd[cur], pool=pool, stream=side, **_cap_kw()):
                    held[cur] = self._forward(self.mfgs[cur])
                with torch.cuda.graph(self.g_smp[nxt], **_cap_kw()):
                    self.mfgs[nxt] = self._sample(nxt, chain, external_rng=True)
                with torch.cuda.graph(self.g_bwd[cur], pool=pool, stream=side, **_cap_kw()):
                    out[cur] = self._backward(held[cur])
        self.losses = tuple(out)
        self.graph = True
        self._replay()                                   # the captures themselves executed nothing
        self._finish_pair(check_flags=False)             # (capture() looks at the flags itself)

    def _half(self, cur, nxt, on_side=None):
        """Enqueue F(cur) X(cur) [ S(nxt) || B(cur) ].  The generator of S(nxt) has been started by the caller.
        ``on_side``: extra work for the backward pass's stream, after B."""
        main, side = torch.cuda.current_stream(), self.side
        if not (self.use_flags and self._flag_boundary):
            main.wait_event(self._bwd_done)              # parameters after the previous step's Adam
        if self.use_flags:
            if self._defer_block0:
                # B(cur) reads the by-source index of its input block, sorted behind that block's ready flag in the PREVIOUS
                # half's g_blk0 (this wait must precede the record further down, which is this half's)
                side.wait_event(self._blk0_done)
            self.g_main[cur].replay()                    # F + X + S: one graph on the critical stream
            if self.g_blk[nxt] is not None:
                with torch.cuda.stream(self.third):
                    self.g_blk[nxt].replay()             # early blocks of S: each waits for the flag of the next layer
                    self._blk_done.record(self.third)
                    if self.g_blk0[nxt] is not None:
                        self.g_blk0[nxt].replay()        # the input layer's block: waits for the end of S, raises FLAG_BLOCK0
                        self._blk0_done.record(self.third)
            with torch.cuda.stream(side):
                self.g_bwd[cur].replay()                 # B: waits for the flag S raises when it starts
                if on_side is not None:
                    on_side()
                # one wait on the critical stream instead of two: "B done" below also means "all blocks of S built"
                if self.g_blk[nxt] is not None:
                    side.wait_event(self._blk_done)
                if self._flag_boundary:
                    _lib.check(_lib.lib.bliss_flag_raise(self.sampler._engine.flags.data_ptr() + 4 * self.FLAG_B_DONE, side.cuda_stream),
                               "bliss_flag_raise")
                self._bwd_done.record(side)
        else:
            self.g_fwd[cur].replay()                     # F + X
            self._fwd_done.record(main)
            with torch.cuda.stream(side):
                side.wait_event(self._fwd_done)
                self.g_bwd[cur].replay()                 # B, beside ...
                if on_side is not None:
                    on_side()
                self._bwd_done.record(side)
            self.g_smp[nxt].replay()                     # ... S (needs the EXP3 weights X just wrote: same stream)

    def _join(self):
        torch.cuda.current_stream().wait_event(self._bwd_done)     # (flag mode: implies the early blocks, see _half)
        if self._defer_block0 and self.graph:
            torch.cuda.current_stream().wait_event(self._blk0_done)

    def _prime_boundary(self):
        # the first forward pass of a run of replays waits for a backward pass nobody launched
        if self.use_flags and self._flag_boundary and self.graph:
            eng = self.sampler._engine
            _lib.check(_lib.lib.bliss_flag_raise(eng.flags.data_ptr() + 4 * self.FLAG_B_DONE, torch.cuda.current_stream().cuda_stream),
                       "bliss_flag_raise")
            if self._defer_block0:                       # (the batch in flight was sampled completely: _join / prime)
                _lib.check(_lib.lib.bliss_flag_raise(eng.flags.data_ptr() + 4 * self.FLAG_BLOCK0, torch.cuda.current_stream().cuda_stream),
                           "bliss_flag_raise")

    def _after_blocks(self):
        """The stream on which 'the sampler of the last half has finished' is to be recorded: the third one when it builds the
        last block (its counts record and error word are complete only then)."""
        return torch.cuda.stream(self.third) if (self._defer_block0 and self.graph) else contextlib.nullcontext()

    def _replay(self, first_chain=False):
        eng = self.sampler._engine
        self._prime_boundary()
        for cur, nxt, chain in ((0, 1, first_chain), (1, 0, True)):
            eng.static_rng_begin(chain)                  # the serial MT19937 chain of S starts now, beside F + X
            self._half(cur, nxt)
            if self._defer_block0:
                torch.cuda.current_stream().wait_event(self._blk0_done)   # (the counts record static_rng_end copies)
            eng.static_rng_end(nxt)
        self._join()

    def __call__(self, loader):
        """Two steps: trains the batch sampled by the previous call and the next batch of ``loader``; samples two."""
        self._load(loader)
        self._replay()
        self._finish_pair()
        return self.losses

    # -- capacities that follow the run --------------------------------------------------------------------------------
    # Static capacities come from a few steps taken while the bandit weights are uniform; as the weights move, the kept sets
    # and blocks drift.  A step that exceeds a capacity is clamped and flagged only afterwards (its update is invalid), so
    # the loop watches the sizes that come back with every pair and acts BEFORE that: once a size passes ``regrow_at`` of
    # its capacity, the next run() first trains the batch in flight, recalibrates from the high-water marks, re-captures
    # the graphs and carries on -- the batches, their order and the sampler's random stream are those of the plain loop.
    regrow_at = 0.85

    def _watch(self, sizes):
        caps = self.sampler._engine.caps
        L = len(caps)
        for sz in sizes:                                   # per batch: blocks input-most first = sampling order reversed
            for l, s_ in enumerate(sz):
                n = L - 1 - l
                hw = self._hw[n]
                for k in ("K", "B", "E"):
                    hw[k] = max(hw.get(k, 0), int(s_[k]))
                if s_["K"] > self.regrow_at * caps[n]["K"] or s_["B"] > self.regrow_at * caps[n]["B"] or \
                        (self.distributed and s_["B"] > self.regrow_at * caps[n].get("X", caps[n]["B"])):
                    self._needs_regrow = True

    def _regrow(self, loader):
        """Train the batch in flight, enlarge the capacities to the high-water marks (x the calibration margins), re-capture.
        Returns the sizes of the two batches the re-capture sampled (it replays one pair)."""
        eng = self.sampler._engine
        L = len(self.sampler.nodes_per_layer)
        self.drain()
        mx = [dict(h) for h in self._hw]
        if self.distributed:                               # every rank must end up with the same capacities
            import torch.distributed as dist
            t = torch.tensor([[m["K"], m["B"], m["E"]] for m in mx], dtype=torch.int64, device=self.g.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            mx = [dict(K=int(k), B=int(b), E=int(e)) for k, b, e in t.tolist()]
        GraphedTrainStep.close(self)                       # quiesce, drop the graphs recorded for the old shapes
        fan = [self.sampler.nodes_per_layer[b] for b in reversed(range(L))]
        eng.set_static_caps(self.bs, fan, mx, *self._margins)
        if self.use_flags:
            eng.scratch_sets = max(eng.scratch_sets, L)
        self._needs_regrow = False
        self.regrows = getattr(self, "regrows", 0) + 1
        self.prime(next(loader))
        primed = [dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in reversed(eng._static[0][0])]
        self._capture_graphs(loader)
        return [primed] + self.sizes2()                   # every batch sampled here, in sampling order

    def run(self, loader, n_pairs, ring=8, pair_events=None):
        # The host stays a few pairs ahead of the device; a generation-2 garbage collection in the middle of the loop can take
        # longer than that lead and drain the queues (one pair of > 3 ms in some 400-step windows): not during the loop.
        import gc
        was_enabled = gc.isenabled()
        if was_enabled:
            gc.disable()
        try:
            return self._run(loader, n_pairs, ring, pair_events)
        finally:
            if was_enabled:
                gc.enable()

    def _run(self, loader, n_pairs, ring=8, pair_events=None):
        """``n_pairs`` calls without a host round trip in between: the generator state is chained on the device from
        batch to batch (torch's CPU generator is brought up to date once, at the end), and sizes / error words come back
        through a small ring of pinned buffers while later pairs are already running.  Returns the block sizes of every
        batch sampled, in order.  ``pair_events``: a list that receives one timing event per pair boundary (recorded on
        the critical stream at the start of every pair and after the last one): consecutive differences are the device
        time of two train steps each."""
        eng = self.sampler._engine
        L = len(self.sampler.nodes_per_layer)
        if getattr(self, "_ring", None) is None or len(self._ring) != ring:
            self._ring = [torch.empty(2 * L * 10, dtype=torch.int32).pin_memory() for _ in range(ring)]
            self._ring_ev = [torch.cuda.Event() for _ in range(ring)]
        sizes, pending, bad = [], [], 0
        if getattr(self, "_needs_regrow", False):          # (the re-capture trains three batches itself: one drained, one pair)
            sizes += self._regrow(loader)
            self._watch(sizes)

        def collect(i):
            nonlocal bad
            self._ring_ev[i].synchronize()
            raw = self._ring[i].numpy().tobytes()
            for half in range(2):
                cs = [_lib.LayerCounts.from_buffer_copy(raw[40 * (half * L + n): 40 * (half * L + n) + 40]) for n in range(L)]
                for c in cs:
                    bad |= c.err
                sizes.append([dict(S=c.S, E=c.E, C=c.C, K=c.K, B=c.B) for c in reversed(cs)])

        eng.stage_rng_from_torch()
        # Free-running loop: nothing but graph replays and event records goes onto the main stream.  The generator hand-over
        # between two samplers (state commit, counts to the host, control block of the next generator) is one kernel on the
        # generator's stream (static_rng_chain); the seed ids of later batches are copied on the backward pass's stream.
        main = torch.cuda.current_stream()
        self._prime_boundary()
        if n_pairs:
            self.seeds2[1].copy_(next(loader))           # S(b) runs first, then S(a')
            self.seeds2[0].copy_(next(loader))
        trace = self._host_trace = [] if pair_events is not None else None   # (host clock per pair: enqueue start, time blocked)
        for k in range(n_pairs):
            t_in = time.perf_counter() if trace is not None else 0.0
            while pending and pending[0] <= k - ring:    # this pair reuses that pair's record
                collect(pending.pop(0) % ring)
            if bad:
                # an error word came back with a pair's record (capacity overrun, non-finite weight, ...): every later step
                # builds on invalid blocks / EXP3 rows, so stop enqueueing -- the error surfaces within `ring` pairs of the step
                # that raised it, not at the end of the window (round-2 advice)
                n_done = k
                break
            if pair_events is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(main)
                pair_events.append(ev)
                trace.append((t_in, time.perf_counter() - t_in))
            last = k == n_pairs - 1
            r = self._ring[k % ring]
            for cur, nxt in ((0, 1), (1, 0)):
                if k == 0 and cur == 0:
                    eng.static_rng_begin(False)          # from the host-staged state
                elif cur == 0:                           # ends S(a') of the previous pair; its sizes complete that pair's record
                    with self._after_blocks():
                        eng.static_rng_chain(0, self._ring[(k - 1) % ring][L * 10:])
                else:
                    with self._after_blocks():
                        eng.static_rng_chain(1, r[:L * 10])
                # (no wait for the hand-over on the main stream: the sampler's first random-number wait checks that the control
                # block is the new generator's -- the event round trip cost ~12 us between every two steps)
                if cur == 0 and k > 0:                   # the previous pair's record is complete once that hand-over has run
                    eng.static_rng_record(self._ring_ev[(k - 1) % ring])
                    pending.append(k - 1)
                # the sampler that read slot ``cur``'s seed ids finished before this half's forward pass: load the next batch
                # there, behind the backward pass.  The loader itself works on the main stream (a new epoch shuffles there).
                on_side = None
                if (cur == 0 and k > 0) or (cur == 1 and not last):
                    batch = next(loader)
                    self._seed_ev.record(main)
                    batch.record_stream(self.side)

                    def on_side(c=cur, b=batch):
                        self.side.wait_event(self._seed_ev)
                        self.seeds2[c].copy_(b)
                self._half(cur, nxt, on_side=on_side)
            if last:
                if self._defer_block0:
                    main.wait_event(self._blk0_done)
                eng.static_rng_end(0)
                r[L * 10:].copy_(eng._slot_counts[0], non_blocking=True)
                self._join()
                if pair_events is not None:
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record(main)
                    pair_events.append(ev)
                self._ring_ev[k % ring].record(main)
                pending.append(k)
        else:
            n_done = n_pairs
        if n_done < n_pairs:                             # stopped early: let the device finish what is enqueued, then report
            torch.cuda.synchronize()                     # (the loop object is not usable afterwards: results are invalid anyway)
            for i in pending:
                collect(i % ring)
            raise RuntimeError(f"static-shape step exceeded its capacities or hit a kernel error 0x{bad:x} ({_lib.err_string(bad)}) "
                               f"within the last {ring} pairs before pair {n_done} of {n_pairs}; results from there on are invalid")
        for i in pending:
            collect(i % ring)
        if n_pairs:
            # what finish_static(1) reads: the last pair's first sampler handed its sizes to the ring
            eng._slot_counts_host[1].copy_(self._ring[(n_pairs - 1) % ring][:L * 10])
            self._finish_pair()
        if bad:
            raise RuntimeError(f"static-shape step exceeded its capacities or hit a kernel error 0x{bad:x} "
                               f"({_lib.err_string(bad)}) before the early-warning regrow could act; results are invalid -- "
                               f"raise the margins or lower regrow_at")
        self._watch(sizes)
        if self.distributed and hasattr(self.sampler, "check_errors"):
            # the exchange truncates an update list that outgrew its capacity and only flags it on the sampler: surface
            # it with the call that produced it, not at the end of training (one tiny read-back per run(), not per step)
            self.sampler.check_errors()
        if hasattr(self.loss_fn, "check_errors"):
            self.loss_fn.check_errors()                  # a label out of range trains silently otherwise (same read-back point)
        return sizes

    def eager_pair(self, loader):
        """The same two steps launched kernel by kernel (used to time individual kernels)."""
        self._load(loader)
        self.losses = self._pair()
        self._finish_pair()
        return self.losses

    def drain(self):
        """Train on the batch that is sampled but not trained yet (end of training)."""
        main, side = torch.cuda.current_stream(), self.side
        side.wait_stream(main)
        with torch.cuda.stream(side):
            loss = self._backward(self._forward(self.mfgs[0]))
        main.wait_stream(side)
        main.synchronize()
        self.num_steps += 1
        return loss

    def _graph_attrs(self):
        return ("graph", "g_main", "g_fwd", "g_bwd", "g_smp", "g_blk", "g_blk0")

    def close(self):
        """Train the batch still in flight (``drain``), wait for every stream of the loop, then destroy the graphs."""
        if self.graph and self.mfgs[0] is not None:
            self.drain()
        for st in (self.side, self.third):
            st.synchronize()
        super().close()
        self.mfgs = [None, None]

    def sizes2(self):
        """sizes() for each of the two batches sampled by the last call."""
        return [[dict(S=c.S, E=c.E, C=c.C, K=c.K, B=c.B) for c in reversed(cs)] for cs in self.last_counts2]


@contextlib.contextmanager
def _keep_static_caps(eng):
    """Eager sampling beside captured graphs: the engine's retry loop answers a capacity overflow by growing the capacities and
    re-allocating its workspaces -- which captured graphs still point at.  Whatever the block changed of the engine's static
    capacities is put back on leaving it (the buffers were kept alive meanwhile); the blocks it sampled stay valid."""
    names = ("ws", "counts_host", "rng_cap", "rng_plan", "rng_out", "rng_raw", "rng_ctl", "n_bins")
    static = eng.caps is not None and all("E" in c for c in eng.caps)
    saved = {k: getattr(eng, k, None) for k in names}
    caps = [dict(c) for c in eng.caps] if static else None
    try:
        yield
    finally:
        if static and (eng.ws is not saved["ws"] or eng.caps != caps):
            eng.caps = caps
            for k, v in saved.items():
                setattr(eng, k, v)


@contextlib.contextmanager
def _rng_kept(sampler, g):
    """Sampler calls that must leave no trace (a calibration beside a run): torch's CPU generator and the device draw step are
    put back on leaving the block."""
    state = torch.get_rng_state()
    ds = sampler._draw_state_on(g.device) if hasattr(sampler, "_draw_state_on") else None
    step = ds.step_dev.clone() if ds is not None else None
    try:
        yield
    finally:
        torch.set_rng_state(state)
        if ds is not None:
            ds.step_dev.copy_(step)


class GraphedEvalStep:
    """validation_step over a split (train_lightning.py:179-203, :410-422) with every full batch REPLAYED from one HIP graph:
    ``sample_blocks_static`` on an output slot of its own, ``model.eval()`` forward under ``no_grad``, the loss, the micro-F1
    update (metrics.MicroF1: counts on the device) and loss * n, all into a per-batch buffer the graph zeroes itself.  The host
    adds that buffer to the split's accumulators (a device add, enqueued) only once ``finish_static`` has passed for the batch;
    metric and loss are read back once, at the end of ``run``.  What ``fit.evaluate`` does eagerly -- ~150 launches and L + 1
    syncs per batch, a ``float()`` per batch, every prediction of the split concatenated -- with the same sampler calls in the
    same order: torch's generator, the draw step and the EXP3 rows end up where the eager pass leaves them (no bandit update).

    Capacities: the sampler engine's static ones when a train step has fixed them already (they are never re-fixed here: a
    captured train graph depends on them); otherwise ``calibrate`` fixes them, from the split's own batches, the first time
    ``run`` needs them.  The ragged last batch runs eagerly through ``sampler.sample`` into the same accumulators, and so does a
    batch whose replay exceeded a capacity (``finish_static`` raised): its per-batch buffer is dropped, torch's generator and the
    draw step are put back, and the batch is sampled again by the engine's regrowing eager loop (``fallbacks`` counts these).

    ``batch_capacity``: the seed buffer has that many slots and a device word says how many are live --
    EVERY batch of 1 .. capacity seeds is then replayed from the one graph, the ragged last batch of a split included
    (``replays`` counts them), the eager path remains only as the capacity-overflow fallback, the static capacities are those
    of ``batch_capacity`` seeds (shared with a train step of the same capacity) and ``set_batch_size`` changes the batch size
    without a re-capture."""

    SLOT = 2                                   # (0 and 1 are the training loops')

    def __init__(self, g, sampler, model, batch_size, multilabel=False, loss_fn=None, batch_capacity=None):
        static = hasattr(sampler, "sample_blocks_static") and (getattr(sampler, "_poisson", False)
                                                               or getattr(sampler, "draw", "host") == "device")
        if not static:
            raise NotImplementedError("GraphedEvalStep needs a sampler with a static-shape path; %s%s has none (the Poisson samplers "
                                      "have one, the multinomial samplers and NeighborSampler with draw='device')"
                                      % (type(sampler).__name__, " with draw='host'" if hasattr(sampler, "draw") else ""))
        from .metrics import MicroF1
        self.g, self.sampler, self.model, self.bs, self.multilabel = g, sampler, model, int(batch_size), bool(multilabel)
        self.loss_fn = loss_fn if loss_fn is not None else (_bce_loss() if multilabel else _ce_loss())
        dev = g.device
        self.capacity = None if batch_capacity is None else _check_capacity(batch_size, batch_capacity, model, type(self).__name__)
        if self.capacity is not None and not hasattr(self.loss_fn, "backward_from"):
            raise NotImplementedError("a batch capacity needs the one-launch losses of csrc/loss.hip: torch's have no live row count")
        self._cap_s = self.bs if self.capacity is None else self.capacity
        self.seeds = torch.zeros(self._cap_s, dtype=torch.int32, device=dev)
        self.n_live, self._n_enqueued = None, None
        if self.capacity is not None:
            self.n_live = torch.full((1,), self.bs, dtype=torch.int32, device=dev)
            self._n_enqueued = self.bs
        self.replays = 0
        self.metric, self._batch_metric = MicroF1(multilabel), MicroF1(multilabel)
        self.metric._state_on(dev)
        self._batch_metric._state_on(dev)
        self._loss_sum = torch.zeros((), dtype=torch.float32, device=dev)          # sum over batches of loss * n, fp32
        self._batch_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.graph, self._captured_for = None, None
        self.fallbacks, self.captures = 0, 0

    # -- capacities -------------------------------------------------------------------------------------------------------
    def _engine(self):
        return self.sampler._bind(self.g)

    def has_static_caps(self):
        caps = self._engine().caps
        L = len(self.sampler.nodes_per_layer)
        if caps is None or len(caps) != L or not all("E" in c for c in caps):
            return False
        if caps[0]["S"] != self._cap_s:
            raise ValueError("the sampler's static capacities were fixed for batches of %d, not %d: a GraphedEvalStep shares them "
                             "with the train step that fixed them and needs its batch size%s"
                             % (caps[0]["S"], self._cap_s, "" if self.capacity is None else " (its batch_capacity)"))
        return True

    def set_batch_size(self, bs):
        """The batch size of the next ``run`` (``val_dataloader`` follows ``datamodule.batch_size``, train_lightning.py:410-422);
        needs a capacity, and stays within it."""
        if self.capacity is None:
            raise RuntimeError("a GraphedEvalStep without batch_capacity is captured for one batch size")
        if not 1 <= int(bs) <= self.capacity:
            raise ValueError("batch size %d outside 1 .. %d (batch_capacity)" % (int(bs), self.capacity))
        self.bs = int(bs)

    def _load_batch(self, seeds):
        """Enqueue the seed copy and, with a capacity, the live count when it changed.  No sync."""
        if self.capacity is None:
            self.seeds.copy_(seeds)
            return
        n = int(seeds.numel())
        if not 1 <= n <= self.capacity:
            raise ValueError("a batch of %d seeds does not fit this step: 1 .. %d (batch_capacity)" % (n, self.capacity))
        self.seeds[:n].copy_(seeds)
        if n != self._n_enqueued:
            self.n_live.fill_(n)
            self._n_enqueued = n

    def _rng_kept(self):
        return _rng_kept(self.sampler, self.g)

    def calibrate(self, loader, steps=8, k_margin=1.5, b_margin=3.0):
        """GraphedTrainStep.calibrate for a sampler no train step has fixed capacities for: eager sampling to learn per-layer
        sizes (leaving generator and draw step as they were), then the static capacities."""
        if self.has_static_caps():
            raise RuntimeError("the sampler's static capacities are fixed already (a captured graph may depend on them)")
        L = len(self.sampler.nodes_per_layer)
        mx = [dict(K=0, B=0, E=0) for _ in range(L)]
        with self._rng_kept():
            for _ in range(steps):
                seeds = next(loader)
                if seeds.numel() != self._cap_s and self.capacity is None:
                    continue
                _, _, blocks = self.sampler.sample_blocks(self.g, seeds)
                for n, b in enumerate(reversed(blocks)):                  # sampling order
                    mx[n]["K"] = max(mx[n]["K"], b.num_src_nodes())
                    mx[n]["B"] = max(mx[n]["B"], b.num_edges())
                    mx[n]["E"] = max(mx[n]["E"], b._counts.E)
        fan = [self.sampler.nodes_per_layer[b] for b in reversed(range(L))]
        self._engine().set_static_caps(self._cap_s, fan, mx, k_margin, b_margin)

    # -- the batch --------------------------------------------------------------------------------------------------------
    def _body(self):
        self._batch_metric._counts.zero_()
        if self.capacity is not None:
            _, _, mfgs = self.sampler.sample_blocks_static(self.g, self.seeds, slot=self.SLOT, n_live_dev=self.n_live)
            with torch.no_grad():
                pred = self.model(mfgs, _inputs(self.model, mfgs))
                loss = self.loss_fn(pred, mfgs[-1].dstdata["labels"], n_rows_dev=self.n_live)
                _update_metric(self._batch_metric, pred, mfgs, self.n_live)
                self._batch_loss.copy_(loss.float() * self.n_live[0].float())      # loss * n, n from the device word
            return
        _, _, mfgs = self.sampler.sample_blocks_static(self.g, self.seeds, slot=self.SLOT)
        with torch.no_grad():
            pred = self.model(mfgs, _inputs(self.model, mfgs))
            loss = self.loss_fn(pred, mfgs[-1].dstdata["labels"])
            _update_metric(self._batch_metric, pred, mfgs)
            self._batch_loss.copy_(loss.float() * float(self.bs))

    def _signature(self):
        eng = self._engine()
        return (eng.ws, eng.n_bins, [dict(c) for c in eng.caps])

    def _stale(self):
        """The engine's workspaces are no longer the ones the graph was captured on (an eager sampler call elsewhere grew a
        capacity).  The graph keeps the old ones alive through ``_captured_for``; it is simply recorded again."""
        ws, n_bins, caps = self._captured_for
        eng = self._engine()
        return eng.ws is not ws or eng.n_bins != n_bins or eng.caps != caps

    def capture(self, seeds, warmup=2):
        """Static-shape warm-up batches on a side stream (allocator and the engine's per-slot buffers), then the capture.
        Leaves torch's generator, the draw step and the accumulators untouched; the model must be in eval mode."""
        import gc
        eng = self._engine()
        self.graph = None
        with self._rng_kept():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    with self._rng_kept():
                        self._load_batch(seeds)
                        eng.stage_rng_from_torch()
                        self._body()
                        side.synchronize()
                        try:
                            self.sampler.finish_static(self.SLOT)
                        except RuntimeError:
                            pass                                          # (a warm-up batch over a capacity: nothing is kept of it)
            torch.cuda.current_stream().wait_stream(side)
            gc.collect()
            torch.cuda.synchronize()
            self._load_batch(seeds)
            eng.stage_rng_from_torch()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, **_cap_kw()):
                self._body()
        self.graph, self._captured_for = graph, self._signature()
        self.captures += 1

    def _replayed(self, seeds):
        eng = self._engine()
        if self.graph is None or self._stale():
            self.capture(seeds)
        state = torch.get_rng_state()
        ds = self.sampler._draw_state_on(self.g.device) if hasattr(self.sampler, "_draw_state_on") else None
        self._load_batch(seeds)
        eng.stage_rng_from_torch()
        self.graph.replay()
        self.replays += 1
        torch.cuda.current_stream().synchronize()
        try:
            self.sampler.finish_static(self.SLOT)
        except RuntimeError:
            # over a capacity: the per-batch buffer is not added; the same draw again, eagerly (the engine regrows there)
            torch.set_rng_state(state)
            if ds is not None:
                ds.step_dev.sub_(1)                                      # as the engine's capacity-regrow loop rewinds it
            self.fallbacks += 1
            self._eager(seeds)
            return
        self.metric._counts.add_(self._batch_metric._counts)
        self._loss_sum.add_(self._batch_loss)

    def _eager(self, seeds):
        with _keep_static_caps(self._engine()):
            _, _, mfgs = self.sampler.sample(self.g, seeds)
        with torch.no_grad():
            pred = self.model(mfgs, _inputs(self.model, mfgs))
            loss = self.loss_fn(pred, mfgs[-1].dstdata["labels"])
            _update_metric(self.metric, pred, mfgs)
            self._loss_sum.add_(loss.float() * float(seeds.numel()))

    def run(self, ids):
        """One pass over ``ids`` in order: ``(micro_f1, mean_loss)``, the pair ``fit.evaluate`` returns."""
        from .metrics import micro_f1_from_counts
        was = self.model.training
        self.model.eval()
        try:
            self.metric.reset()
            self._loss_sum.zero_()
            if self.capacity is not None:
                if ids.numel() and not self.has_static_caps():      # from batches of `capacity` seeds (the whole split if it is smaller)
                    self.calibrate(BatchLoader(ids, min(self.capacity, ids.numel()), shuffle=False, drop_last=True).forever())
            elif ids.numel() >= self.bs and not self.has_static_caps():
                self.calibrate(BatchLoader(ids, self.bs, shuffle=False, drop_last=True).forever())
            for seeds in BatchLoader(ids, self.bs, shuffle=False, drop_last=False):
                if seeds.numel() == self.bs or self.capacity is not None:
                    self._replayed(seeds)
                else:
                    self._eager(seeds)
            words = [self.metric._err, self._batch_metric._err]
            st = getattr(self.loss_fn, "_state", None)
            if st is not None:
                words.append(st[1:2])
            out = torch.cat([self.metric._counts.double(), self._loss_sum.double().reshape(1)]
                            + [w.double() for w in words]).tolist()                                         # THE read-back
        finally:
            self.model.train(was)
        if any(out[5:]):                                                  # (the error words came with it: read again only to raise)
            for m in (self.metric, self._batch_metric):
                m.check_errors()
            if hasattr(self.loss_fn, "check_errors"):
                self.loss_fn.check_errors()
        self.last_counts = tuple(int(v) for v in out[:4])
        return micro_f1_from_counts(self.last_counts, self.multilabel, self.g.device), out[4] / max(ids.numel(), 1)

    def close(self):
        """Quiesce the device and destroy the captured graph now."""
        import gc
        torch.cuda.synchronize()
        self.graph, self._captured_for = None, None
        gc.collect()
        torch.cuda.synchronize()
