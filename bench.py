#!/usr/bin/env python3
"""bench.py -- steps/sec of the BLISS-GNN hot path on MI355X.

One *step* = sample_blocks (3 layers) + feature gather + SAGE forward + backward + Adam + exp3 update
(validation excluded) on the workload BASELINE.json's metric is quoted on:
Reddit-shaped synthetic graph, 3-layer SAGE, poisson-bandit sampler, fanouts 4096/2048/1024, batch 256.
Synthetic data (no network): seeded Chung-Lu graph with Reddit's |V|, |E|, F, classes.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times K steps and prints the result line.  ``--full`` adds what else the benchmark measures
after the timed steps: the ``roofline`` object (the same steps launched kernel by kernel, HIP events around the library
kernels) and, on one GPU, the ``cpu_baseline`` (the oracle port of the step on the host).  ``--dump-outputs DIR`` writes what
the timed path computed in its last step as DIR/<name>.npy (see ``write_outputs``); the inputs are seeded, so two builds can
be compared array for array.

N > 1: either launched under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the environment, as the driver
does), or started plainly -- then this process starts N fresh ranks itself (a child ``python -m torch.distributed.run``,
before anything here has touched the GPU) and exits with the child's code.  ``--gpus`` that disagrees with WORLD_SIZE is
an error.  Prints ONE JSON line on rank 0.  Multi-GPU: one process per GPU, every rank holds a replica of the graph
and samples its own batch (weak scaling); gradients are all-reduced over RCCL and the EXP3 updates are
all-gathered so that the bandit state stays identical on every rank.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400,
                    help="timed steps; the default window is long enough to contain the occasional EXP3 renormalisation passes")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--config", default="reddit", choices=["cora", "pubmed", "reddit", "yelp"])
    ap.add_argument("--sampler", default="poisson-bandit", choices=["poisson-bandit", "poisson-ladies"],
                    help="train_lightning.py:536-540; poisson-ladies = the static-weight baseline sampler (no EXP3 update)")
    ap.add_argument("--model", default="sage", choices=["sage", "gat"], help="gat = SURVEY config 4 (GATv2, heads 4/4/1, hidden 256)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the roofline object and (one GPU) the CPU baseline; a plain run does neither")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step (loss, parameters, a fixed sample of the EXP3 rows, "
                         "block sizes; inference: a fixed sample of the output rows) as DIR/<name>.npy, float32 / float64, <= 64 MB")
    ap.add_argument("--cpu-baseline-steps", type=int, default=-1, help="with --full: -1: auto (bounded sample), 0: skip")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline object")
    ap.add_argument("--tune-gemm", type=int, default=1, help="1: TunableOp picks the library GEMM solutions during warm-up")
    ap.add_argument("--eager", action="store_true", help="launch kernel by kernel instead of replaying the step's HIP graph")
    ap.add_argument("--no-pipeline", action="store_true", help="one step per graph, sampling not overlapped with the backward pass")
    ap.add_argument("--force-dist", action="store_true",
                    help="single process: run the replica exchange path (gradient all-reduce, EXP3 all-gather + apply) on a world of "
                         "one rank -- what the multi-GPU step costs per GPU before any communication time")
    ap.add_argument("--dist", default="auto", choices=["auto", "replicas", "shards"],
                    help="multi-GPU layout.  shards: destination-range shards, the north star's split (bliss_gnn_amd/shard_static.py: "
                         "static shapes, dense exchanges, one HIP graph per step; --eager: the routed step of shard.py); replicas: whole "
                         "graph per rank, graph-captured pipelined step.  auto (default): shards for --gpus > 1 (SAGE, poisson-bandit), "
                         "the single-GPU step for --gpus 1.  With one GPU, shards = a world of one rank")
    ap.add_argument("--mode", default="train", choices=["train", "inference"],
                    help="inference: time SAGE.inference -- layer-wise full-neighbour evaluation of ALL nodes (model.py:335-383), the one "
                         "whole-graph SpMM of the reference -- with its own roofline (--full)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / reduction plumbing only (gloo, no GPU, no kernels): what a CPU-only box can check of --gpus N")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def relaunch_ranks(args):
    """--gpus N > 1 without a launcher: start N ranks as a CHILD process tree (never re-exec: nothing here has touched the
    GPU yet, and nothing will in this parent) and exit with its code."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def dry_run(args, rank, world):
    """No GPU: every rank joins a gloo group, 'steps' are empty, the timing reduction and the JSON line are the real ones."""
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    t1 = time.perf_counter()
    dt = time.perf_counter() - t1 + 1e-9
    t = torch.tensor([dt, float(rank)], dtype=torch.float64)
    ranks = [rank]
    if world > 1:
        dist.barrier()
        tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        got = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(got, torch.tensor([rank], dtype=torch.int64))
        ranks, dt = [int(x) for x in got], float(tmax[0])
    if rank == 0:
        print(json.dumps({"metric": "dry run (no kernels)", "value": None, "unit": "steps/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "dry_run": True, "ranks": ranks, "scaling": "weak"}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def percentiles(xs):
    xs = sorted(xs)
    if not xs:
        return None
    q = lambda f: xs[min(len(xs) - 1, max(0, int(round(f * (len(xs) - 1)))))]
    return {"p10": q(0.10), "median": q(0.50), "p90": q(0.90), "min": xs[0], "max": xs[-1], "n": len(xs)}


def algorithmic_bytes(sizes, feat, dims):
    """SURVEY.md section 8d per-step algorithmic HBM bytes from the ACTUAL sizes of a step.
    sizes: list over layers (block order 0..L-1) of dicts S,E,C,K,B;  dims: SpMM widths per layer."""
    samp = sum(8 * s["S"] + 6 * s["E"] + 12 * s["C"] + 16 * s["B"] + 6 * s["K"] for s in sizes)
    gather = 2 * sizes[0]["K"] * feat
    spmm = sum(2 * (4 * (s["S"] + 1) + 6 * s["B"] + 2 * s["K"] * d + 2 * s["S"] * d) for s, d in zip(sizes, dims))
    bandit = sum(12 * s["B"] + 4 * s["K"] + 4 * s["S"] for s in sizes)
    return dict(sampler=samp, gather=gather, spmm=spmm, bandit=bandit, total=samp + gather + spmm + bandit)


def chung_lu_graph(num_nodes, num_edges, seed, device, sigma=1.0, chunk=1 << 26):
    """bliss_gnn_amd.synth.chung_lu_csc's graph model (lognormal expected degrees, loops dropped, duplicates merged, one self
    loop per node added last), drawn so that the same seed gives the same graph in every run: torch.multinomial on the GPU
    goes through a float prefix sum whose rounding changes from run to run (torch lists CUDA cumsum among its nondeterministic
    ops), and a few of the ~114 M Reddit-like edges came out differently each time.  Here the cumulative weights are summed once
    on the host in float64 and seeded uniforms are inverted on the device; prepare_graph (csrc/prep.hip) builds the CSC with
    chung_lu_csc's numbering (edge ids dst-major, the self loops last).  Returns (indptr, indices, eid)."""
    from bliss_gnn_amd.prep import prepare_graph
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    V = int(num_nodes)
    w = torch.exp(sigma * torch.randn(V, generator=gen, device=device, dtype=torch.float32)).double().cpu()
    cdf = torch.cumsum(w, 0)
    cdf = (cdf / cdf[-1]).to(device)
    keys, left = [], int(num_edges)
    while left > 0:
        n = min(left, chunk)
        dst, src = (torch.searchsorted(cdf, torch.rand(n, generator=gen, device=device, dtype=torch.float64), right=True).clamp_(max=V - 1)
                    for _ in range(2))
        m = src != dst
        keys.append(dst[m] * V + src[m])
        left -= n
    key = torch.unique(torch.cat(keys))            # sorted: dst-major, src ascending, no duplicates
    del keys
    dst = torch.div(key, V, rounding_mode="floor")
    g = prepare_graph(key - dst * V, dst, V)
    return g.indptr, g.indices, g.eid


DUMP_LIMIT = 64 << 20                      # bytes, all arrays of one --dump-outputs together


def fixed_sample(n, k, device=None):
    """Sorted distinct ids of a fixed, seeded sample of about ``k`` of ``range(n)`` (all of them when n <= k): the same ids in
    every run with the same n."""
    if n <= k:
        return torch.arange(n, device=device)
    draw = torch.randint(0, n, (k,), generator=torch.Generator().manual_seed(12345))
    return torch.unique(draw).to(device)


def write_outputs(path, arrays):
    """--dump-outputs: each array as ``path/<name>.npy``, float64 where it is float64 or an integer (sizes, ids: exact), float32
    otherwise (bf16 values are exact in float32).  More than DUMP_LIMIT bytes in all is an error, not a silent cut."""
    import numpy as np
    out = {}
    for name, a in arrays.items():
        t = torch.as_tensor(a).detach()
        wide = t.dtype == torch.float64 or not (t.is_floating_point() or t.is_complex())
        out[name] = t.to(torch.float64 if wide else torch.float32).cpu().numpy()
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT))
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def model_outputs(model, loss, sizes=None, sampler=None):
    """What a caller of the train step holds after its last step: the loss, every parameter, the sampled block sizes (per
    layer S, E, C, K, B) and, for the bandit samplers, the EXP3 rows at a fixed sample of edge ids."""
    arrays = {"loss": torch.as_tensor(loss, dtype=torch.float32).reshape(1)}
    for name, p in model.named_parameters():
        arrays["param." + name] = p
    if sizes:
        arrays["block_sizes"] = torch.tensor([[s_.get(k, 0) for k in "SECKB"] for s_ in sizes], dtype=torch.float64)
    w = getattr(sampler, "exp3_weights", None) if sampler is not None else None
    if w is not None:
        ids = fixed_sample(w.shape[1], 1 << 20, w.device)
        arrays["exp3_weights_sample"] = w[:, ids]
        arrays["exp3_sample_edge_ids"] = ids
    return arrays


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_ranks(args))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch with --nproc-per-node equal to --gpus, or without a "
                         "launcher)" % (args.gpus, world))
    if args.dry_run:
        return dry_run(args, rank, world)
    if args.dist == "auto":
        args.dist = "shards" if (world > 1 and args.model == "sage" and args.sampler == "poisson-bandit" and args.mode == "train") else "replicas"
    force_dist = (args.force_dist or args.dist == "shards") and world == 1
    if world > 1 or force_dist:
        from bliss_gnn_amd.dist import want_hw_queues
        want_hw_queues()                                  # before the first GPU call of this process
    if force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", local))
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    import bliss_gnn_amd as bg
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.synth import CONFIGS, node_data
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, PipelinedTrainStep, TrainStep
    from bliss_gnn_amd import dist as bdist

    cfg = CONFIGS[args.config]
    t0 = time.time()
    ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
    feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                         multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
    g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
    g.edata["w"] = bg.normalized_edata(g)                                              # train_lightning.py:362
    torch.cuda.synchronize()
    t_setup = time.time() - t0

    fan, eta, hidden = cfg["fanouts"], 0.1, 256
    if args.mode == "inference":
        return bench_inference(args, g, cfg, hidden, dev, t_setup)
    if args.dist == "shards":
        return bench_shards(args, ip, ix, ei, feats, labels, train_nid, cfg, hidden, dev, rank, max(world, 1), t_setup)
    if args.sampler == "poisson-ladies":
        sampler = bg.PoissonLadiesSampler(fan)
    else:
        sampler = bg.PoissonBanditLadiesSampler(fan, importance_sampling=1, node_embedding="features", num_steps=3000, eta=eta,
                                                model=args.model)
    torch.manual_seed(1234)
    if args.model == "gat":                                  # train_lightning.py:245-249, 504-511
        from bliss_gnn_amd.model import GATv2
        model = GATv2(3, cfg["feat"], hidden, cfg["classes"], [4, 4, 1], torch.nn.functional.elu, 0.1, 0.1, 0.2, False).to(dev).bfloat16()   # :587 F.elu
    else:
        model = SAGE(cfg["feat"], hidden, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()   # train_lightning.py:609-618
    grad_sync = exp3_sync = None
    if world > 1:
        bdist.broadcast_parameters(model)
        grad_sync, exp3_sync = bdist.allreduce_gradients, bdist.exp3_all_ranks
    # every rank draws its own batches (different loader seed) and its own sampler stream
    loader = BatchLoader(train_nid, cfg["batch"], shuffle=True, drop_last=True, seed=2 + rank).forever()
    torch.manual_seed(3 + rank)                                                          # sampler stream (CPU generator)
    dims = [hidden, hidden, cfg["classes"]] if args.model == "sage" else [4 * hidden, 4 * hidden, cfg["classes"]]
    from bliss_gnn_amd import roofline
    timer = roofline.KernelTimer()
    graphed = not args.eager

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    step, launch = None, "eager (kernel by kernel)"
    if graphed:
        # the whole step (sampler + gather + fwd/bwd + [grad all-reduce] + Adam + exp3 [+ all-gather]) comes from ONE HIP
        # graph; by default two consecutive steps per graph, with the next batch's sampling overlapped with the backward pass
        try:
            cls = GraphedTrainStep if args.no_pipeline else PipelinedTrainStep
            step = cls(g, sampler, model, cfg["batch"], lr=0.002, multilabel=cfg["multilabel"], distributed=world > 1 or force_dist)
            step.calibrate(loader, steps=8)
            step.capture(loader, warmup=2, tune_gemm=args.tune_gemm)
            launch = ("one HIP graph per step" if args.no_pipeline else
                      ("one HIP graph per step on the critical stream (forward up to the output layer's input + exp3 + sampling of batch t+1); "
                       "output layer, loss, backward and Adam of batch t on a second stream, all block builds on a third, handed off through device flags") if step.use_flags else
                      "HIP graphs on two streams ordered by events (sampler | model); sampling of batch t+1 overlaps backward+Adam of batch t")
        except Exception as e:                       # e.g. a runtime that cannot capture collectives: launch kernel by kernel
            if world == 1:
                raise
            print("rank %d: graph capture failed (%r); falling back to the eager step" % (rank, e), file=sys.stderr)
            graphed, step = False, None
            if args.sampler == "poisson-ladies":
                sampler = bg.PoissonLadiesSampler(fan)
            else:
                sampler = bg.PoissonBanditLadiesSampler(fan, importance_sampling=1, node_embedding="features", num_steps=3000,
                                                        eta=eta, model=args.model)
    if not graphed:
        step = TrainStep(g, sampler, model, lr=0.002, multilabel=cfg["multilabel"], grad_sync=grad_sync, exp3_sync=exp3_sync)
    pipelined = isinstance(step, PipelinedTrainStep)
    last = {}                                                # the loss of the last step trained (for --dump-outputs)

    def advance(n, eager=False, pair_events=None):
        """Run exactly n train steps; returns the per-step block sizes (one list per sampled batch)."""
        sizes = []
        while n > 0:
            if pipelined and n >= 2 and not eager:
                got = step.run(loader, n // 2, pair_events=pair_events)
                last["loss"] = step.losses[-1]
                sizes += got
                n -= max(len(got), n // 2 * 2)              # (a capacity regrow inside run() trains three batches more)
            elif pipelined and n >= 2:
                last["loss"] = step.eager_pair(loader)[-1]
                sizes += step.sizes2()
                n -= 2
            elif pipelined:                          # an odd step: train the batch in flight, sample the next one
                last["loss"] = step.drain()
                step.prime(next(loader))
                sizes.append(step.sizes())
                n -= 1
            elif graphed:
                last["loss"] = (step.eager_step if eager else step)(next(loader))
                sizes.append(step.sizes())
                n -= 1
            else:
                last["loss"] = step(next(loader))
                sizes.append([dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in step.last["mfgs"]])
                n -= 1
        return sizes

    advance(args.warmup)
    sync()
    pair_events = [] if pipelined else None
    t1 = time.perf_counter()
    all_sizes = advance(args.steps, pair_events=pair_events)
    sync()
    dt = time.perf_counter() - t1
    steps_done = len(all_sizes)                        # == args.steps unless a capacity regrow happened inside the window (+3)
    # per-step device time: differences of timing events recorded on the critical stream at every pair boundary (two steps)
    step_ms = []
    if pair_events:
        step_ms = [0.5 * a.elapsed_time(b) for a, b in zip(pair_events[:-1], pair_events[1:])]
        if os.environ.get("BLISS_BENCH_DUMP"):          # the per-pair series with the sampled sizes beside it (tail hunting)
            with open(os.environ["BLISS_BENCH_DUMP"], "w") as f:
                json.dump({"step_ms": step_ms, "sizes": all_sizes, "host": getattr(step, "_host_trace", None)}, f)
    if pipelined and os.environ.get("BLISS_BENCH_NORMS") and hasattr(sampler, "_scratch"):
        # what F.normalize saw on every second step of 600 more: bf16 norm bits per layer (0x3f80 = 1.0 = pass skipped)
        rec = []
        for _ in range(300):
            try:
                step.run(loader, 1)
            except RuntimeError as e:
                rec.append(str(e)[:200])
                break
            finally:
                rec.append([int(v) & 0xffffff for v in sampler._scratch[:, 0].tolist()]
                           + [float(w.float().sum(dtype=torch.float64)) for w in sampler._w_pos]
                           + [float(w.float().max()) for w in sampler._w_pos] + [float(w.float().min()) for w in sampler._w_pos]
                           + sampler._row_sum.view(-1, 32, 3).sum(1).tolist())
        with open(os.environ["BLISS_BENCH_NORMS"], "w") as f:
            json.dump(rec, f)
    n_edges = sum(x["B"] for sz in all_sizes for x in sz)
    n_frontier = sum(x["E"] for sz in all_sizes for x in sz)
    sizes_acc = [{k: sum(sz[l][k] for sz in all_sizes) for k in all_sizes[0][l]} for l in range(len(all_sizes[0]))]
    t = torch.tensor([dt, float(n_edges), float(n_frontier)], dtype=torch.float64, device=dev)
    if world > 1:
        tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt, n_edges, n_frontier = float(tmax[0]), float(tsum[1]), float(tsum[2])
    if args.dump_outputs and rank == 0:                  # (before --full trains further steps)
        write_outputs(args.dump_outputs, model_outputs(model, last["loss"], all_sizes[-1], sampler))

    # ---- roofline (--full): the same steps launched kernel by kernel, HIP events around the library kernels --------
    dominant, calib, dom_timing, alg_dom = None, {}, None, 0.0
    if rank == 0 and world == 1 and args.full and not args.no_roofline:
        torch.cuda.synchronize()
        timer.enable("all")
        calib_sizes = advance(6, eager=True)
        torch.cuda.synchronize()
        calib = timer.read()
        # every library kernel with an algorithmic-byte model, the random-number generator included (one launch per step)
        hbm_kernels = {k: v for k, v in calib.items()
                       if roofline.algorithmic_bytes(k, dict(S=1, E=1, C=1, K=1, B=1), [1, 1, 1], 0)}
        for k, v in hbm_kernels.items():
            tot = sum(roofline.algorithmic_bytes(k, s_, dims, l) for sz in calib_sizes for l, s_ in enumerate(sz))
            v["alg_bytes_per_launch"] = tot / max(v["launches"], 1)
            v["GBps"] = v["alg_bytes_per_launch"] / (v["avg_us"] * 1e-6) / 1e9
        # the dominant kernel = largest total time over the calibration steps.  Two kernels are listed in all_kernels but not
        # eligible: the random-number generator (it runs BESIDE the chain on its own stream) and k_cand_number, whose last
        # workgroup hosts the wait for those numbers -- launched kernel by kernel the generator is not ahead of the sampler as it
        # is in the replayed loop, so that wait lands inside its timed duration.  Near-ties (within 5 %: k_col_sums and
        # k_bin_scatter trade places from run to run) go to the kernel that moves more bytes, so the line is stable.
        elig = {k: v for k, v in hbm_kernels.items() if k not in ("k_cand_number", "k_mt19937_uniform")} or hbm_kernels
        top = max(v["total_ms"] for v in elig.values())
        dominant = max((k for k, v in elig.items() if v["total_ms"] >= 0.95 * top), key=lambda k: elig[k]["alg_bytes_per_launch"])
        timer.enable(dominant)                       # only this kernel carries events now
        n_dom = min(args.steps, 30) // 2 * 2
        for sz in advance(n_dom, eager=True):
            alg_dom += sum(roofline.algorithmic_bytes(dominant, s_, dims, l) for l, s_ in enumerate(sz))
        torch.cuda.synchronize()
        dom_timing = timer.read().get(dominant)
        timer.enable("off")
    sampler.check_errors()
    steps_total = steps_done * world
    mean_sizes = [{k: v / steps_done for k, v in s.items()} for s in sizes_acc]
    alg = algorithmic_bytes(mean_sizes, cfg["feat"], dims)

    out = {
        "metric": "steps/sec (train step: sample_blocks + gather + %s fwd/bwd + Adam + exp3), %s-like" % ("SAGE" if args.model == "sage" else "GATv2", args.config),
        "value": steps_total / dt, "unit": "steps/s", "n_gpus": world, "steps": steps_done, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / steps_done, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {"workload": "%s-like Chung-Lu graph |V|=%d |E|=%d F=%d, 3-layer %s hidden %d, poisson-bandit eta %.1f, "
                               "fanouts %s, batch %d per GPU%s" % (args.config, g.num_nodes(), g.num_edges(), cfg["feat"],
                                                                 "SAGE" if args.model == "sage" else "GATv2 (heads 4/4/1)", hidden, eta,
                                                                 "/".join(map(str, fan)), cfg["batch"],
                                                                 "" if args.sampler == "poisson-bandit" else " [sampler: poisson-ladies, no EXP3 update]"),
                   "parallelism": ("replicas x%d (grad all-reduce + exp3 all-gather over RCCL)" % world if world > 1 else
                                   "single GPU, replica exchange path on a world of one rank" if force_dist else "single GPU"),
                   "launch": launch,
                   "global_batch": cfg["batch"] * world},
        "sampled_edges_per_sec": n_edges / dt, "frontier_edges_per_sec": n_frontier / dt,
        "sizes_per_step": mean_sizes, "algorithmic_bytes_per_step": alg,
        "algorithmic_GBps": alg["total"] * (steps_done / dt) / 1e9, "frac_of_8TBps": alg["total"] * (steps_done / dt) / 8e12,
        "setup_s": t_setup,
        # `value` is the mean over the whole timed window (EXP3 renormalisation passes included when they fall into it);
        # the distribution of the per-step device time over the same window, from events at every two-step boundary:
        "value_is": "mean over %d consecutive steps" % steps_done,
        "capacity_regrows": int(getattr(step, "regrows", 0)),
        "step_ms_percentiles": percentiles(step_ms),
    }

    if dom_timing:
        per_launch = alg_dom / dom_timing["launches"]
        achieved = per_launch / (dom_timing["avg_us"] * 1e-6) / 1e9
        traffic, traffic_src = None, None
        import glob
        pmc_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))   # separate rocprofv3 --pmc passes
        # (the passes of THIS workload: a GATv2 run's file carries the same sampler kernels, but it is not this command's)
        pmc_files = [f for f in pmc_files if ("gat" in os.path.basename(f)) == (args.model == "gat")] or pmc_files
        pmc_file = pmc_files[-1] if pmc_files else ""
        if pmc_file:
            raw = json.load(open(pmc_file))
            # profiler symbol(s) of the timed kernel id: k_spmm_fwd / k_spmm_bwd are the BWD = false / true instantiations of k_spmm<>
            if dominant in ("k_spmm_fwd", "k_spmm_bwd"):
                want = "true>" if dominant == "k_spmm_bwd" else "false>"
                rows = [v for k, v in raw.items() if k.startswith("k_spmm<") and k.endswith(want)]
            else:
                # timer id -> profiler symbol where the two differ
                sym = {"k_mt19937_uniform": "k_mt19937_stream", "k_select_pass2": "k_select_fused", "k_bitmap_scan": "k_bitmap_tiles",
                       "k_indptr_scan": "k_block_scans", "k_block_transpose": "k_tr_sort_lists"}.get(dominant, dominant)
                rows = [v for k, v in raw.items() if k.split("<")[0] == sym]
            if rows:
                # KiB counters; FETCH_SIZE doubled per MI355X_MICROARCH.md (64 B tallied per 128-B request on gfx950);
                # launch-weighted mean over the instantiations
                n = sum(r["launches"] for r in rows)
                traffic = 1024.0 * sum(r["launches"] * (r["fetch_KiB_x2_corrected"] + r["write_KiB_per_launch"]) for r in rows) / max(n, 1)
                traffic_src = "profiles/%s: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (two passes), bytes per launch" % os.path.basename(pmc_file)
        out["roofline"] = {"bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": roofline.HBM_PEAK_GBPS, "unit": "GB/s",
                           "frac": achieved / roofline.HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_src,
                           "avg_launch_us": dom_timing["avg_us"], "launches": dom_timing["launches"],
                           "measured_over": "%d kernel-by-kernel runs of the same step right after the timed region" % n_dom,
                           "algorithmic_bytes_per_launch": per_launch,
                           "kernel_time_share_in_calibration": {k: round(v["total_ms"] / max(sum(x["total_ms"] for x in calib.values()), 1e-9), 4)
                                                                for k, v in sorted(calib.items(), key=lambda kv: -kv[1]["total_ms"])[:8]},
                           # the other library kernels of the step, same definition (HIP events, kernel-by-kernel launches)
                           "all_kernels": {k: {"avg_launch_us": round(v["avg_us"], 2), "launches_per_step": round(v["launches"] / 6.0, 2),
                                               "algorithmic_bytes_per_launch": round(v["alg_bytes_per_launch"]),
                                               "achieved_GBps": round(v["GBps"], 1), "frac": round(v["GBps"] / roofline.HBM_PEAK_GBPS, 5)}
                                           for k, v in sorted(hbm_kernels.items(), key=lambda kv: -kv[1]["total_ms"])}}
    if rank == 0 and world == 1 and args.full and args.cpu_baseline_steps != 0:
        out["cpu_baseline"] = cpu_baseline(g, feats, labels, train_nid, cfg, fan, eta, hidden, args.cpu_baseline_steps)
    if rank == 0:
        print(json.dumps(out), flush=True)
    # teardown in dependency order: the batch in flight, every stream of the loop, the captured graphs (they hold RCCL
    # nodes), only then the communicator -- graphs that outlive it abort the process at exit
    if hasattr(step, "close"):
        step.close()
    del step
    torch.cuda.synchronize()
    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()


def bench_shards(args, ip, ix, ei, feats, labels, train_nid, cfg, hidden, dev, rank, world, t_setup):
    """The destination-range-sharded step: every rank owns a node range, draws its batch from the train ids it owns (weak
    scaling: global batch = world x batch) and takes part in one global step at a time.  Default: the STATIC-SHAPE step of
    bliss_gnn_amd/shard_static.py (dense exchanges, no host sync, one HIP graph per step over RCCL); ``--eager``: the routed
    step of bliss_gnn_amd/shard.py with its host sync per exchange."""
    from bliss_gnn_amd import roofline
    from bliss_gnn_amd import shard as sh
    from bliss_gnn_amd import shard_static as ss
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader
    bounds = sh.partition_by_in_edges(ip, world)
    g = sh.GraphShard.from_global(ip, ix, ei, bounds, rank, device=dev, ndata={"features": feats, "labels": labels})
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], hidden, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    mine = train_nid[(train_nid >= g.lo) & (train_nid < g.hi)]
    loader = BatchLoader(mine, cfg["batch"], shuffle=True, drop_last=True, seed=2 + rank).forever()
    static = not args.eager
    edges_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    last = {}                                                      # the loss of the last step (for --dump-outputs)
    if static:
        caps = None
        if os.environ.get("BLISS_SHARD_CALIBRATE", "1") != "0":     # capacities from observed sizes (a throw-away model / EXP3 state)
            caps = ss.measure_caps(g, cfg["fanouts"], model, cfg["batch"], loader, steps=4, eta=0.1, seed=7, multilabel=cfg["multilabel"])
        sampler = ss.DenseShardedSampler(g, cfg["fanouts"], eta=0.1, seed=7, fixed_caps=caps)
        pipelined = os.environ.get("BLISS_SHARD_PIPELINE", "1") != "0"
        cls = ss.PipelinedShardedTrainStep if pipelined else ss.StaticShardedTrainStep
        step = cls(g, sampler, model, cfg["batch"], lr=0.002, multilabel=cfg["multilabel"])
        launch = "static shapes, launched kernel by kernel (no host sync inside a step)"
        if (world == 1 or dist.get_backend() == "nccl") and os.environ.get("BLISS_SHARD_GRAPH", "1") != "0":
            try:
                step.capture(loader, warmup=2)
                launch = ("%s per step on two streams (static shapes): forward + EXP3 and the next batch's sampling with its "
                          "dense all-reduces on the critical stream; loss, backward, gradient all-reduce and Adam beside them, on a "
                          "communicator of their own" % (("three HIP graphs on three streams (the third builds the next batch's blocks) ordered by device flags" if step.use_third else
                                                          ("two HIP graphs ordered by device flags, the input-most block built on the backward stream beside the next forward pass's first transform" if step.late_block else "two HIP graphs ordered by device flags")) if step.use_flags else
                                                         "three HIP graphs ordered by stream events")) if pipelined else \
                         "ONE HIP graph per step: sampler + its dense all-reduces + halo all-reduces + model + Adam + EXP3 (static shapes)"
            except Exception as e:                                 # noqa: BLE001 -- a runtime that cannot capture collectives
                print("rank %d: graph capture of the sharded step failed (%r); static shapes, eager launches" % (rank, e), file=sys.stderr)
                step.graph = None
        if pipelined and not step.primed:
            step.prime(next(loader))

        def one():
            last["loss"] = step(next(loader))
            cnt = sampler._slot_bufs(step.slot if pipelined else 0)["counts"]
            if pipelined and step.graph is not None and (step.use_third or step.late_block):
                # (the blocks just sampled are finished on another stream: the third one, or the backward stream for the last block)
                with torch.cuda.stream(step.third if step.use_third else step.side):
                    edges_dev.add_(cnt[4::10].sum())
            else:
                edges_dev.add_(cnt[4::10].sum())
    else:
        sampler = sh.ShardedPoissonBanditSampler(g, cfg["fanouts"], eta=0.1, seed=7)
        step = sh.ShardedTrainStep(g, sampler, model, lr=0.002, multilabel=cfg["multilabel"])
        launch = "eager, routed exchanges (one host sync per exchange)"

        def one():
            last["loss"] = step(next(loader))
            edges_dev.add_(sum(b.num_edges() for b in step.last["mfgs"]))
    for _ in range(args.warmup):
        one()
    if static and step.graph is not None:
        # the replayed loop is checked BEFORE it is timed (error words, flag time-outs), on every rank; if any rank objects, all ranks
        # go on with the same step launched kernel by kernel (same collectives in the same order, so the ranks stay in step)
        ok = torch.ones(1, dtype=torch.int32, device=dev)
        try:
            step.finish()
        except RuntimeError as e:
            print("rank %d: the captured sharded loop failed its check (%s)" % (rank, e), file=sys.stderr)
            ok.zero_()
        if world > 1:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 0:
            step.graph = None
            launch = "static shapes, launched kernel by kernel (the captured loop failed its check on this node)"
            eng = sampler.ops.eng
            for w in (sampler._bufs["err"], eng.flag_err, eng.flags):
                w.zero_()
            torch.cuda.synchronize()
            if pipelined:
                step.prime(next(loader))
            for _ in range(max(2, args.warmup // 4)):
                one()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    edges_dev.zero_()
    t1 = time.perf_counter()
    for _ in range(args.steps):
        one()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    edges = float(edges_dev.item())
    t = torch.tensor([dt, edges], dtype=torch.float64, device=dev)
    if world > 1:
        tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt, edges = float(tmax[0]), float(tsum[1])
    sizes = None
    if static:
        _, sizes = step.finish()                                   # (error words, capacity overflows, flag time-outs: a bad run raises here)
    else:
        sampler.check_errors()
    if args.dump_outputs and rank == 0:                            # (before --full trains further steps)
        write_outputs(args.dump_outputs, model_outputs(model, last["loss"], sizes))
    roof = None
    if static and rank == 0 and args.full and not args.no_roofline:
        # the dominant library kernel of the sampler, timed with HIP events over a few steps launched kernel by kernel
        # (every rank must take part in the steps: the others run them too, below)
        timer = roofline.KernelTimer()
        timer.enable("k_bin_scatter")
    n_roof = 0 if (not static or args.no_roofline or not args.full) else 6
    if n_roof:
        saved, step.graph = step.graph, None
        alg = 0.0
        for _ in range(n_roof):
            step(next(loader))
            loss, sizes = step.finish()
            alg += sum(roofline.algorithmic_bytes("k_bin_scatter", dict(S=z["S"], E=z["E"], C=0, K=z["K"], B=z["B"])) for z in sizes)
        step.graph = saved
        if rank == 0:
            tm = timer.read().get("k_bin_scatter")
            timer.enable("off")
            if tm:
                ach = alg / tm["launches"] / (tm["avg_us"] * 1e-6) / 1e9
                roof = {"bound": "hbm", "kernel": "k_bin_scatter", "achieved": ach, "peak": roofline.HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": ach / roofline.HBM_PEAK_GBPS, "traffic": None, "avg_launch_us": tm["avg_us"], "launches": tm["launches"],
                        "algorithmic_bytes_per_launch": alg / tm["launches"],
                        "note": "this rank's shard of the frontier; the step's other cost is the exchanges (bytes_per_rank_per_step)"}
    if rank == 0:
        out = {
            "metric": "steps/sec (train step: sample_blocks + gather + SAGE fwd/bwd + Adam + exp3; destination-range shards, one step = "
                      "%d seeds per GPU), %s-like" % (cfg["batch"], args.config),
            "value": args.steps * world / dt, "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic",
            "config": {"workload": "%s-like Chung-Lu graph |V|=%d, 3-layer SAGE hidden %d, sharded poisson-bandit (keyed draws) fanouts %s, "
                                   "batch %d per GPU" % (args.config, ip.numel() - 1, hidden, "/".join(map(str, cfg["fanouts"])), cfg["batch"]),
                       "parallelism": ("destination-range shards x%d (per layer ONE dense int64 [|V|,2] all-reduce; halo rows as capacity-sized "
                                       "all-reduces; gradient, EXP3 row-sum and loss all-reduces)" % world) if static else
                                      ("destination-range shards x%d (partials all-to-all, histogram all-reduce, kept-list all-gather, halo "
                                       "gathers, gradient all-reduce)" % world),
                       "launch": launch, "global_batch": cfg["batch"] * world},
            "sampled_edges_per_sec": edges / dt, "setup_s": t_setup}
        if static:
            out["bytes_per_rank_per_step"] = int(step.bytes_per_step)
            out["roofline"] = roof
        print(json.dumps(out), flush=True)
    if static:
        step.close()
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def bench_inference(args, g, cfg, hidden, dev, t_setup):
    """SAGE.inference over the whole graph (train_lightning.py:686-705 -> model.py:335-383): per layer one mean-SpMM over all
    |E_g| edges + the two Linear layers.  A 'step' here = one full inference pass (3 layers, all nodes)."""
    from bliss_gnn_amd import roofline
    from bliss_gnn_amd.model import SAGE
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], hidden, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    V, E = g.num_nodes(), g.num_edges()
    timer = roofline.KernelTimer()
    for _ in range(max(1, min(args.warmup, 2))):
        model.inference(g)
    torch.cuda.synchronize()
    n = args.steps
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        h = model.inference(g)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]
    if args.dump_outputs:                         # the output rows of the last pass at a fixed sample of node ids
        rows = fixed_sample(V, max(1, (16 << 20) // (4 * h.shape[1])), h.device)
        write_outputs(args.dump_outputs, {"inference_rows_sample": h[rows], "inference_sample_node_ids": rows})
    spmm = None
    if args.full and not args.no_roofline:        # one more pass, HIP events around the SpMM launches
        timer.enable("k_spmm_fwd")
        model.inference(g)
        torch.cuda.synchronize()
        spmm = timer.read().get("k_spmm_fwd")
        timer.enable("off")
    dims = [hidden, hidden, cfg["classes"]]                       # SpMM widths (in > out: the Linear runs first), SURVEY.md m2
    # algorithmic HBM bytes of the aggregation per layer: CSC pointers + indices once, the feature rows in, the result out
    layer_bytes = [4 * (V + 1) + 4 * E + 2 * V * d * 2 for d in dims]
    total = float(sum(layer_bytes))
    mean_ms = sum(ms) / len(ms)
    out = {"metric": "full-neighbour inference passes/sec (SAGE.inference, all %d nodes, 3 layers), %s-like" % (V, args.config),
           "value": 1e3 / mean_ms, "unit": "passes/s", "n_gpus": 1, "steps": n, "warmup": args.warmup, "ms_per_step": mean_ms,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": "%s-like Chung-Lu graph |V|=%d |E|=%d F=%d, 3-layer SAGE hidden %d, layer-wise full-neighbour inference"
                                  % (args.config, V, E, cfg["feat"], hidden)},
           "pass_ms_percentiles": percentiles(ms), "edges_per_sec": 3.0 * E / (mean_ms * 1e-3), "setup_s": t_setup}
    if spmm:
        achieved = total / (spmm["total_ms"] * 1e-3) / 1e9
        # what the kernel actually moves into the CUs: one D-wide bf16 row per edge (|E| x 2 D bytes per layer), gathered from a
        # [V, D] table of ~120 MB that lives in the 256 MiB Infinity Cache, not in the 4 MiB L2s.  MI355X_MICROARCH.md (section
        # "Indexed rows: gather into LDS") measures 7.4-7.9 TB/s chip-wide for uniformly random rows of a 151 MB table: that,
        # not the HBM peak, is this kernel's ceiling.
        gather_bytes = float(sum(2 * E * d for d in dims))
        gather_gbps = gather_bytes / (spmm["total_ms"] * 1e-3) / 1e9
        traffic, pmc = None, None
        import glob
        pm = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_inference_pmc.json")))
        if pm:
            pmc = json.load(open(pm[-1]))
            if "fetch_bytes_per_pass_x2_corrected" in pmc:
                traffic = pmc["fetch_bytes_per_pass_x2_corrected"] + pmc.get("write_bytes_per_pass", 0.0)
        out["roofline"] = {"bound": "hbm", "kernel": "k_spmm_fwd (mean over ALL in-edges, %d launches per pass)" % spmm["launches"],
                           "achieved": achieved, "peak": roofline.HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / roofline.HBM_PEAK_GBPS,
                           "traffic": traffic, "traffic_source": None if not pm else "profiles/%s (three rocprofv3 --pmc passes, bytes per inference pass)" % os.path.basename(pm[-1]),
                           "algorithmic_bytes_per_pass": total, "spmm_ms_per_pass": spmm["total_ms"],
                           "gather_bytes_per_pass": gather_bytes, "gather_GBps": gather_gbps,
                           "gather_ceiling_GBps": [7400.0, 7900.0], "gather_frac_of_ceiling": gather_gbps / 7400.0,
                           "pmc": pmc,
                           "note": "algorithmic bytes = 4(V+1) + 4|E| + 2 V D (in) + 2 V D (out) per layer (what must cross HBM once); the kernel's "
                                   "own bound is the row gather: |E| x 2D bytes per layer out of a cache-resident table, ceiling 7.4-7.9 TB/s "
                                   "(MI355X_MICROARCH.md, 151 MB table, uniformly random rows)"}
    print(json.dumps(out), flush=True)


def host_cpu():
    """(model name, physical cores, logical CPUs) of the host, from /proc/cpuinfo."""
    model, cores, logical = "unknown", set(), 0
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "processor":
                logical += 1
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
                cores.add((phys, core))
    except OSError:
        pass
    logical = logical or (os.cpu_count() or 1)
    return model, (len(cores) or logical), logical


def cpu_baseline(g, feats, labels, train_nid, cfg, fan, eta, hidden, n_steps, budget_s=30.0):
    """The oracle port of the same step on the host's physical cores, on a BOUNDED sample: at least two
    timed steps, at most ten, as many as fit ``budget_s`` seconds going by the (untimed) first step -- the line says which
    limit applied.  A correctness restatement being timed, not a tuned CPU implementation: a reported baseline, not a target."""
    from oracle import bliss_oracle as bo
    from oracle.train_ref import RefTrainStep
    model_name, phys, logical = host_cpu()
    try:
        avail = len(os.sched_getaffinity(0))                     # (a container may expose fewer CPUs than the host has)
    except AttributeError:
        avail = logical
    threads = max(1, min(phys, avail))
    try:                                                         # (a host shared with other jobs says how many CPUs are ours)
        threads = min(threads, max(1, int(os.environ["OMP_NUM_THREADS"])))
    except (KeyError, ValueError):
        pass
    torch.set_num_threads(threads)
    og = bo.CSC(g.indptr.cpu(), g.indices.cpu(), g.eid.cpu())
    ref = RefTrainStep(og, feats.cpu(), labels.cpu(), fan, eta, cfg["feat"], hidden, cfg["classes"], multilabel=cfg["multilabel"])
    ids = train_nid.cpu()
    bs = cfg["batch"]
    torch.manual_seed(3)
    t0 = time.perf_counter()
    ref(ids[:bs])                                       # first step allocates + normalises from ones; not timed
    first = time.perf_counter() - t0
    fit = int(budget_s / max(first, 1e-3))
    n = n_steps if n_steps > 0 else max(2, min(10, fit))
    n = min(n, max(1, ids.numel() // bs - 1))
    t0 = time.perf_counter()
    edges = 0
    for i in range(1, n + 1):
        _, blocks = ref(ids[i * bs:(i + 1) * bs])
        edges += sum(b.src.numel() for b in blocks)
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "steps/s", "cores": threads, "kind": "port",
            "sample": "%d steps of the same workload (oracle sampler + torch-CPU SAGE fwd/bwd + Adam + exp3), after 1 untimed step of %.1f s"
                      % (n, first),
            "steps_timed": n, "seconds_timed": dt, "budget_s": budget_s,
            "limited_by": "explicit --cpu-baseline-steps" if n_steps > 0 else ("time budget" if fit < 10 else "10-step cap"),
            "sampled_edges_per_sec": edges / dt, "host_cpu_model": model_name, "host_physical_cores": phys, "host_cpu_count": logical,
            "cpus_available_to_the_process": avail}


if __name__ == "__main__":
    main()
