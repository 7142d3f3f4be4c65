"""ms/step of the train loops ``fit`` can drive on the Reddit-like graph of bench.py, batch 256, 3-layer SAGE
hidden 256:

  poisson-bandit 4096/2048/1024   "eager": TrainStep with the loss read back per step (fit's train_step="eager": the yardstick);
                                  "run": GraphedTrainStep(ledger=True).run -- the per-step protocol of the Poisson samplers
  labor 15/10/5                   "eager"; "call": GraphedTrainStep.__call__ per step; "free": the free-running ``run``

Three alternating windows of 200 steps per variant in one process; the host clock around a window that ends in one device sync;
medians with the three windows beside them.  Usage: ``python scratch/fit_graphed_measure.py [out.json]``."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bliss_gnn_amd as bg  # noqa: E402
from bench import chung_lu_graph  # noqa: E402
from bliss_gnn_amd import fit  # noqa: E402
from bliss_gnn_amd.model import SAGE  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402
from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep  # noqa: E402

STEPS = 200
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
g.edata["w"] = bg.normalized_edata(g)


def setup(sampler_name, fan, variant):
    s = fit.make_sampler(sampler_name, fan)
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    model.train()
    loader = BatchLoader(train_nid, cfg["batch"], shuffle=True, drop_last=True, seed=2).forever()
    if variant == "eager":
        step = TrainStep(g, s, model, multilabel=cfg["multilabel"])

        def window(n):
            tot = 0.0
            for _ in range(n):
                tot += float(step(next(loader)))                 # fit's eager loop
            return tot
        return step, window
    step = GraphedTrainStep(g, s, model, cfg["batch"], multilabel=cfg["multilabel"], ledger=variant != "call")
    step.calibrate(loader, steps=8)
    step.capture(loader, warmup=2)
    if variant == "call":
        def window(n):
            for _ in range(n):
                step(next(loader))
    else:
        def window(n):
            step.run(loader, n)
    return step, window


def timed(window, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    window(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def measure(sampler_name, fan, variants):
    modes = {v: setup(sampler_name, fan, v) for v in variants}
    for _, window in modes.values():
        timed(window, 10)                                        # warm-up
    runs = {v: [] for v in variants}
    for r in range(3):
        for v, (_, window) in modes.items():
            runs[v].append(timed(window, STEPS))
            print(sampler_name, "/".join(map(str, fan)), v, r, "%.3f ms/step" % runs[v][-1], flush=True)
    out = {"sampler": sampler_name, "fanouts": fan, "steps_per_window": STEPS, "windows_ms_per_step": runs,
           "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
           "regrows": {v: getattr(st, "regrows", 0) for v, (st, _) in modes.items()}}
    for st, _ in modes.values():
        if hasattr(st, "close"):
            st.close()
    return out


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fit_graphed_bench.json")
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, 3-layer SAGE hidden 256, batch %d; host clock around %d-step windows "
                   "that end in one device sync" % (cfg["num_nodes"], ix.numel(), cfg["batch"], STEPS), "configs": []}
for name, fan, variants in (("poisson-bandit", [4096, 2048, 1024], ("eager", "run")), ("labor", [15, 10, 5], ("eager", "call", "free"))):
    out["configs"].append(measure(name, fan, variants))
    json.dump(out, open(path, "w"), indent=1)
print(json.dumps([{k: c[k] for k in ("sampler", "median_ms_per_step", "regrows")} for c in out["configs"]]))
