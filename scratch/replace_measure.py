"""ms/step and sampled sizes of GraphedTrainStep with the draws WITH replacement of csrc/replace_draw.hip
against the draws without, on the Reddit-like graph of bench.py (batch 256, 3-layer SAGE hidden 256):
  node-wise, fanouts 15/10/5 and 10/10/10: ``NeighborSampler(draw="device")`` -- the yardstick -- against the same with
  ``replace=True`` and with ``replace=True, prob="w"``;
  layer-wise, 4096/2048/1024: ``LadiesSampler(draw="device")`` against ``draw="device-replace"``.
Three alternating timed windows of 40 replayed steps per sampler in one process, medians with the windows beside them; per sampler
also the mean K and B of every layer over the timed steps.  Usage: ``python scratch/replace_measure.py [out.json]``."""
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
from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep  # noqa: E402

dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
g.edata["w"] = bg.normalized_edata(g)
NODE_WISE = ("neighbor", "neighbor-replace", "neighbor-replace-prob")
LAYER_WISE = ("ladies", "ladies-replace")


def setup(fan, name):
    if name.startswith("ladies"):
        s = bg.LadiesSampler(fan, draw="device-replace" if name == "ladies-replace" else "device")
        s.reset_draw(seed=7)
    else:
        s = fit.NeighborSampler(fan, seed=7, draw="device", replace=name != "neighbor", prob="w" if name.endswith("prob") else None)
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    loader = BatchLoader(train_nid, cfg["batch"], shuffle=True, drop_last=True, seed=2).forever()
    step = GraphedTrainStep(g, s, model, cfg["batch"], multilabel=cfg["multilabel"])
    step.calibrate(loader, steps=8)
    step.capture(loader, warmup=2)
    return step, loader


def timed(step, loader, n, sizes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step(next(loader))
        sizes.append(step.sizes())                           # (host data of the step's own end-of-step read-back)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def measure(fan, names, steps):
    modes = {name: setup(fan, name) for name in names}
    for step, loader in modes.values():                      # warm-up
        timed(step, loader, 5, [])
    runs, sizes = {name: [] for name in modes}, {name: [] for name in modes}
    for r in range(3):
        for name, (step, loader) in modes.items():
            runs[name].append(timed(step, loader, steps, sizes[name]))
            print("/".join(map(str, fan)), name, r, "%.3f ms/step" % runs[name][-1], flush=True)
    out = {"fanouts": fan, "steps_per_window": steps, "windows_ms_per_step": runs,
           "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
           "mean_K_per_layer_input_first": {k: [statistics.fmean(s[n]["K"] for s in v) for n in range(len(fan))] for k, v in sizes.items()},
           "mean_B_per_layer_input_first": {k: [statistics.fmean(s[n]["B"] for s in v) for n in range(len(fan))] for k, v in sizes.items()}}
    for step, _ in modes.values():
        step.sampler.check_errors()
        step.close()
    return out


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "replace_bench.json")
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, 3-layer SAGE hidden 256, GraphedTrainStep, batch %d"
                   % (cfg["num_nodes"], ix.numel(), cfg["batch"]), "configs": []}
for fan, names in (([15, 10, 5], NODE_WISE), ([10, 10, 10], NODE_WISE), ([4096, 2048, 1024], LAYER_WISE)):
    out["configs"].append(measure(fan, names, 40))
    json.dump(out, open(path, "w"), indent=1)
print(json.dumps([{k: c[k] for k in ("fanouts", "median_ms_per_step", "mean_K_per_layer_input_first", "mean_B_per_layer_input_first")}
                  for c in out["configs"]]))
