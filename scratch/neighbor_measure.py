"""ms/step of the neighbor sampler on the Reddit-like graph of bench.py (batch 256, 3-layer SAGE hidden 256): (a) TrainStep with
draw="host" (the torch-op path), (b) TrainStep with draw="device", (c) GraphedTrainStep with draw="device"; fanouts 15/10/5 and
4096/2048/1024.  Three alternating timed runs per mode in one process, medians.
Usage: ``python scratch/neighbor_measure.py [out.json] [small|large|both]``."""
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

dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})


def setup(fan, draw, graphed):
    s = fit.NeighborSampler(fan, seed=7, draw=draw)
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    loader = BatchLoader(train_nid, cfg["batch"], shuffle=True, drop_last=True, seed=2).forever()
    if graphed:
        step = GraphedTrainStep(g, s, model, cfg["batch"], multilabel=cfg["multilabel"])
        step.calibrate(loader, steps=4)
        step.capture(loader, warmup=2)
    else:
        step = TrainStep(g, s, model, multilabel=cfg["multilabel"])
    return step, loader, s


def timed(step, loader, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step(next(loader))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def measure(fan, steps):
    modes = {"a_eager_host": setup(fan, "host", False), "b_eager_device": setup(fan, "device", False),
             "c_graphed_device": setup(fan, "device", True)}
    for name, (step, loader, s) in modes.items():            # warm-up
        timed(step, loader, 3)
    runs = {name: [] for name in modes}
    for r in range(3):
        for name, (step, loader, s) in modes.items():
            runs[name].append(timed(step, loader, steps))
            print("/".join(map(str, fan)), name, r, "%.3f ms/step" % runs[name][-1], flush=True)
    out = {"fanouts": fan, "steps_per_run": steps, "runs_ms_per_step": runs,
           "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
           "sizes_last_graphed": modes["c_graphed_device"][0].sizes()}
    modes["c_graphed_device"][0].close()
    return out


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "neighbor_bench.json")
which = sys.argv[2] if len(sys.argv) > 2 else "both"
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, 3-layer SAGE hidden 256, NeighborSampler, batch %d"
                   % (cfg["num_nodes"], ix.numel(), cfg["batch"]), "configs": []}
if which in ("small", "both"):
    out["configs"].append(measure([15, 10, 5], 40))
    json.dump(out, open(path, "w"), indent=1)
if which in ("large", "both"):
    out["configs"].append(measure([4096, 2048, 1024], 5))
json.dump(out, open(path, "w"), indent=1)
print(json.dumps([c["median_ms_per_step"] for c in out["configs"]]))
