"""ms/step of the multinomial bandit sampler on the Reddit-like graph of bench.py: eager host draw, eager device draw, graphed
device draw.  Three alternating timed runs per mode in one process, medians.  Usage: ``python scratch/mn_draw_measure.py [out.json]``;
``python scratch/mn_draw_measure.py profile``: a dozen eager device-draw steps, to be run under ``rocprofv3 --kernel-trace --stats``."""
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
from bliss_gnn_amd.model import SAGE  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402
from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, TrainStep  # noqa: E402

dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
fan = cfg["fanouts"]


def setup(draw, graphed):
    g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
    g.edata["w"] = bg.normalized_edata(g)
    s = bg.BanditLadiesSampler(fan, importance_sampling=1, node_embedding="features", num_steps=3000, eta=0.1, draw=draw)
    if draw == "device":
        s.reset_draw(seed=7)
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    loader = BatchLoader(train_nid, cfg["batch"], shuffle=True, drop_last=True, seed=2).forever()
    if graphed:
        step = GraphedTrainStep(g, s, model, cfg["batch"], multilabel=cfg["multilabel"])
        step.calibrate(loader, steps=4)
        step.capture(loader, warmup=3)
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


if len(sys.argv) > 1 and sys.argv[1] == "profile":
    step, loader, s = setup("device", False)
    for _ in range(12):
        step(next(loader))
    torch.cuda.synchronize()
    print("sizes", [(b._counts.S, b._counts.C, b._counts.K, b._counts.B) for b in step.last["mfgs"]])
    sys.exit(0)

torch.manual_seed(3)
modes = {"eager_host": setup("host", False), "eager_device": setup("device", False), "graphed_device": setup("device", True)}
for name, (step, loader, s) in modes.items():            # warm-up
    timed(step, loader, 5)
runs = {name: [] for name in modes}
for r in range(3):
    for name, (step, loader, s) in modes.items():
        runs[name].append(timed(step, loader, 40))
        print(name, r, "%.3f ms/step" % runs[name][-1], flush=True)
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, 3-layer SAGE hidden 256, BanditLadiesSampler eta 0.1, fanouts %s, batch %d"
                   % (cfg["num_nodes"], ix.numel(), "/".join(map(str, fan)), cfg["batch"]),
       "steps_per_run": 40, "runs_ms_per_step": runs, "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
       "draw_steps": {k: v[2].draw_step() for k, v in modes.items()},
       "sizes_last_graphed": modes["graphed_device"][0].sizes()}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mn_draw_bench.json")
json.dump(out, open(path, "w"), indent=1)
print(json.dumps(out["median_ms_per_step"]))
modes["graphed_device"][0].close()
