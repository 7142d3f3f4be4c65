"""GCN on the bounded kernels on the Reddit-like graph of bench.py: a 3-layer GCN (hidden 256, ReLU, dropout
0.1), ``poisson-bandit`` 4096/2048/1024, batch 256, ``GraphedTrainStep``:

  (a) tile against library   equal static shapes (no capacity), ``transforms="library"`` against ``"tile"``: three alternating
                             windows of 100 replayed steps in one process, each window ending in one device sync; medians.
  (b) capacity overhead      the tile model, static at 256 seeds against ``batch_capacity=512`` with 256 live, the same way.
  count MODE N               N replayed steps of one mode and nothing else measured: run it under ``rocprofv3 --kernel-trace
                             --stats`` with two values of N; the difference of the launch totals over the difference of N is the
                             launches per step.
  launches JSON DIR N1 N2    reads DIR/<mode>_<N>/**/*kernel_stats.csv of those four runs and writes the launches per step into JSON.

Usage: ``python scratch/gcn_tile_measure.py [out.json]``, ``... count library|tile N``, ``... launches out.json dir N1 N2``."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if len(sys.argv) > 1 and sys.argv[1] == "launches":
    path, base, n1, n2 = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    out = json.load(open(path)) if os.path.exists(path) else {}
    per = {}
    for mode in ("library", "tile"):
        tot = {}
        for n in (n1, n2):
            files = glob.glob(os.path.join(base, "%s_%d" % (mode, n), "**", "*kernel_stats.csv"), recursive=True)
            tot[n] = sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))
        per[mode] = {"launches_at_%d_steps" % n1: tot[n1], "launches_at_%d_steps" % n2: tot[n2], "launches_per_step": (tot[n2] - tot[n1]) / (n2 - n1)}
    out["launches"] = per
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(per))
    sys.exit(0)

import torch  # noqa: E402

import bliss_gnn_amd as bg  # noqa: E402
from bench import chung_lu_graph  # noqa: E402
from bliss_gnn_amd.model import GCN  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402
from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep  # noqa: E402

BS, CAP, FAN = 256, 512, [4096, 2048, 1024]
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
g.edata["w"] = bg.normalized_edata(g)


def step_(transforms, capacity=None):
    torch.manual_seed(1234)
    model = GCN(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1, transforms=transforms).to(dev).bfloat16()
    model.train()
    sampler = bg.PoissonBanditLadiesSampler(FAN, importance_sampling=1, node_embedding="features", num_steps=3000, eta=0.1)
    step = GraphedTrainStep(g, sampler, model, BS, multilabel=cfg["multilabel"], **({} if capacity is None else dict(batch_capacity=capacity)))
    torch.manual_seed(3)
    step.calibrate(BatchLoader(train_nid, capacity or BS, seed=2).forever(), steps=8)
    loader = BatchLoader(train_nid, BS, seed=2).forever()
    cal = BatchLoader(train_nid, capacity or BS, seed=3).forever()
    step.capture(cal, warmup=2)
    for _ in range(5):
        step(next(loader))
    return step, loader


def timed(step, loader, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step(next(loader))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def windows(modes, n=100):
    runs = {k: [] for k in modes}
    for r in range(3):
        for k, (step, loader) in modes.items():
            runs[k].append(timed(step, loader, n))
            print(k, r, "%.3f ms/step" % runs[k][-1], flush=True)
    out = {"steps_per_window": n, "windows_ms_per_step": runs, "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
           "last_loss": {k: float(st.loss) for k, (st, _) in modes.items()}}
    for st, _ in modes.values():
        st.close()
    return out


if len(sys.argv) > 1 and sys.argv[1] == "count":
    step, loader = step_(sys.argv[2])
    for _ in range(int(sys.argv[3])):
        step(next(loader))
    torch.cuda.synchronize()
    step.close()
    sys.exit(0)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gcn_tile.json")
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, GCN 3 layers hidden 256 (ReLU, dropout 0.1), poisson-bandit 4096/2048/1024, "
                   "batch %d; host clock around windows of per-step replays that end in one device sync" % (cfg["num_nodes"], ix.numel(), BS)}
out["tile_vs_library"] = windows({"library": step_("library"), "tile": step_("tile")})
json.dump(out, open(path, "w"), indent=1)
out["capacity_overhead"] = windows({"tile_static_256": step_("tile"), "tile_capacity_512_live_256": step_("tile", CAP)})
json.dump(out, open(path, "w"), indent=1)
print(json.dumps({k: out[k]["median_ms_per_step"] for k in ("tile_vs_library", "capacity_overhead")}))
