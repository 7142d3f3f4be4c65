"""ms/step of ``GraphedTrainStep(ledger=True).run`` with the two draws of the Poisson bandit sampler on the
Reddit-like graph of bench.py, batch 256, 3-layer SAGE hidden 256, fanouts 4096/2048/1024:

  "stream": ``poisson-bandit`` -- the draw against torch's CPU stream; ``run`` keeps the per-step protocol (stage, replay, one sync,
            ``finish_static``) and a generator kernel runs beside every step's candidate chain (the yardstick)
  "keyed":  ``poisson-bandit-keyed`` -- the keyed draw on the device; ``run`` is free-running

Three alternating windows of 200 steps per variant in one process; the host clock around a window that ends in one device sync;
medians with the three windows beside them, and the ledger's mean sizes per layer.  Usage:
``python scratch/poisson_keyed_measure.py [out.json]``."""
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

STEPS, FAN = 200, [4096, 2048, 1024]
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
g.edata["w"] = bg.normalized_edata(g)


def setup(sampler_name):
    s = fit.make_sampler(sampler_name, FAN)
    torch.manual_seed(1234)
    model = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    model.train()
    loader = BatchLoader(train_nid, cfg["batch"], shuffle=True, drop_last=True, seed=2).forever()
    step = GraphedTrainStep(g, s, model, cfg["batch"], multilabel=cfg["multilabel"], ledger=True)
    step.calibrate(loader, steps=8)
    step.capture(loader, warmup=2)
    return step, lambda n: step.run(loader, n)


def timed(window, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    window(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


torch.manual_seed(3)
modes = {"stream": setup("poisson-bandit"), "keyed": setup("poisson-bandit-keyed")}
for _, window in modes.values():
    timed(window, 10)                                            # warm-up
runs = {v: [] for v in modes}
for r in range(3):
    for v, (_, window) in modes.items():
        runs[v].append(timed(window, STEPS))
        print(v, r, "%.3f ms/step" % runs[v][-1], flush=True)
sizes = {}
for v, (st, _) in modes.items():
    rec = st.ledger()
    sizes[v] = {"steps": rec["steps_total"], "mean_nodes_input_to_output": [st.num_sampled_nodes(i, rec) for i in range(4)],
                "mean_edges_per_block": [st.num_sampled_edges(i, rec) for i in range(3)], "regrows": st.regrows}
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, 3-layer SAGE hidden 256, batch %d, poisson-bandit %s; "
                   "GraphedTrainStep(ledger=True).run, host clock around %d-step windows that end in one device sync"
                   % (cfg["num_nodes"], ix.numel(), cfg["batch"], "/".join(map(str, FAN)), STEPS),
       "steps_per_window": STEPS, "windows_ms_per_step": runs, "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
       "sizes": sizes}
for st, _ in modes.values():
    st.close()
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "poisson_keyed.json")
json.dump(out, open(path, "w"), indent=1)
print(json.dumps({"median_ms_per_step": out["median_ms_per_step"], "sizes": sizes}))
