"""The live batch size on the Reddit-like graph of bench.py, 3-layer SAGE hidden 256, batch 256:

  (a) overhead    GraphedTrainStep(ledger=True).run with LABOR-0 15/10/5: static at 256 seeds against batch_capacity=512 with 256
                  live.  Three alternating windows of 200 steps in one process, medians.  The price of the feature's own switch.
  (b) equal budget  fit(train_step="graphed", vertex_limit=V) for labor, neighbor (draw="device") and poisson-bandit, V = LABOR-0's
                  measured input-layer K at batch 256, epochs of about 40 steps: the batch size each sampler settles at, its input
                  K there, and ms/step of a captured step at that size (three windows of 100 steps, median).

Usage: ``python scratch/live_batch_measure.py [out.json]``."""
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

BS, CAP, EPOCH_STEPS, EPOCHS = 256, 512, 40, 5
SAMPLERS = (("labor", [15, 10, 5], {}), ("neighbor", [15, 10, 5], dict(draw="device")), ("poisson-bandit", [4096, 2048, 1024], {}))
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
g.edata["w"] = bg.normalized_edata(g)


def model_():
    torch.manual_seed(1234)
    m = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
    m.train()
    return m


def step_(name, fan, kw, bs, capacity):
    s = fit.make_sampler(name, fan, **kw)
    step = GraphedTrainStep(g, s, model_(), bs, multilabel=cfg["multilabel"], ledger=True, batch_capacity=capacity)
    step.calibrate(BatchLoader(train_nid, capacity or bs, seed=2).forever(), steps=8)
    loader = BatchLoader(train_nid, bs, seed=2).forever()
    step.run(loader, 10)                                         # captures; warm
    return step, loader


def timed(step, loader, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step.run(loader, n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def overhead():
    modes = {"static_256": step_("labor", [15, 10, 5], {}, BS, None), "capacity_512_live_256": step_("labor", [15, 10, 5], {}, BS, CAP)}
    runs = {k: [] for k in modes}
    for r in range(3):
        for k, (step, loader) in modes.items():
            runs[k].append(timed(step, loader, 200))
            print("overhead", k, r, "%.3f ms/step" % runs[k][-1], flush=True)
    out = {"sampler": "labor", "fanouts": [15, 10, 5], "steps_per_window": 200, "windows_ms_per_step": runs,
           "median_ms_per_step": {k: statistics.median(v) for k, v in runs.items()},
           "regrows": {k: st.regrows for k, (st, _) in modes.items()}}
    for st, _ in modes.values():
        st.close()
    return out


def labor_k():
    s = fit.make_sampler("labor", [15, 10, 5])
    loader = BatchLoader(train_nid, BS, seed=2).forever()
    ks = [s.sample_blocks(g, next(loader))[2][0].num_src_nodes() for _ in range(20)]
    return sum(ks) / len(ks)


def equal_budget(limit):
    rows = []
    tr, va = train_nid[:EPOCH_STEPS * BS], train_nid[EPOCH_STEPS * BS:EPOCH_STEPS * BS + BS]
    for name, fan, kw in SAMPLERS:
        s = fit.make_sampler(name, fan, **kw)
        out = fit.fit(g, s, model_(), tr, va, None, batch_size=BS, max_epochs=EPOCHS, multilabel=cfg["multilabel"], train_step="graphed",
                      vertex_limit=limit, batch_capacity=CAP, seed=2)
        hist = out["history"]
        settled = hist[-1]["batch_size"]
        step, loader = step_(name, fan, kw, settled, CAP)
        ms = [timed(step, loader, 100) for _ in range(3)]
        k_there = step.batch_stats()["m"]
        step.close()
        rows.append({"sampler": name, "fanouts": fan, "batch_size_per_epoch": [h["batch_size"] for h in hist],
                     "clamped_per_epoch": [h["batch_size_clamped"] for h in hist],
                     "input_K_per_epoch": [h["input_nodes"]["m"] for h in hist], "settled_batch_size": settled,
                     "input_K_at_settled": k_there, "windows_ms_per_step": ms, "median_ms_per_step": statistics.median(ms),
                     "ms_per_1000_seeds": statistics.median(ms) * 1000.0 / settled})
        print("equal budget", json.dumps(rows[-1]), flush=True)
    return rows


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "live_batch.json")
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, 3-layer SAGE hidden 256, batch %d, capacity %d; host clock around windows of "
                   "free-running / per-step replays that end in one device sync" % (cfg["num_nodes"], ix.numel(), BS, CAP)}
out["overhead"] = overhead()
json.dump(out, open(path, "w"), indent=1)
limit = int(labor_k())
out["vertex_limit"] = limit
out["equal_budget"] = equal_budget(limit)
json.dump(out, open(path, "w"), indent=1)
print(json.dumps({"overhead": out["overhead"]["median_ms_per_step"], "vertex_limit": limit,
                  "equal_budget": [{k: r[k] for k in ("sampler", "settled_batch_size", "input_K_at_settled", "median_ms_per_step")}
                                   for r in out["equal_budget"]]}))
