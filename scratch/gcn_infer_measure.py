"""GCN full-neighbour inference off the CSC on the Reddit-like graph of bench.py, a 3-layer GCN
(602 -> 256 -> 256 -> 41, ReLU) with ``transforms="tile"``, ``batch_size`` 128:

  passes      one warm pass of each path, then N alternating timed passes (default 3) of ``inference(path="blocks")`` (the code of
              before, untouched: the baseline in the same process) and ``inference(path="csc")``; a host clock around one
              ``inference()`` call that ends in a device sync; the outputs are compared bit for bit.
  csc split   one more pass of the csc loop with device events around the source norms and each layer's transform, SpMM and
              finish (aggregate-first product + epilogue), and the SpMM's row-gather rate  edges x dim x 2 B / time  beside the
              random-row ceiling of DESIGN.md section 8.

Usage: ``python scratch/gcn_infer_measure.py [out.json] [blocks passes]``."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bliss_gnn_amd as bg  # noqa: E402
from bench import chung_lu_graph  # noqa: E402
from bliss_gnn_amd.model import GCN  # noqa: E402
from bliss_gnn_amd.nn import gcn_infer_src_norms, gcn_infer_state  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402

BS = 128
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats.bfloat16(), "labels": labels})
torch.manual_seed(1234)
model = GCN(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1, transforms="tile").to(dev).bfloat16()
model.train()
V, E = g.num_nodes(), g.num_edges()
idle = torch.cuda.memory_allocated()


def one_pass(path):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    y = model.inference(g, dev, BS, False, 0, path=path)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, y, (torch.cuda.max_memory_allocated() - idle) / 1e9


def csc_split():
    """The loop of GCN._inference_csc with events around its parts (ms)."""
    model.eval()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    ranges, state = model._csc_ranges(g, BS), gcn_infer_state()
    with torch.no_grad():
        a, b = ev(), ev()
        ns = torch.empty(E, dtype=torch.float32, device=dev)
        a.record()
        for r0, r1, e0, edges in ranges:
            gcn_infer_src_norms(g.indptr, g.indices, BS, r0, r1, e0, edges, ns[e0:e0 + edges], state)
        b.record()
        torch.cuda.synchronize()
        groups = model._csc_groups(ranges)
        out = {"ranges": len(ranges), "max_range_edges": max(r[3] for r in ranges), "spmm_launches_per_layer": len(groups),
               "src_norms_ms": a.elapsed_time(b), "layers": []}
        h = g.ndata["features"]
        for l, layer in enumerate(model.layers):
            t = [ev() for _ in range(4)]
            t[0].record()
            table = layer.infer_transform(h)
            t[1].record()
            agg = torch.empty(V, table.shape[1], dtype=torch.bfloat16, device=dev)
            for r0, r1, e0, edges in groups:
                layer.infer_rows(g, BS, r0, r1, e0, edges, ns[e0:e0 + edges], table, agg[r0:r1])
            t[2].record()
            h = layer.infer_finish(agg)
            t[3].record()
            torch.cuda.synchronize()
            dim, ms = table.shape[1], t[1].elapsed_time(t[2])
            out["layers"].append({"layer": l, "weight_first": layer._in_feats > layer._out_feats, "spmm_dim": dim,
                                  "transform_ms": t[0].elapsed_time(t[1]), "spmm_ms": ms, "finish_ms": t[2].elapsed_time(t[3]),
                                  "gather_TB_per_s": E * dim * 2 / (ms * 1e-3) / 1e12})
    model.train()
    return out


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gcn_infer.json")
n_blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
deg = ip[1:] - ip[:-1]
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d (largest in-degree %d), GCN 602-256-256-41 ReLU, transforms=tile, batch_size %d; "
                   "host clock around one inference() call that ends in a device sync" % (V, E, int(deg.max()), BS),
       "random_row_ceiling_TB_per_s": [7.4, 7.9], "idle_memory_GB": idle / 1e9}
warm = {p: one_pass(p) for p in ("blocks", "csc")}
out["warm_pass_ms"] = {p: warm[p][0] for p in warm}
out["bits_equal"] = bool(torch.equal(warm["blocks"][1], warm["csc"][1]))
print("warm", out["warm_pass_ms"], "bits equal", out["bits_equal"], flush=True)
json.dump(out, open(path, "w"), indent=1)
runs, peak = {"blocks": [], "csc": []}, {"blocks": 0.0, "csc": 0.0}
for r in range(3):
    for p in ("blocks", "csc"):
        if p == "blocks" and r >= n_blocks:
            continue
        ms, _, mem = one_pass(p)
        runs[p].append(ms)
        peak[p] = max(peak[p], mem)
        print(p, r, "%.1f ms" % ms, flush=True)
out["pass_ms"] = runs
out["peak_memory_over_idle_GB"] = peak
out["speedup_per_pair"] = [b / c for b, c in zip(runs["blocks"], runs["csc"])]
out["csc_faster_in_every_pair"] = all(c < b for b, c in zip(runs["blocks"], runs["csc"]))
json.dump(out, open(path, "w"), indent=1)
out["csc_split"] = csc_split()
json.dump(out, open(path, "w"), indent=1)
print(json.dumps({k: out[k] for k in ("pass_ms", "speedup_per_pair", "bits_equal", "peak_memory_over_idle_GB", "csc_split")}))
