"""GATv2 full-neighbour inference off the CSC on the Reddit-like graph of bench.py, the GATv2 of config 4
(heads 4/4/1, hidden 256, ELU, no residual) with ``transforms="tile"``:

  passes      one warm pass of each path, then three alternating timed passes of ``inference(path="blocks")`` (the code of before,
              untouched: the baseline in the same process) and ``inference(path="csc")``; the outputs are compared bit for bit.
  csc split   one more pass of the csc loop with device events around each layer's transforms, message passing and glue, and the
              message passing's gather rate  row gathers x H*D x 2 B / time  (a row of more than 64 in-edges is gathered twice
              but for the last chunk of each 256-edge segment) beside the random-row ceiling of DESIGN.md section 8.

Usage: ``python scratch/gat_infer_measure.py [out.json]``."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bliss_gnn_amd as bg  # noqa: E402
from bench import chung_lu_graph  # noqa: E402
from bliss_gnn_amd.model import GATv2  # noqa: E402
from bliss_gnn_amd.nn import gat_glue, gat_infer_state  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402

dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats.bfloat16(), "labels": labels})
torch.manual_seed(1234)
model = GATv2(3, cfg["feat"], 256, cfg["classes"], [4, 4, 1], torch.nn.functional.elu, 0.1, 0.1, 0.2, False, transforms="tile").to(dev).bfloat16()
V, E = g.num_nodes(), g.num_edges()


def one_pass(path):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = model.inference(g, dev, 128, False, 0, path=path)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, y


def row_gathers():
    """Feature rows the message passing fetches over the whole graph: every edge once, and once more unless it lies in the last
    64-edge chunk of its 256-edge segment."""
    deg = ip[1:] - ip[:-1]
    full, rest = deg // 256, deg % 256
    again = full * 192 + torch.where(rest > 0, (rest + 63) // 64 - 1, torch.zeros_like(rest)) * 64
    return int(deg.sum()) + int(again.sum())


def csc_split():
    """The loop of GATv2._inference_csc with events around its three parts (ms per layer)."""
    model.eval()
    ranges, state = model._csc_ranges(g, 4096), gat_infer_state(dev)
    h, n, rows_out = g.ndata["features"], len(model.gatv2_layers), []
    ev = lambda: torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for l, layer in enumerate(model.gatv2_layers):
            H, D, last = layer._num_heads, layer._out_feats, l == n - 1
            t = [ev() for _ in range(3)]
            t[0].record()
            feat_src, res = layer.infer_transform(h)
            t[1].record()
            flat = torch.empty(V, H * D, dtype=torch.bfloat16, device=dev)
            for r0, r1, edges in ranges:
                layer.infer_rows(g, r0, r1, edges, feat_src, res, flat[r0:r1], state)
            t[2].record()
            glue_ms = 0.0
            if last:
                a, b = ev(), ev()
                a.record()
                flat = gat_glue(flat, None, H, D, head_mean=True)[0]
                b.record()
                torch.cuda.synchronize()
                glue_ms = a.elapsed_time(b)
            torch.cuda.synchronize()
            mp_ms = t[1].elapsed_time(t[2])
            rows_out.append({"layer": l, "heads": H, "head_dim": D, "transform_ms": t[0].elapsed_time(t[1]), "message_passing_ms": mp_ms,
                             "glue_ms": glue_ms, "gather_TB_per_s": gathers * H * D * 2 / (mp_ms * 1e-3) / 1e12})
            h = flat
    model.train()
    assert int(state["err"].item()) == 0
    return {"ranges": len(ranges), "max_range_edges": max(r[2] for r in ranges), "layers": rows_out}


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gat_infer.json")
gathers = row_gathers()
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d, GATv2 heads 4/4/1 hidden 256 ELU no residual, transforms=tile; host clock "
                   "around one inference() call that ends in a device sync" % (V, E),
       "row_gathers": gathers, "gathers_per_edge": gathers / E, "random_row_ceiling_TB_per_s": [7.4, 7.9]}
warm = {p: one_pass(p) for p in ("blocks", "csc")}
out["warm_pass_ms"] = {p: warm[p][0] for p in warm}
out["bits_equal"] = bool(torch.equal(warm["blocks"][1], warm["csc"][1]))
runs = {"blocks": [], "csc": []}
for r in range(3):
    for p in ("blocks", "csc"):
        runs[p].append(one_pass(p)[0])
        print(p, r, "%.1f ms" % runs[p][-1], flush=True)
out["pass_ms"] = runs
out["speedup_per_pair"] = [b / c for b, c in zip(runs["blocks"], runs["csc"])]
out["csc_faster_in_every_pair"] = all(c < b for b, c in zip(runs["blocks"], runs["csc"]))
json.dump(out, open(path, "w"), indent=1)
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
one_pass("csc")
out["csc_peak_extra_memory_GB"] = (torch.cuda.max_memory_allocated() - base) / 1e9
out["csc_split"] = csc_split()
json.dump(out, open(path, "w"), indent=1)
print(json.dumps({k: out[k] for k in ("pass_ms", "speedup_per_pair", "bits_equal", "csc_split")}))
