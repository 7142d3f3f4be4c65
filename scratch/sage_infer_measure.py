"""SAGE full-neighbour inference off the CSC on the Reddit-like graph of bench.py, bench.py's default
3-layer SAGE (602 -> 256 -> 256 -> 41, ReLU, 'mean', transforms="auto": the MFMA path), ``batch_size`` 128:

  passes      one warm pass of each path, then three alternating timed passes of ``inference(path="chunks")`` (the code of before,
              untouched: the baseline in the same process) and ``inference(path="csc")``; a host clock around one ``inference()``
              call that ends in a device sync; ``torch.cuda.max_memory_allocated`` above the resident graph and features.
  csc split   one more pass of the csc path with device events around each ``nn.sage_infer_spmm`` launch, and the row-gather
              rate  edges x dim x 2 B / time  beside the random-row ceiling of DESIGN.md section 8.

"chunks" runs its Linears on library GEMMs and "csc" on the tile kernels, so their outputs differ in the last bits: the largest
difference is reported, not asserted (tests/test_gpu_sage_infer_model.py holds "csc" to "blocks" bit for bit).

Usage: ``python scratch/sage_infer_measure.py [out.json]``."""
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bliss_gnn_amd as bg  # noqa: E402
from bench import chung_lu_graph  # noqa: E402
from bliss_gnn_amd import nn as bnn  # noqa: E402
from bliss_gnn_amd.model import SAGE  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402

BS = 128
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev,
                                     multilabel=cfg["multilabel"], features=cfg.get("features", "normal"), nnz=cfg.get("nnz", 18))
g = bg.Graph(ip, ix, ei, ndata={"features": feats.bfloat16(), "labels": labels})
del feats
torch.manual_seed(1234)
model = SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()
model.train()
V, E = g.num_nodes(), g.num_edges()
g.ndata.pop("h", None)
idle = torch.cuda.memory_allocated()


def one_pass(path):
    g.ndata.pop("h", None)                                    # (the last pass's result is not part of this pass's footprint,
    gc.collect()                                              #  nor are the Blocks of a "chunks" pass, which wait for the collector)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    y = model.inference(g, dev, BS, False, 0, path=path)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, y, (torch.cuda.max_memory_allocated() - idle) / 1e9


def csc_split():
    """One csc pass with events around every message-passing launch (ms, by layer)."""
    inner, spans = bnn.sage_infer_spmm, []

    def timed(indptr, indices, bs, r0, r1, e0, edges, h, out, reduce="mean"):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        inner(indptr, indices, bs, r0, r1, e0, edges, h, out, reduce)
        b.record()
        spans.append((h.shape[1], edges, a, b))
        return out

    bnn.sage_infer_spmm = timed
    try:
        total = one_pass("csc")[0]
    finally:
        bnn.sage_infer_spmm = inner
    layers = []
    for dim, edges, a, b in spans:
        ms = a.elapsed_time(b)
        layers.append({"spmm_dim": dim, "edges": edges, "spmm_ms": ms, "gather_TB_per_s": edges * dim * 2 / (ms * 1e-3) / 1e12})
    return {"pass_ms": total, "spmm_launches": len(spans), "spmm_ms_total": sum(l["spmm_ms"] for l in layers), "launches": layers}


path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sage_infer.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
deg = ip[1:] - ip[:-1]
out = {"workload": "reddit-like Chung-Lu graph |V|=%d |E|=%d (largest in-degree %d), SAGE 602-256-256-41 ReLU mean, transforms=auto, "
                   "batch_size %d; host clock around one inference() call that ends in a device sync" % (V, E, int(deg.max()), BS),
       "random_row_ceiling_TB_per_s": [7.4, 7.9], "idle_memory_GB": idle / 1e9}
warm = {p: one_pass(p) for p in ("chunks", "csc")}
out["warm_pass_ms"] = {p: warm[p][0] for p in warm}
a, b = warm["chunks"][1].float(), warm["csc"][1].float()
out["largest_difference"] = float((a - b).abs().max())
out["largest_magnitude"] = float(a.abs().max())
out["argmax_agreement"] = float((a.argmax(1) == b.argmax(1)).float().mean())
del warm, a, b
print("warm", out["warm_pass_ms"], "largest difference", out["largest_difference"], "of", out["largest_magnitude"], flush=True)
json.dump(out, open(path, "w"), indent=1)
runs, peak = {"chunks": [], "csc": []}, {"chunks": 0.0, "csc": 0.0}
for r in range(3):
    for p in ("chunks", "csc"):
        ms, _, mem = one_pass(p)
        runs[p].append(ms)
        peak[p] = max(peak[p], mem)
        print(p, r, "%.1f ms" % ms, "%.3f GB" % mem, flush=True)
out["pass_ms"] = runs
out["peak_memory_over_idle_GB"] = peak
out["speedup_per_pair"] = [c / s for c, s in zip(runs["chunks"], runs["csc"])]
out["csc_faster_in_every_pair"] = all(s < c for c, s in zip(runs["chunks"], runs["csc"]))
json.dump(out, open(path, "w"), indent=1)
out["csc_split"] = csc_split()
json.dump(out, open(path, "w"), indent=1)
print(json.dumps({k: out[k] for k in ("pass_ms", "speedup_per_pair", "largest_difference", "peak_memory_over_idle_GB", "csc_split")}))
