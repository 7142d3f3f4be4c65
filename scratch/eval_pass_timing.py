"""Timing behind DESIGN.md section 14 and profiles/r05_a_eval_pass_timing.json: one validation pass of the Reddit-like bench.py
graph (batch 256, a 20 K-node split) through fit.evaluate and through train.GraphedEvalStep, and the GraphedTrainStep with and
without train_acc.  One warm pass, then three alternating timed passes; a host clock around work that ends in a device
synchronise.  ROOT is the checkout whose package is measured (a checkout of the parent commit has no GraphedEvalStep and times
the eager pass only), so two commits are compared by alternating processes.

usage: python scratch/eval_pass_timing.py ROOT eval|train OUT.json"""
import json
import statistics
import sys
import time

import os
root, what, out = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3]
sys.path[:] = [p for p in sys.path if p not in ("", ".", os.getcwd())]
sys.path.insert(0, root)
import torch  # noqa: E402

import bench  # noqa: E402  (ROOT's bench.py: only its graph generator)
import bliss_gnn_amd as bg  # noqa: E402
from bliss_gnn_amd import fit  # noqa: E402
from bliss_gnn_amd.model import SAGE  # noqa: E402
from bliss_gnn_amd.synth import CONFIGS, node_data  # noqa: E402
from bliss_gnn_amd.train import BatchLoader, TrainStep  # noqa: E402

assert bg.__file__.startswith(root), (bg.__file__, root)
dev = torch.device("cuda", 0)
cfg = CONFIGS["reddit"]
ip, ix, ei = bench.chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
feats, labels, train_nid = node_data(cfg["num_nodes"], cfg["feat"], cfg["classes"], cfg["n_train"], seed=1, device=dev)
g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
g.edata["w"] = bg.normalized_edata(g)
val = torch.randperm(cfg["num_nodes"], generator=torch.Generator().manual_seed(4))[:20000].to(torch.int32).to(dev)
fan, BS = cfg["fanouts"], cfg["batch"]


def sampler():
    return bg.PoissonBanditLadiesSampler(fan, importance_sampling=1, node_embedding="features", num_steps=3000, eta=0.1, model="sage")


def model():
    torch.manual_seed(1234)
    return SAGE(cfg["feat"], 256, cfg["classes"], 3, torch.relu, 0.1).to(dev).bfloat16()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


res = {"root": root, "what": what}
if what == "eval":
    m = model()
    s_e = sampler()
    step = TrainStep(g, s_e, m, lr=0.002)
    loader = BatchLoader(train_nid, BS, seed=2).forever()
    torch.manual_seed(3)
    for _ in range(5):
        step(next(loader))
    eager = lambda: fit.evaluate(g, s_e, m, val, BS, False, step.loss_fn)
    modes = {"eager": eager}
    if hasattr(__import__("bliss_gnn_amd.train", fromlist=["x"]), "GraphedEvalStep"):
        from bliss_gnn_amd.train import GraphedEvalStep
        s_g = sampler()
        s_g.sample_blocks(g, val[:BS])                     # (binds the engine, creates the rows)
        s_g._w_pos.copy_(s_e._w_pos); s_g._row_sum.copy_(s_e._row_sum)
        es = GraphedEvalStep(g, s_g, m, BS)
        modes["graphed"] = lambda: es.run(val)
    vals = {}
    for k, fn in modes.items():                            # warm: every shape, the calibration, the capture
        torch.manual_seed(9)
        vals[k] = timed(fn)
    res["warm"] = {k: v[0] for k, v in vals.items()}
    res["values"] = {k: v[1] for k, v in vals.items()}
    times = {k: [] for k in modes}
    for rep in range(3):                                   # alternating
        for k, fn in modes.items():
            torch.manual_seed(10 + rep)
            times[k].append(timed(fn)[0])
    res["ms"] = times
    res["median_ms"] = {k: statistics.median(v) for k, v in times.items()}
    if "graphed" in modes:
        res["fallbacks"], res["captures"] = es.fallbacks, es.captures
else:
    from bliss_gnn_amd.train import GraphedTrainStep
    steps = {}
    for tm in (False, True):
        s = sampler()
        st = GraphedTrainStep(g, s, model(), BS, lr=0.002, train_metric=tm)
        ld = BatchLoader(train_nid, BS, seed=2).forever()
        torch.manual_seed(3)
        st.calibrate(ld, steps=8)
        st.capture(ld, warmup=2)
        for _ in range(50):
            st(next(ld))
        steps[tm] = (st, ld)
    times = {False: [], True: []}
    N = 500
    for rep in range(3):
        for tm in (False, True):
            st, ld = steps[tm]

            def window():
                for _ in range(N):
                    st(next(ld))
            times[tm].append(timed(window)[0] / N)
    res["ms_per_step"] = {"train_metric=%s" % k: v for k, v in times.items()}
    res["median_ms_per_step"] = {"train_metric=%s" % k: statistics.median(v) for k, v in times.items()}
    res["train_acc"] = steps[True][0].train_acc.compute()
print(json.dumps(res))
json.dump(res, open(out, "w"), indent=1)
