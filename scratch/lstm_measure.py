"""Measurement for DESIGN.md section 37 (profiles/lstm_measure.json): k_lstm_agg_fwd / k_lstm_agg_bwd on the two blocks of one
NeighborSampler([25, 10], draw="device") step, batch 1024, on bench.py's Reddit-shaped graph at D = 256, against what a user would
run today on the same block (torch.nn.LSTM in bf16 over destinations bucketed by degree); the cost of one full-fanout
poisson-bandit block; and the largest |kernel - model_f32| per tensor over the asserted cases of tests/test_gpu_lstm_agg.py.

Run from the repository root on the GPU:  python scratch/lstm_measure.py OUT.json"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D = 256


def event_us(fn, launches=20, figures=5):
    """Five figures of 20 launches each, a HIP event pair per launch: microseconds per launch."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(figures):
        pairs = []
        for _ in range(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs.append((a, b))
        torch.cuda.synchronize()
        each.append(round(1000.0 * sum(a.elapsed_time(b) for a, b in pairs) / launches, 2))
    return {"median": statistics.median(each), "each": each}


def prof_us(name, fn, launches=20, figures=5):
    from bliss_gnn_amd import _lib
    import ctypes as C
    L = _lib.lib
    names = [L.bliss_prof_kernel_name(i).decode() for i in range(L.bliss_prof_kernel_count())]
    kid = names.index(name)
    each = []
    for _ in range(figures):
        L.bliss_prof_enable(kid)
        L.bliss_prof_reset()
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        ms, n = C.c_double(), C.c_int64()
        L.bliss_prof_read(kid, C.byref(ms), C.byref(n))
        L.bliss_prof_enable(-2)
        each.append(round(1000.0 * ms.value / max(n.value, 1), 2))
    return {"median": statistics.median(each), "each": each}


def kernel_block(blk, dev, figures=5, launches=20):
    """The two recurrence kernels alone on one block (direct C calls on pre-allocated buffers)."""
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd._engine import _stream
    L = _lib.lib
    S, K, B = blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()
    gen = torch.Generator(device=dev).manual_seed(5)
    lstm = torch.nn.LSTM(D, D, batch_first=True).to(dev).bfloat16()
    h = torch.randn(K, D, generator=gen, device=dev).bfloat16()
    p = torch.nn.functional.linear(h, lstm.weight_ih_l0)
    gout = torch.randn(S, D, generator=gen, device=dev).bfloat16()
    out = torch.empty(S, D, dtype=torch.bfloat16, device=dev)
    gates = torch.empty(B, 4 * D, dtype=torch.float32, device=dev)
    cell = torch.empty(B, D, dtype=torch.float32, device=dev)
    hprev = torch.empty(B, D, dtype=torch.bfloat16, device=dev)
    dgate = torch.empty(B, 4 * D, dtype=torch.bfloat16, device=dev)
    wt = lstm.weight_hh_l0.detach().t().contiguous()
    whh = lstm.weight_hh_l0.detach()
    counts = getattr(blk, "_counts_dev", None) if blk._nnz_ptr else None
    cs, cn = (counts.data_ptr(), counts.data_ptr() + 16) if counts is not None else (0, 0)

    def fwd(save=True):
        _lib.check(L.bliss_lstm_agg_fwd(blk.indptr.data_ptr(), blk.src.data_ptr(), 0, p.data_ptr(), 4 * D, whh.data_ptr(), D,
                                        lstm.bias_ih_l0.data_ptr(), lstm.bias_hh_l0.data_ptr(), S, cs, cn, B, D, out.data_ptr(), D,
                                        gates.data_ptr() if save else 0, cell.data_ptr() if save else 0, hprev.data_ptr() if save else 0,
                                        _stream()), "fwd")

    def bwd():
        _lib.check(L.bliss_lstm_agg_bwd(blk.indptr.data_ptr(), gout.data_ptr(), D, wt.data_ptr(), 4 * D, gates.data_ptr(), cell.data_ptr(), S,
                                        cs, cn, B, D, dgate.data_ptr(), _stream()), "bwd")

    deg = (blk.indptr[1:] - blk.indptr[:-1])
    res = {"n_dst": S, "n_src": K, "edges": B, "max_degree": int(deg.max()), "workgroups": (S + 31) // 32,
           "saved_bytes": 22 * D * B,
           "fwd_train_us": event_us(fwd, launches, figures), "fwd_infer_us": event_us(lambda: fwd(False), launches, figures),
           "bwd_us": event_us(bwd, launches, figures),
           "prof_fwd_train_us": prof_us("k_lstm_agg_fwd", fwd, launches, figures), "prof_bwd_us": prof_us("k_lstm_agg_bwd", bwd, launches, figures)}
    return res, (lstm, h, gout, deg)


def baseline_block(blk, lstm, h, gout, deg):
    """torch.nn.LSTM in bf16 over the destinations bucketed by degree: forward, and forward + backward."""
    src = blk.src.long()
    buckets = []
    for d in torch.unique(deg).tolist():
        if d == 0:
            continue
        rows = torch.nonzero(deg == d).flatten()
        e = (blk.indptr[rows].long().unsqueeze(1) + torch.arange(d, device=h.device).unsqueeze(0)).reshape(-1)
        buckets.append((rows, src[e], d))
    hh = h.clone().requires_grad_()

    def fwd():
        out = torch.zeros(blk.num_dst_nodes(), D, dtype=h.dtype, device=h.device)
        for rows, s, d in buckets:
            out = out.index_copy(0, rows, lstm(hh[s].view(rows.numel(), d, D))[1][0][0])
        return out

    def both():
        lstm.zero_grad()
        hh.grad = None
        fwd().backward(gout)

    try:
        with torch.no_grad():
            f = event_us(fwd, 5, 3)
        fb = event_us(both, 5, 3)
        return {"buckets": len(buckets), "fwd_us": f, "fwd_bwd_us": fb}
    except Exception as exc:                                     # (the library may have no bf16 LSTM here)
        return {"not_taken": repr(exc)[:300]}


def model_diff(dev):
    """max |kernel - model_f32| per tensor over the asserted cases (the fp32 sum order, the fast exponentials, the flips they cause)."""
    import bounds
    import lstm_agg_ref as ref
    import test_gpu_lstm_agg as tg
    worst = {}
    for name, degs in tg.CASES.items():
        if not ref.asserted(degs):
            continue
        for dim in ref.DIMS:
            for weighted in (False, True):
                spec, inp, gout, _t, _c = tg._case(name, dim, weighted)
                raw = tg._run(dev, bounds.to_block(spec, dev), spec, inp, gout, dim)
                model = ref.model_f32(spec, inp, gout)
                for k, v in raw.items():
                    worst[k] = max(worst.get(k, 0.0), ref.max_err(v.double().cpu(), model[k]))
    return worst


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "lstm_measure.json"
    import bliss_gnn_amd as bg
    from bench import chung_lu_graph
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.synth import CONFIGS, node_data
    dev = torch.device("cuda", 0)
    res = {"what": "k_lstm_agg_fwd / k_lstm_agg_bwd at D = 256 on the two blocks of one NeighborSampler([25, 10], draw='device') step, batch "
                   "1024, bench.py's Reddit-shaped graph; baseline torch.nn.LSTM (bf16) over destinations bucketed by degree on the same "
                   "blocks; one full-fanout poisson-bandit block; max |kernel - model_f32| over the asserted test cases",
           "method": "HIP event pair around every launch, 20 launches per figure, 5 figures (baseline: 5 launches, 3 figures); prof_*: the "
                     "in-tree profiler over launches of its own",
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per launch", "dim": D}
    res["max_abs_kernel_minus_model_f32"] = model_diff(dev)
    json.dump(res, open(out_path, "w"), indent=1)
    cfg = CONFIGS["reddit"]
    ip, ix, ei = chung_lu_graph(cfg["num_nodes"], cfg["num_edges"], seed=0, device=dev)
    feats, labels, train_nid = node_data(cfg["num_nodes"], 8, cfg["classes"], cfg["n_train"], seed=1, device=dev)
    g = bg.Graph(ip, ix, ei, ndata={"features": feats, "labels": labels})
    seeds = train_nid[:1024].to(torch.int32)
    _, _, mfgs = fit.NeighborSampler([25, 10], draw="device").sample_blocks(g, seeds)
    res["neighbor_blocks"] = []
    for blk in mfgs:
        r, (lstm, h, gout, deg) = kernel_block(blk, dev)
        r["baseline_nn_lstm"] = baseline_block(blk, lstm, h, gout, deg)
        res["neighbor_blocks"].append(r)
        json.dump(res, open(out_path, "w"), indent=1)
    g.edata["w"] = bg.normalized_edata(g)
    _, _, mfgs = fit.make_sampler("poisson-bandit", cfg["fanouts"]).sample_blocks(g, train_nid[:256].to(torch.int32))
    r, _ = kernel_block(mfgs[0], dev, figures=3, launches=3)
    res["poisson_bandit_block"] = r
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
