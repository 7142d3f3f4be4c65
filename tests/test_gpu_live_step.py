"""GPU suite (-m gpu): the train and evaluation steps under a batch capacity.  One captured
``GraphedTrainStep(batch_capacity=64)`` driven with 64, 37, 1 and 64 live seeds against eager ``TrainStep`` calls on the same seeds;
``GraphedEvalStep(batch_capacity=64)`` over a ragged split against ``fit.evaluate``; the refusals."""
import math

import pytest
import torch

import batch_stats_ref as ref
from test_gpu_eval_step import _loss_bound

pytestmark = pytest.mark.gpu

V, E, F, CLASSES, CAP, HIDDEN = 600, 7000, 24, 4, 64, 32
SAMPLERS = {"labor": [5, 5, 5], "poisson-bandit": [24, 16, 12]}
LIVE = (64, 37, 1, 64)


def _task(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, F, generator=gen).bfloat16()
    labels = (feats.float() @ torch.randn(F, CLASSES, generator=gen)).argmax(1)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    perm = torch.randperm(V, generator=gen).to(torch.int32).to(cuda)
    return g, perm[:400], perm[400:400 + 2 * CAP + 37]


def _build(cuda, name):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader
    g, tr, va = _task(cuda)
    torch.manual_seed(0)
    model = SAGE(F, HIDDEN, CLASSES, 3, torch.relu, 0.0).to(cuda).bfloat16()
    model.train()
    return g, fit.make_sampler(name, SAMPLERS[name]), model, tr, va, BatchLoader(tr, CAP, seed=5).forever()


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


def _live_batches(tr):
    """The four batches of the test, of 64, 37, 1 and 64 seeds: slices of one permutation, so no seed repeats inside a batch."""
    perm = tr[torch.randperm(tr.numel(), generator=torch.Generator().manual_seed(9)).to(tr.device)]
    out, o = [], 0
    for n in LIVE:
        out.append(perm[o:o + n].clone())
        o += n
    return out


def _graphed(cuda, name, **kw):
    from bliss_gnn_amd.train import GraphedTrainStep
    g, s, m, tr, va, loader = _build(cuda, name)
    step = GraphedTrainStep(g, s, m, CAP, lr=0.01, ledger=True, batch_capacity=CAP, **kw)
    torch.manual_seed(3)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)                                              # three real steps of 64 seeds
    return g, s, m, tr, va, loader, step


def _eager(cuda, name, **kw):
    """The eager twin behind the same sampler calls: three for the calibration, three steps of 64 seeds."""
    from bliss_gnn_amd.train import TrainStep
    g, s, m, tr, va, loader = _build(cuda, name)
    step = TrainStep(g, s, m, lr=0.01, **kw)
    torch.manual_seed(3)
    for _ in range(3):
        s.sample_blocks(g, next(loader))
    ks = []
    for _ in range(3):
        step(next(loader))
        ks.append(step.last["mfgs"][0].num_src_nodes())
    return g, s, m, tr, va, step, ks


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_one_captured_step_serves_every_batch_size(cuda, name):
    """Blocks, loss per step, parameters, train_acc counts, the ledger's size averages and the batch statistics: those of the eager
    steps, bit for bit (no kernel's per-row result depends on the row capacity; the weight-gradient chunks of 64 rows start at the
    same rows under either bound).  The graphed run first, then its eager twin from the same generator state."""
    import bliss_gnn_amd as bg
    L = 3
    gA, sA, mA, trA, _, _, step = _graphed(cuda, name, train_metric=True)
    step.last_batch_counts()
    seen = []
    for seeds in _live_batches(trA):
        loss = float(step(seeds))
        blocks = []
        for blk, c in zip(sA._engine._static[0][0], step.last_counts):                      # sampling order
            blocks.append(dict(indptr=blk.indptr[:c.S + 1].clone(), src=blk.src[:c.B].clone(), dst=blk.dst[:c.B].clone(),
                               nid=blk.srcdata[bg.NID][:c.K].clone(), eid=blk.edata[bg.EID][:c.B].clone(),
                               w=_bits(blk._edge_weights[:c.B]).clone()))
        seen.append(dict(loss=loss, sizes=step.sizes(), blocks=blocks, counts=step.last_batch_counts()))
    rec = step.ledger()
    stats = step.batch_stats()
    rng_a = torch.get_rng_state()
    draw_a = sA.draw_step() if hasattr(sA, "draw_step") and getattr(sA, "draw", "host") == "device" else None

    gB, sB, mB, trB, _, eager, ks = _eager(cuda, name, train_metric=True)
    assert torch.equal(trA, trB)
    eager.last_batch_counts()
    for i, (seeds, got) in enumerate(zip(_live_batches(trB), seen)):
        n = int(seeds.numel())
        want = float(eager(seeds))
        ks.append(eager.last["mfgs"][0].num_src_nodes())
        print(name, n, got["loss"], want, got["sizes"][0]["K"], ks[-1])
        want_sizes = [dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in eager.last["mfgs"]]
        assert got["sizes"] == want_sizes and got["sizes"][-1]["S"] == n, (n, got["sizes"], want_sizes)
        for ba, bb in zip(got["blocks"], reversed(eager.last["mfgs"])):
            assert torch.equal(ba["indptr"], bb.indptr) and torch.equal(ba["src"], bb.src) and torch.equal(ba["dst"], bb.dst)
            assert torch.equal(ba["nid"], bb.srcdata[bg.NID]) and torch.equal(ba["eid"], bb.edata[bg.EID])
            assert torch.equal(ba["w"], _bits(bb.edata["edge_weights"]))
        assert got["loss"] == want and math.isfinite(want), (i, n, got["loss"], want)
        assert got["counts"] == eager.last_batch_counts() and got["counts"][3] == n
    for p, q in zip(mA.parameters(), mB.parameters()):
        assert torch.equal(_bits(p), _bits(q))
    if getattr(sA, "_w_pos", None) is not None:
        assert torch.equal(_bits(sA._w_pos), _bits(sB._w_pos))
    assert torch.equal(rng_a, torch.get_rng_state())
    if draw_a is not None:
        assert draw_a == sB.draw_step()
    assert rec["steps_total"] == 7 and rec["err"] == 0 and rec["nonfinite"] == 0
    assert [step.num_sampled_nodes(i, rec) for i in range(L + 1)] == [eager.num_sampled_nodes(i) for i in range(L + 1)]
    assert [step.num_sampled_edges(i, rec) for i in range(L)] == [eager.num_sampled_edges(i) for i in range(L)]
    cum_out = 0.0
    for s_out in (CAP, CAP, CAP) + LIVE:
        cum_out = cum_out * 0.99 + s_out
    assert rec["cum_out"] == cum_out                                            # the live sizes, not the capacity
    want = ref.BatchStats()
    for k in ks:
        want.push(k)
    assert len(ks) == 7 and stats == dict(n=7, m=want.m, s=want.s) == step.batch_stats(rec)
    step.clear_batch_stats()
    assert step.batch_stats() == dict(n=0, m=0.0, s=0.0)
    step.close()


def test_stale_capacity_rows_reach_no_parameter(cuda, monkeypatch):
    """Every floating-point device buffer the step allocates -- the activations, their gradients, the logits -- is filled with NaN
    before the kernels write it, in the warm-up steps and (recorded) in every replay: rows past the live count then hold NaN,
    and a parameter or a loss that had read one would be NaN."""
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)
    g, s, m, tr, _, _, step = _graphed(cuda, "labor")
    losses = [float(step(seeds)) for seeds in _live_batches(tr)]
    monkeypatch.undo()
    gB, sB, mB, trB, _, eager, _ = _eager(cuda, "labor")
    want = [float(eager(seeds)) for seeds in _live_batches(trB)]
    print(losses, want)
    assert all(math.isfinite(x) for x in losses) and losses == want
    for p, q in zip(m.parameters(), mB.parameters()):
        assert bool(torch.isfinite(p.float()).all()) and torch.equal(_bits(p), _bits(q))
    step.close()


def test_sizes_outside_the_capacity_are_refused_before_anything_is_enqueued(cuda):
    g, s, m, tr, _, _, step = _graphed(cuda, "labor")
    draw, seeds0, params = s.draw_step(), step.seeds.clone(), [_bits(p).clone() for p in m.parameters()]
    for bad in (tr[:0], tr[:CAP + 1]):
        with pytest.raises(ValueError, match="1 .. 64"):
            step(bad)
    with pytest.raises(ValueError, match="1 .. 64"):
        step.run(iter([tr[:CAP + 1]]), 1)
    torch.cuda.synchronize()
    assert s.draw_step() == draw and torch.equal(step.seeds, seeds0) and int(step.n_live) == CAP
    assert all(torch.equal(_bits(p), q) for p, q in zip(m.parameters(), params))
    step.close()


def test_run_follows_the_loaders_batch_size_without_a_recapture(cuda):
    """``run`` over a loader whose batch size changes: one capture, the ledger's output-size average follows."""
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    g, s, m, tr, va, _ = _build(cuda, "labor")
    step = GraphedTrainStep(g, s, m, 32, lr=0.01, ledger=True, batch_capacity=CAP)
    step.calibrate(BatchLoader(tr, CAP, seed=5).forever(), steps=3)
    captures, real = [], step._capture_graph
    step._capture_graph = lambda loader: (captures.append(1), real(loader))[1]
    loader = BatchLoader(tr, 32, seed=5)
    step.run(iter(loader), len(loader))                                         # 12 steps of 32
    loader.set_batch_size(50)
    it = iter(loader)
    step.run(it, len(loader))                                                   # 8 steps of 50
    rec = step.ledger()
    cum = 0.0
    for s_out in [32] * 12 + [50] * 8:
        cum = cum * 0.99 + s_out
    assert rec["steps_total"] == 20 and rec["cum_out"] == cum and rec["err"] == 0 and rec["batch_stats"]["n"] == 20
    assert captures == [1] and step.regrows == 0 and step.sizes()[-1]["S"] == 50
    step.close()


def _trained_pair(cuda, name):
    from bliss_gnn_amd.train import BatchLoader, TrainStep
    g, s, m, tr, va, loader = _build(cuda, name)
    step = TrainStep(g, s, m, lr=0.01)
    torch.manual_seed(5)                                                        # (the Poisson samplers draw from torch's generator)
    for _ in range(3):
        step(next(loader))
    return g, s, m, va


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_ragged_split_is_replayed_whole(cuda, name):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import GraphedEvalStep, _ce_loss
    import metrics_ref
    gA, sA, mA, va = _trained_pair(cuda, name)
    gB, sB, mB, _ = _trained_pair(cuda, name)
    assert va.numel() == 2 * CAP + 37
    es = GraphedEvalStep(gA, sA, mA, CAP, False, batch_capacity=CAP)
    for rep in range(2):                                                        # the second pass reuses the graph
        torch.manual_seed(7 + rep)
        acc_g, loss_g = es.run(va)
        rng_g = torch.get_rng_state()
        lf, preds, ys, terms = _ce_loss(), [], [], []

        def recording(pred, y):
            loss = lf(pred, y)
            preds.append(pred.float().cpu()); ys.append(y.cpu()); terms.append(float(loss) * pred.shape[0])
            return loss

        torch.manual_seed(7 + rep)
        acc_e, loss_e = fit.evaluate(gB, sB, mB, va, CAP, False, recording)
        counts = metrics_ref.multiclass_counts(torch.cat(preds), torch.cat(ys))[0]
        print(name, rep, acc_g, acc_e, loss_g, loss_e, es.last_counts, counts)
        assert [p.shape[0] for p in preds] == [CAP, CAP, 37]
        assert es.last_counts == counts and es.last_counts[3] == va.numel() and acc_g == acc_e
        assert abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
        assert torch.equal(rng_g, torch.get_rng_state())
        if hasattr(sA, "draw_step"):
            assert sA.draw_step() == sB.draw_step()
    assert es.fallbacks == 0 and es.replays == 6 and es.captures == 1           # every batch, the ragged ones too, went through replay
    es.set_batch_size(40)                                                       # 40 40 40 40 5: the same graph
    torch.manual_seed(1)
    acc_g, _ = es.run(va)
    torch.manual_seed(1)
    acc_e, _ = fit.evaluate(gB, sB, mB, va, 40, False, _ce_loss())
    assert acc_g == acc_e and es.replays == 11 and es.captures == 1 and es.fallbacks == 0
    with pytest.raises(ValueError):
        es.set_batch_size(CAP + 1)
    es.close()


def test_refusals(cuda, monkeypatch):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import GATv2, GCN, SAGE
    from bliss_gnn_amd.train import GraphedEvalStep, GraphedTrainStep, PipelinedTrainStep
    g, s, m, tr, va, _ = _build(cuda, "poisson-bandit")
    with pytest.raises(NotImplementedError, match="batch_capacity"):
        PipelinedTrainStep(g, s, m, CAP, batch_capacity=CAP)
    with pytest.raises(NotImplementedError, match="batch_capacity"):
        GraphedTrainStep(g, s, m, CAP, distributed=True, batch_capacity=CAP)
    with pytest.raises(ValueError):
        GraphedTrainStep(g, s, m, CAP, batch_capacity=CAP - 1)
    gat = GATv2(2, F, 8, CLASSES, [2, 1], torch.relu, 0.0, 0.0, 0.2, False).to(cuda).bfloat16()
    gcn = GCN(F, HIDDEN, CLASSES, 2, torch.relu, 0.0).to(cuda).bfloat16()
    for model, word in ((gat, "GATv2"), (gcn, "GCN")):
        with pytest.raises(NotImplementedError, match=word):
            GraphedTrainStep(g, s, model, CAP, batch_capacity=CAP)
        with pytest.raises(NotImplementedError, match=word):
            GraphedEvalStep(g, s, model, CAP, batch_capacity=CAP)
    monkeypatch.setenv("BLISS_SAGE_MFMA", "0")                                  # SAGE's library-GEMM path
    with pytest.raises(NotImplementedError, match="MFMA"):
        GraphedTrainStep(g, s, m, CAP, batch_capacity=CAP)
    monkeypatch.undo()
    fp32 = SAGE(F, HIDDEN, CLASSES, 3, torch.relu, 0.0).to(cuda)
    with pytest.raises(NotImplementedError, match="MFMA"):
        GraphedTrainStep(g, s, fp32, CAP, batch_capacity=CAP)
    es = GraphedEvalStep(g, s, m, CAP)
    with pytest.raises(RuntimeError):
        es.set_batch_size(32)                                                   # no capacity: captured for one size
