"""GPU suite (-m gpu): the two Poisson samplers with the keyed draw (``poisson-bandit-keyed`` / ``poisson-ladies-keyed``, DESIGN.md
section 21) inside the train and evaluation steps -- shapes as in tests/test_gpu_live_step.py.  A captured ``GraphedTrainStep``
against eager ``TrainStep`` calls, with and without a batch capacity; the free-running ``run``; ``GraphedEvalStep`` over a ragged
split; ``fit(train_step="graphed")`` against the eager ``fit``; the refusals."""
import math

import pytest
import torch

from test_gpu_eval_step import _loss_bound
from test_gpu_live_step import CAP, CLASSES, F, HIDDEN, LIVE, _bits, _live_batches, _task

pytestmark = pytest.mark.gpu

FAN = [24, 16, 12]
NAMES = ["poisson-bandit-keyed", "poisson-ladies-keyed"]


def _build(cuda, name):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader
    g, tr, va = _task(cuda)
    torch.manual_seed(0)
    model = SAGE(F, HIDDEN, CLASSES, 3, torch.relu, 0.0).to(cuda).bfloat16()
    model.train()
    s = fit.make_sampler(name, FAN)
    assert s.draw == "device" and s._poisson
    s.reset_draw(seed=77)
    return g, s, model, tr, va, BatchLoader(tr, CAP, seed=5).forever()


def _graphed(cuda, name, capacity):
    from bliss_gnn_amd.train import GraphedTrainStep
    g, s, m, tr, va, loader = _build(cuda, name)
    step = GraphedTrainStep(g, s, m, CAP, lr=0.01, ledger=True, batch_capacity=capacity)
    step.calibrate(loader, steps=3)
    step.capture(loader, warmup=2)                                              # three real steps of 64 seeds
    return g, s, m, tr, va, loader, step


def _eager(cuda, name):
    """The eager twin behind the same sampler calls: three for the calibration, three steps of 64 seeds."""
    from bliss_gnn_amd.train import TrainStep
    g, s, m, tr, va, loader = _build(cuda, name)
    step = TrainStep(g, s, m, lr=0.01)
    for _ in range(3):
        s.sample_blocks(g, next(loader))
    for _ in range(3):
        step(next(loader))
    return g, s, m, tr, va, loader, step


def _state_equal(sA, mA, sB, mB):
    for p, q in zip(mA.parameters(), mB.parameters()):
        assert torch.equal(_bits(p), _bits(q))
    assert (getattr(sA, "_w_pos", None) is None) == (getattr(sB, "_w_pos", None) is None)
    if getattr(sA, "_w_pos", None) is not None:
        assert torch.equal(_bits(sA._w_pos), _bits(sB._w_pos))
        assert not bool((sA._w_pos == sA._w_pos.flatten()[0]).all())            # the rows moved
    assert sA.draw_step() == sB.draw_step()


@pytest.mark.parametrize("capacity", [None, CAP])
@pytest.mark.parametrize("name", NAMES)
def test_captured_step_is_the_eager_step(cuda, name, capacity):
    """Loss per step, blocks, parameters, EXP3 rows and the draw step of the eager steps, bit for bit; under a batch capacity of
    64 the one graph is driven with 64, 37, 1 and 64 seeds.  Torch's generator is not touched by either loop."""
    import bliss_gnn_amd as bg
    gA, sA, mA, trA, _, loaderA, step = _graphed(cuda, name, capacity)
    assert sA.draw_step() == 6
    rng0 = torch.get_rng_state()                                                # (the model's initialisation drew from it)
    batches = _live_batches(trA) if capacity else [next(loaderA) for _ in range(4)]
    seen = []
    for seeds in batches:
        loss = float(step(seeds))
        blocks = []
        for blk, c in zip(sA._engine._static[0][0], step.last_counts):          # sampling order
            blocks.append(dict(indptr=blk.indptr[:c.S + 1].clone(), src=blk.src[:c.B].clone(), nid=blk.srcdata[bg.NID][:c.K].clone(),
                               w=_bits(blk._edge_weights[:c.B]).clone()))
        seen.append(dict(loss=loss, sizes=step.sizes(), blocks=blocks))
    rec = step.ledger()
    assert sA.draw_step() == 10 and rec["steps_total"] == 7 and rec["err"] == 0 and rec["nonfinite"] == 0
    assert torch.equal(rng0, torch.get_rng_state())

    gB, sB, mB, trB, _, loaderB, eager = _eager(cuda, name)
    batchesB = _live_batches(trB) if capacity else [next(loaderB) for _ in range(4)]
    for seeds, seedsA, got in zip(batchesB, batches, seen):
        assert torch.equal(seeds, seedsA)
        want = float(eager(seeds))
        print(name, capacity, int(seeds.numel()), got["loss"], want, got["sizes"][0]["K"])
        want_sizes = [dict(S=b._counts.S, E=b._counts.E, C=b._counts.C, K=b._counts.K, B=b._counts.B) for b in eager.last["mfgs"]]
        assert got["sizes"] == want_sizes and got["sizes"][-1]["S"] == int(seeds.numel())
        for ba, bb in zip(got["blocks"], reversed(eager.last["mfgs"])):
            assert torch.equal(ba["indptr"], bb.indptr) and torch.equal(ba["src"], bb.src)
            assert torch.equal(ba["nid"], bb.srcdata[bg.NID]) and torch.equal(ba["w"], _bits(bb.edata["edge_weights"]))
        assert got["loss"] == want and math.isfinite(want)
    _state_equal(sA, mA, sB, mB)
    assert torch.equal(rng0, torch.get_rng_state())                             # the twin's model drew the same numbers, nothing else
    if capacity:
        assert [s["S"] for s in (x["sizes"][-1] for x in seen)] == list(LIVE)
    step.close()


@pytest.mark.parametrize("name", NAMES)
def test_run_is_free_and_equals_the_per_step_calls(cuda, name, monkeypatch):
    """``run(loader, n)``: no generator state is staged, the stream is not synchronised per step, and parameters, EXP3 rows, the
    draw step and the ledger are those of n per-step calls."""
    gA, sA, mA, _, _, loaderA, stepA = _graphed(cuda, name, None)
    gB, sB, mB, _, _, loaderB, stepB = _graphed(cuda, name, None)
    staged, syncs = [], []
    engA = sA._engine
    real_stage = engA.stage_rng_from_torch
    monkeypatch.setattr(engA, "stage_rng_from_torch", lambda: (staged.append(1), real_stage())[1])
    for owner, attr in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.cuda.Event, "synchronize")):
        real = getattr(owner, attr)

        def counted(*a, _real=real, **kw):
            syncs.append(1)
            return _real(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    rng0 = torch.get_rng_state()
    stepA.run(loaderA, 12, poll=4)
    monkeypatch.undo()
    print(name, "stagings", len(staged), "synchronize calls", len(syncs))
    assert staged == [] and len(syncs) <= 2
    losses = [float(stepB(next(loaderB))) for _ in range(12)]
    recA, recB = stepA.ledger(), stepB.ledger()
    assert recA["steps_total"] == recB["steps_total"] == 15 and recA["err"] == 0
    assert recA == recB and all(math.isfinite(x) for x in losses)
    _state_equal(sA, mA, sB, mB)
    assert sA.draw_step() == 6 + 12 and torch.equal(rng0, torch.get_rng_state())
    assert [c.K for c in stepA.last_counts] == [c.K for c in stepB.last_counts]
    stepA.close()
    stepB.close()


def _trained_pair(cuda, name):
    from bliss_gnn_amd.train import TrainStep
    g, s, m, tr, va, loader = _build(cuda, name)
    step = TrainStep(g, s, m, lr=0.01)
    for _ in range(3):
        step(next(loader))
    return g, s, m, va


@pytest.mark.parametrize("name", NAMES)
def test_eval_step_replays_a_ragged_split(cuda, name):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import GraphedEvalStep, _ce_loss
    import metrics_ref
    gA, sA, mA, va = _trained_pair(cuda, name)
    gB, sB, mB, _ = _trained_pair(cuda, name)
    assert va.numel() == 2 * CAP + 37
    es = GraphedEvalStep(gA, sA, mA, CAP, False, batch_capacity=CAP)
    rng0 = torch.get_rng_state()
    for rep in range(2):                                                        # the second pass reuses the graph
        acc_g, loss_g = es.run(va)
        lf, preds, ys, terms = _ce_loss(), [], [], []

        def recording(pred, y):
            loss = lf(pred, y)
            preds.append(pred.float().cpu()); ys.append(y.cpu()); terms.append(float(loss) * pred.shape[0])
            return loss

        acc_e, loss_e = fit.evaluate(gB, sB, mB, va, CAP, False, recording)
        counts = metrics_ref.multiclass_counts(torch.cat(preds), torch.cat(ys))[0]
        print(name, rep, acc_g, acc_e, loss_g, loss_e, es.last_counts, counts)
        assert [p.shape[0] for p in preds] == [CAP, CAP, 37]
        assert es.last_counts == counts and es.last_counts[3] == va.numel() and acc_g == acc_e
        assert abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
        assert sA.draw_step() == sB.draw_step() == 3 + 3 * (rep + 1)
    assert es.fallbacks == 0 and es.replays == 6 and es.captures == 1
    assert torch.equal(rng0, torch.get_rng_state())
    es.close()


def test_fit_graphed_is_fit_eager(cuda):
    """fit(train_step="graphed") against the eager fit for poisson-bandit-keyed, three epochs: every history entry, all parameter
    bits, the EXP3 rows, the draw step and torch's generator."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from test_gpu_fit import _task as fit_task
    out, state = {}, {}
    for kind in ("eager", "graphed"):
        g, tr, va, te = fit_task(cuda)
        g.edata["w"] = bg.normalized_edata(g)
        sampler = fit.make_sampler("poisson-bandit-keyed", [64, 32, 16])
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        torch.manual_seed(11)                                                   # (seed=None: the draw seed is torch.initial_seed())
        out[kind] = fit.fit(g, sampler, model, tr, va, te, batch_size=128, lr=0.01, max_epochs=3, eval_step="graphed",
                            train_metric=True, train_step=kind)
        state[kind] = dict(params=[_bits(q).clone() for q in model.parameters()], rng=torch.get_rng_state(),
                           draw=sampler.draw_step(), exp3=_bits(sampler._w_pos).clone())
    e, gr = out["eager"], out["graphed"]
    print([h["train_loss"] for h in gr["history"]], [h["train_loss"] for h in e["history"]], state["graphed"]["draw"])
    assert len(gr["history"]) == len(e["history"]) == 3 and gr["steps"] == e["steps"]
    for hg, he in zip(gr["history"], e["history"]):
        for k in he:
            assert hg[k] == he[k], (k, hg, he)
    assert gr["best_val_acc"] == e["best_val_acc"] and gr["final"] == e["final"]
    sg, se = state["graphed"], state["eager"]
    assert all(torch.equal(a, b) for a, b in zip(sg["params"], se["params"]))
    assert torch.equal(sg["rng"], se["rng"]) and sg["draw"] == se["draw"] and sg["draw"] > 0
    assert torch.equal(sg["exp3"], se["exp3"]) and not bool((sg["exp3"] == sg["exp3"].flatten()[0]).all())


def test_refusals(cuda):
    from bliss_gnn_amd.train import PipelinedTrainStep
    for name in NAMES:
        g, s, m, tr, va, loader = _build(cuda, name)
        with pytest.raises(NotImplementedError):
            PipelinedTrainStep(g, s, m, CAP)
        seeds = next(loader)
        s.sample_blocks(g, seeds)                                               # binds the engine
        step = s.draw_step()
        for kw in (dict(part="main", external_rng=True), dict(external_rng=True), dict(chain_rng=True)):
            with pytest.raises(NotImplementedError):
                s.sample_blocks_static(g, seeds, **kw)
        with pytest.raises(ValueError):
            s.sample_blocks(g, seeds, uniforms=[torch.zeros(1)] * 3)
        assert s.draw_step() == step
