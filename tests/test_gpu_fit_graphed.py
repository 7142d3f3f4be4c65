"""GPU suite (-m gpu): ``fit(train_step="graphed")`` and ``GraphedTrainStep.run`` on the small task of
tests/test_gpu_fit.py -- the replayed loop computes the eager loop's bits, the free-running loop does not sync per step, the
regrow keeps the plain loop's batches and random streams, an error word stops the enqueueing, and ``ledger=False`` is the step
as it was."""
import pytest
import torch

from test_gpu_fit import _task

pytestmark = pytest.mark.gpu

BS = 128
SAMPLERS = {"poisson-bandit": ([64, 32, 16], {}, "eager"), "labor": ([5, 5, 5], {}, "eager"), "neighbor-exp3": ([5, 5, 5], {}, "eager"),
            "bandit-device": ([64, 32, 16], dict(draw="device"), "graphed")}


def _setup(cuda, name, p):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    fan, kw, _ = SAMPLERS[name]
    g, tr, va, te = _task(cuda)
    g.edata["w"] = bg.normalized_edata(g)
    sampler = fit.make_sampler(name.replace("-device", ""), fan, **kw)
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, p).to(cuda).bfloat16()
    return g, sampler, model, tr, va, te


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_fit_graphed_is_fit_eager_bit_for_bit(cuda, name, p, monkeypatch):
    from bliss_gnn_amd import fit
    eval_step = SAMPLERS[name][2]
    out, state, sizes = {}, {}, []
    for kind in ("eager", "graphed"):
        g, sampler, model, tr, va, te = _setup(cuda, name, p)
        held = {}
        if kind == "eager":                                                       # the TrainStep fit builds: its size averages per epoch
            real = fit.TrainStep

            def spy(*a, **kw):
                held["step"] = real(*a, **kw)
                return held["step"]
            monkeypatch.setattr(fit, "TrainStep", spy)
            log = lambda h: sizes.append(([held["step"].num_sampled_nodes(i) for i in range(4)],
                                          [held["step"].num_sampled_edges(i) for i in range(3)]))
        else:
            monkeypatch.undo()
            log = None
        torch.manual_seed(11)
        out[kind] = fit.fit(g, sampler, model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=3, eval_step=eval_step, train_metric=True,
                            train_step=kind, log=log)
        state[kind] = dict(params=[_bits(q).clone() for q in model.parameters()], rng=torch.get_rng_state(),
                           draw=sampler.draw_step() if hasattr(sampler, "draw_step") else None,
                           exp3=_bits(sampler._w_pos).clone() if getattr(sampler, "_w_pos", None) is not None else None)
    e, gr = out["eager"], out["graphed"]
    print(name, p, [h["train_loss"] for h in gr["history"]], [h["train_loss"] for h in e["history"]], gr["history"][-1]["sampled_nodes"])
    assert len(gr["history"]) == len(e["history"]) == 3 and gr["steps"] == e["steps"] == 3 * 14
    for hg, he, (sn, se) in zip(gr["history"], e["history"], sizes):
        for k in ("epoch", "train_loss", "val_acc", "val_loss", "lr", "train_acc"):
            assert hg[k] == he[k], (k, hg, he)
        assert set(hg) == set(he) | {"sampled_nodes", "sampled_edges"}
        assert hg["sampled_nodes"] == sn and hg["sampled_edges"] == se
    assert gr["best_val_acc"] == e["best_val_acc"] and gr["final"] == e["final"]
    sg, se_ = state["graphed"], state["eager"]
    assert all(torch.equal(a, b) for a, b in zip(sg["params"], se_["params"]))
    assert torch.equal(sg["rng"], se_["rng"]) and sg["draw"] == se_["draw"]
    assert (sg["exp3"] is None) == (se_["exp3"] is None) and (sg["exp3"] is None or torch.equal(sg["exp3"], se_["exp3"]))
    if "bandit" in name or "exp3" in name:
        assert sg["exp3"] is not None and not bool((sg["exp3"] == sg["exp3"].flatten()[0]).all())      # the rows moved


def _labor_step(cuda, p=0.0, **kw):
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    g, sampler, model, tr, va, te = _setup(cuda, "labor", p)
    step = GraphedTrainStep(g, sampler, model, BS, lr=0.01, ledger=True, **kw)
    loader = BatchLoader(tr, BS, seed=5).forever()
    model.train()
    step.calibrate(loader, steps=3)
    return g, sampler, model, va, step, loader


def test_the_free_running_loop_does_not_sync_per_step(cuda, monkeypatch):
    g, sampler, model, va, step, loader = _labor_step(cuda)
    step.run(loader, 6)                                                           # the capture (3 warm-up steps + 1) and 2 replays
    calls = []
    for owner, name in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.cuda.Event, "synchronize")):
        real = getattr(owner, name)

        def counted(*a, _real=real, _n=(owner.__name__, name), **kw):
            calls.append(_n)
            return _real(*a, **kw)
        monkeypatch.setattr(owner, name, counted)
    counts = []
    for n in (14, 28):
        calls.clear()
        step.run(loader, n, poll=4)
        counts.append(len(calls))
    monkeypatch.undo()
    print("synchronize calls for 14 and 28 steps:", counts)
    assert counts[0] == counts[1] and counts[0] <= 2
    rec = step.ledger()
    assert rec["steps_total"] == 6 + 14 + 28 == step.num_steps and rec["err"] == 0 and step.regrows == 0
    assert sampler.draw_step() == 3 + 48
    assert [s["S"] for s in step.sizes()] == [c.S for c in reversed(step.last_counts)] and step.sizes()[-1]["S"] == BS
    step.close()


def test_regrow_keeps_the_plain_loops_batches_and_streams(cuda):
    """A: the graphed step, 6 steps, then 14 with the warning threshold lowered to 0.05 (every size is over it) and a ring of 2, so
    that the third poll waits for the first one's record.  B: an eager twin over the same batches."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import BatchLoader, GraphedEvalStep, TrainStep
    gA, sA, mA, va, step, lA = _labor_step(cuda)
    es = GraphedEvalStep(gA, sA, mA, BS, False, loss_fn=step.loss_fn)
    rng0 = torch.get_rng_state()
    step.run(lA, 6)
    accA = [es.run(va)[0]]
    caps0 = [dict(c) for c in sA._engine.caps]
    step.regrow_at = 0.05
    try:
        step.run(lA, 14, poll=4, ring=2)
    finally:
        del step.regrow_at
    assert step.regrow_at == 0.85
    recA = step.ledger()
    accA.append(es.run(va)[0])
    print("regrows", step.regrows, "first_near_step", recA["first_near_step"], caps0, sA._engine.caps)
    assert step.regrows >= 1 and recA["err"] == 0 and recA["steps_total"] == 20 == step.num_steps
    assert es.captures == 2 and es.fallbacks == 0                                 # the validation graph was recorded again

    gB, sB, mB, trB, _, _ = _setup(cuda, "labor", 0.0)
    eager = TrainStep(gB, sB, mB, lr=0.01)
    lB = BatchLoader(trB, BS, seed=5).forever()
    mB.train()
    for _ in range(3):
        sB.sample_blocks(gB, next(lB))
    lossB = [float(eager(next(lB))) for _ in range(6)]
    accB = [fit.evaluate(gB, sB, mB, va, BS, False, eager.loss_fn)[0]]
    lossB += [float(eager(next(lB))) for _ in range(14)]
    accB.append(fit.evaluate(gB, sB, mB, va, BS, False, eager.loss_fn)[0])
    tot = 0.0
    for x in lossB:
        tot += x
    assert recA["loss_sum"] == tot and recA["loss_last"] == lossB[-1] and recA["nonfinite"] == 0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(mA.parameters(), mB.parameters()))
    assert sA.draw_step() == sB.draw_step() and torch.equal(torch.get_rng_state(), rng0)
    assert accA == accB
    assert [step.num_sampled_nodes(i, recA) for i in range(4)] == [eager.num_sampled_nodes(i) for i in range(4)]
    assert [step.num_sampled_edges(i, recA) for i in range(3)] == [eager.num_sampled_edges(i) for i in range(3)]
    es.close()
    step.close()


def test_an_error_word_in_a_polled_record_stops_the_enqueueing(cuda):
    """Planted on the host only: the first polled record the loop looks at is made to carry an error word."""
    from bliss_gnn_amd import _lib
    g, sampler, model, va, step, loader = _labor_step(cuda)
    step.run(loader, 6)
    real, seen = step._parse, []

    def planted(buf):
        rec = real(buf)
        seen.append(rec["steps_total"])
        if len(seen) == 1:
            rec["err"], rec["first_bad_step"] = 2, 5                              # BLISS_ERR_CAP_CAND
        return rec
    step._parse = planted
    with pytest.raises(RuntimeError, match=r"0x2 .*at step 5 ") as ei:
        step.run(loader, 28, poll=2, ring=2)
    step._parse = real
    assert _lib.err_string(2) in str(ei.value) and "exceeded its capacities or hit a kernel error" in str(ei.value)
    assert seen[0] == 6 + 2                                                       # the first poll's record: looked at on the third poll at
    rec = step.ledger()                                                           # the latest (the ring wraps), on the second if it had landed
    assert rec["steps_total"] == step.num_steps and rec["steps_total"] in (6 + 4, 6 + 6)   # enqueueing stopped there
    assert rec["err"] == 0                                                        # nothing on the device went wrong
    step.close()


def test_fit_graphed_refusals(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    g, tr, va, te = _task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
    with pytest.raises(NotImplementedError, match="MultiLayerFullNeighborSampler"):
        fit.fit(g, fit.make_sampler("full", [5, 5, 5]), model, tr, va, te, batch_size=BS, train_step="graphed")
    with pytest.raises(NotImplementedError, match="NeighborSampler with draw='host'"):
        fit.fit(g, fit.make_sampler("neighbor", [5, 5, 5]), model, tr, va, te, batch_size=BS, train_step="graphed")
    fp32 = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda)
    with pytest.raises(TypeError, match="learning rate"):
        fit.fit(g, fit.make_sampler("labor", [5, 5, 5]), fp32, tr, va, te, batch_size=BS, train_step="graphed")


def test_without_the_ledger_the_step_is_the_one_it_was(cuda):
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    res = {}
    for ledger in (False, True):
        g, sampler, model, tr, va, te = _setup(cuda, "poisson-bandit", 0.1)
        step = GraphedTrainStep(g, sampler, model, BS, lr=0.01, ledger=ledger)
        loader = BatchLoader(tr, BS, seed=5).forever()
        model.train()
        torch.manual_seed(3)
        step.calibrate(loader, steps=3)
        step.capture(loader, warmup=2)
        losses = [float(step(next(loader))) for _ in range(10)]
        res[ledger] = (losses, [_bits(q).clone() for q in model.parameters()], _bits(sampler._w_pos).clone(), torch.get_rng_state())
        if ledger:
            rec = step.ledger()
            assert rec["steps_total"] == 13 and rec["loss_last"] == losses[-1] and rec["err"] == 0
        else:
            assert step._ledger is None
            with pytest.raises(RuntimeError):
                step.run(loader, 1)
        step.close()
    assert res[False][0] == res[True][0] and torch.equal(res[False][2], res[True][2]) and torch.equal(res[False][3], res[True][3])
    assert all(torch.equal(a, b) for a, b in zip(res[False][1], res[True][1]))
