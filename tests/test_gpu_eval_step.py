"""GPU suite: the replayed validation pass (train.GraphedEvalStep) against the eager one (fit.evaluate), train_acc inside the
train steps, and both through fit.fit -- on the 3000-node task of tests/test_gpu_fit.py (500 validation ids, batch 128: three
replayed batches and a ragged one) and a multi-label variant of it."""
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu

BS, FAN = 128, [64, 32, 16]


def _task(cuda, multilabel=False, V=3000, E=40000, F=24, classes=4):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=21)
    gen = torch.Generator().manual_seed(2)
    feats = torch.randn(V, F, generator=gen).bfloat16()
    score = feats.float() @ torch.randn(F, classes, generator=gen)
    labels = (score > 0).float() if multilabel else score.argmax(1)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
    perm = torch.randperm(V, generator=gen).to(torch.int32).to(cuda)
    return g, perm[:1800], perm[1800:2300], perm[2300:]


def _trained(cuda, name, draw, multilabel, steps=4):
    """Graph, sampler and a model trained for a few eager steps; called twice it gives twins in the same state."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, TrainStep
    g, tr, va, _ = _task(cuda, multilabel)
    if name != "neighbor":
        g.edata["w"] = bg.normalized_edata(g)
    sampler = fit.make_sampler(name, FAN, draw=draw)
    torch.manual_seed(0)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
    step = TrainStep(g, sampler, model, lr=0.01, multilabel=multilabel)
    loader = BatchLoader(tr, BS, seed=5).forever()
    model.train()
    for _ in range(steps):
        step(next(loader))
    return g, sampler, model, va


def _eager_pass(g, sampler, model, va, multilabel):
    """fit.evaluate, with its loss function wrapped to keep what it saw: (val_acc, val_loss, host counts of the concatenated
    predictions, the per-batch loss terms)."""
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import _bce_loss, _ce_loss
    lf = _bce_loss() if multilabel else _ce_loss()
    preds, ys, terms = [], [], []

    def recording(pred, y):
        loss = lf(pred, y)
        preds.append(pred.float().cpu()); ys.append(y.cpu()); terms.append(float(loss) * pred.shape[0])
        return loss

    acc, loss = fit.evaluate(g, sampler, model, va, BS, multilabel, recording)
    lf.check_errors()
    counts = (ref.multilabel_counts if multilabel else ref.multiclass_counts)(torch.cat(preds), torch.cat(ys))[0]
    return acc, loss, counts, terms


def _loss_bound(terms, n):
    """|graphed - eager| for val_loss, from the code: per batch the graphed pass forms fp32(loss_b) * n_b (one fp32 product; the
    batch losses are bf16 for cross-entropy and fp32 for BCE, the same bits on both sides) and adds it to an fp32 sum (one fp32
    add): 2 B roundings of at most 2^-24 relative to S = sum |loss_b n_b|.  The eager pass sums the same terms in double (B
    roundings of 2^-53).  Both then divide by n in double."""
    B, S = len(terms), sum(abs(t) for t in terms)
    return (2 * B * 2.0 ** -24 + B * 2.0 ** -52) * S / n


CASES = [("poisson-bandit", "host", False), ("poisson-ladies", "host", False), ("ladies", "device", False), ("neighbor", "device", False),
         ("poisson-bandit", "host", True), ("neighbor", "device", True)]


@pytest.mark.parametrize("name,draw,multilabel", CASES)
def test_replayed_validation_is_the_eager_one(cuda, name, draw, multilabel):
    from bliss_gnn_amd.train import GraphedEvalStep
    gA, sA, mA, va = _trained(cuda, name, draw, multilabel)
    gB, sB, mB, _ = _trained(cuda, name, draw, multilabel)
    assert all(torch.equal(p, q) for p, q in zip(mA.parameters(), mB.parameters()))
    es = GraphedEvalStep(gA, sA, mA, BS, multilabel)
    for rep in range(2):                                                       # the second pass reuses the graph
        rows = sA._w_pos.clone() if hasattr(sA, "exp3") else None
        mA.train(); mB.train()
        torch.manual_seed(7 + rep)
        acc_g, loss_g = es.run(va)
        rng_g = torch.get_rng_state()
        torch.manual_seed(7 + rep)
        acc_e, loss_e, counts, terms = _eager_pass(gB, sB, mB, va, multilabel)
        print(name, draw, multilabel, rep, acc_g, acc_e, loss_g, loss_e, es.last_counts, counts, _loss_bound(terms, va.numel()))
        assert len(terms) == 4 and va.numel() == 500
        assert es.last_counts == counts                                        # the host counts of the concatenated predictions
        assert acc_g == acc_e                                                  # equal as floats
        assert abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
        assert torch.equal(rng_g, torch.get_rng_state())                       # torch's generator ends where the eager pass leaves it
        if draw == "device":
            assert sA.draw_step() == sB.draw_step()
        if rows is not None:
            assert torch.equal(rows, sA._w_pos) and torch.equal(sA._w_pos, sB._w_pos)      # no bandit update
        assert mA.training and mB.training
    assert es.captures == 1 and es.fallbacks == 0
    mA.eval()
    es.run(va[:BS])
    assert not mA.training                                                     # the flag is RESTORED, not set
    es.close()


@pytest.mark.parametrize("name,draw", [("poisson-bandit", "host"), ("ladies", "device")])
def test_a_batch_whose_finish_raises_is_redone_eagerly(cuda, name, draw):
    """finish_static is wrapped on the host to raise for the second replayed batch (no capacity is exceeded on the device): the
    per-batch buffer must be dropped, generator / draw step rewound and the batch redone, so the pass still equals the eager one."""
    from bliss_gnn_amd.train import GraphedEvalStep
    gA, sA, mA, va = _trained(cuda, name, draw, False)
    gB, sB, mB, _ = _trained(cuda, name, draw, False)
    es = GraphedEvalStep(gA, sA, mA, BS)
    torch.manual_seed(3)
    es.run(va)                                                                 # (calibrates and captures)
    torch.manual_seed(3)
    _eager_pass(gB, sB, mB, va, False)
    orig, calls = sA.finish_static, [0]

    def finish(slot=0, commit=True):
        out = orig(slot, commit)
        calls[0] += 1
        if calls[0] == 2:
            raise RuntimeError("planted: static-shape step exceeded its capacities")
        return out

    sA.finish_static = finish
    torch.manual_seed(4)
    acc_g, loss_g = es.run(va)
    rng_g = torch.get_rng_state()
    torch.manual_seed(4)
    acc_e, loss_e, counts, terms = _eager_pass(gB, sB, mB, va, False)
    assert calls[0] == 3 and es.fallbacks == 1 and es.captures == 1
    assert es.last_counts == counts and acc_g == acc_e and abs(loss_g - loss_e) <= _loss_bound(terms, va.numel())
    assert torch.equal(rng_g, torch.get_rng_state())
    if draw == "device":
        assert sA.draw_step() == sB.draw_step()
    es.close()


def test_samplers_without_a_static_path_are_refused(cuda):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import GraphedEvalStep
    g, _, _, _ = _task(cuda)
    model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
    for name, cls in (("full", "MultiLayerFullNeighborSampler"), ("ladies", "LadiesSampler"), ("bandit", "BanditLadiesSampler"),
                      ("neighbor", "NeighborSampler")):
        with pytest.raises(NotImplementedError, match=cls):
            GraphedEvalStep(g, fit.make_sampler(name, FAN), model, BS)


def test_train_acc_inside_the_replayed_step_changes_nothing_else(cuda):
    """Three twins on poisson-bandit: A replayed with train_metric=True, B replayed without, C stepping eagerly with a forward
    hook that keeps every prediction.  A and B: the same loss bits, parameters and EXP3 rows; A's counts: the host's over C's
    predictions of the ten batches."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep, PipelinedTrainStep

    def build(**kw):
        g, tr, _, _ = _task(cuda)
        g.edata["w"] = bg.normalized_edata(g)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.0).to(cuda).bfloat16()
        sampler = fit.make_sampler("poisson-bandit", FAN)
        step = GraphedTrainStep(g, sampler, model, BS, lr=0.01, **kw)
        loader = BatchLoader(tr, BS, seed=5).forever()
        torch.manual_seed(1)
        step.calibrate(loader, steps=3)
        return g, sampler, model, step, loader

    def run(step, loader, graphed, each=None):
        if graphed:
            step.capture(loader, warmup=2)
        else:
            for _ in range(3):
                step.eager_step(next(loader))
        if step.train_acc is not None:
            step.train_acc.reset()
        losses = []
        for _ in range(10):
            seeds = next(loader)
            losses.append((step(seeds) if graphed else step.eager_step(seeds)).clone())
            if each is not None:
                each(seeds)
        return losses

    gA, sA, mA, A, lA = build(train_metric=True)
    deltas = []
    lossA = run(A, lA, True, lambda seeds: deltas.append(A.last_batch_counts()))
    gB, sB, mB, B, lB = build()
    assert B.train_acc is None
    lossB = run(B, lB, True)
    assert all(torch.equal(a, b) for a, b in zip(lossA, lossB))
    assert all(torch.equal(p, q) for p, q in zip(mA.parameters(), mB.parameters()))
    assert torch.equal(sA._w_pos, sB._w_pos)
    gC, sC, mC, C, lC = build()
    preds, want = [], []
    hook = mC.register_forward_hook(lambda mod, inp, out: preds.append(out.detach().float().cpu()))
    labels = gC.ndata["labels"]
    run(C, lC, False, lambda seeds: want.append(ref.multiclass_counts(preds[-1], labels[seeds.long()].cpu())[0]))
    hook.remove()
    assert deltas == want                                                      # batch by batch
    total = tuple(sum(w[k] for w in want) for k in range(4))
    assert A.train_acc.counts() == total and total[3] == 10 * BS
    assert A.train_acc.compute() == ref.micro_f1(total)
    A.train_acc.check_errors()
    with pytest.raises(NotImplementedError, match="train_acc"):
        PipelinedTrainStep(gB, sB, mB, BS, train_metric=True)
    A.close(); B.close()


def test_final_split_accuracy_keeps_fit_micro_f1s_float(cuda):
    from bliss_gnn_amd.fit import _split_f1, micro_f1
    gen = torch.Generator().manual_seed(9)
    for multilabel in (False, True):
        x, y = (ref.multilabel_case(3000, 4, seed=3, tiny=False) if multilabel else ref.multiclass_case(3000, 4, seed=3))
        xd, yd = x.to(cuda), y.to(cuda)
        for n in (1, 387, 500, 1800):
            nid = torch.randperm(3000, generator=gen)[:n].to(torch.int32).to(cuda)
            assert _split_f1(xd, yd, nid, multilabel) == micro_f1(xd[nid.long()].float(), yd[nid.long()], multilabel), (multilabel, n)


def test_fit_with_the_graphed_validation_and_train_acc(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.model import SAGE

    def one(**kw):
        g, tr, va, te = _task(cuda)
        g.edata["w"] = bg.normalized_edata(g)
        torch.manual_seed(0)
        model = SAGE(24, 32, 4, 3, torch.relu, 0.1).to(cuda).bfloat16()
        return fit.fit(g, fit.make_sampler("poisson-bandit", FAN), model, tr, va, te, batch_size=BS, lr=0.01, max_epochs=3, **kw)

    base = one()
    new = one(eval_step="graphed", train_metric=True)
    assert [h["val_acc"] for h in new["history"]] == [h["val_acc"] for h in base["history"]]
    assert new["best_val_acc"] == base["best_val_acc"] and new["final"] == base["final"] and new["steps"] == base["steps"]
    assert [h["train_loss"] for h in new["history"]] == [h["train_loss"] for h in base["history"]]
    for h, b in zip(new["history"], base["history"]):
        assert 0.0 <= h["train_acc"] <= 1.0 and "train_acc" not in b
        assert abs(h["val_loss"] - b["val_loss"]) <= 1e-5 * abs(b["val_loss"])  # (the exact bound: test_replayed_validation_...)
    with pytest.raises(ValueError):
        one(eval_step="replayed")
