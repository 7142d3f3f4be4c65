"""GPU suite: the one-launch multi-label loss (csrc/loss.hip: k_bce_logits; nn.BCEWithLogitsLoss) per element against fp64, its
folded and masked forms, its determinism, and the train loops that use it.

The yardstick is ``binary_cross_entropy_with_logits`` on the same bf16 logits in float64 with its autograd gradient -- not torch's
own bf16 route, which rounds log_sigmoid(x) and sigmoid(x) to bf16 before it meets the fp32 target.

    gradient   |got - ref| <= 1 ulp_bf16(ref) + 2^-22 / denom      every element, none left out
    loss       |got - ref| <= 2^-18 |ref|

Gradient: the one final rounding gives half an ulp of the fp32 value (which may sit one binade above ref: 1 ulp of ref); the
absolute term covers the fp32 evaluation of sigma - y, a few roundings of 2^-24 on values below 1, before the 1 / denom scale.
Loss: the longest fp32 addition chain (a lane's stride over the classes, the wave's tree, the row-ordered sum) is under 64
additions of 2^-24 relative each, on terms that are all >= 0.

Infinite logits take their limits: the gradient (1 - y) / denom or -y / denom, the loss term 0 where the target agrees with the
logit entirely (+inf with y = 1, -inf with y = 0) and +inf elsewhere -- the float64 reference itself gives NaN there (inf - inf),
so the reference is evaluated with +-1e4 in their place (exp(-1e4) = 0 in float64: the limits, exactly) and the expected loss is
+inf when one of those terms is.  Because a batch with such a term has no finite loss to hold to the bound, every case runs a
second time without the two infinite plants (0, -0, +-88, +-200 stay), where the loss bound applies in full.

Measured on the MI355X (kernel on the accurate expf / log1pf; the fast __expf / __logf forms were not tried), worst ratio to the
bound over logit scales 1, 3, 20, both kinds of target, with and without the infinite plants -- gradient / loss:
    (256, 100) 0.500 / 0.020    (1000, 100) 0.500 / 0.022    (7, 1000) 0.500 / 0.023
    (32, 3)    0.499 / 0.016    (1, 1)      0.346 / 0.001    (300, 65) 0.500 / 0.027
    (4097, 5)  0.500 / 0.016    (9001, 3)   0.500 / 0.025    (the second trip of the grid-stride row loop; the full 1024-workgroup grid)
i.e. the gradient is the correctly rounded bf16 of the fp64 value up to the rounding's own half ulp, as the fp32 restatement with
an exact exponential is on the CPU, and the loss is within 1e-7 relative.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

from bounds import assert_within, ulp_bf16   # noqa: E402

SHAPES = [(256, 100), (1000, 100), (7, 1000), (32, 3), (1, 1), (300, 65), (4097, 5), (9001, 3)]
PLANTS = [0.0, -0.0, 88.0, -88.0, 200.0, -200.0, float("inf"), -float("inf")]
LOSS_REL = 2.0 ** -18


def _case(shape, scale, soft, seed, infs=True):
    """bf16 logits N(0, 1) * scale with the plants in the first entries, fp32 targets (0/1 at density 0.1, or uniform) -- CPU."""
    gen = torch.Generator().manual_seed(seed)
    n, c = shape
    x = (torch.randn(n, c, generator=gen) * scale).bfloat16()
    plants = PLANTS if infs else PLANTS[:6]
    k = min(len(plants), n * c)
    x.view(-1)[:k] = torch.tensor(plants[:k]).bfloat16()
    y = torch.rand(n, c, generator=gen) if soft else (torch.rand(n, c, generator=gen) < 0.1).float()
    return x, y


def _reference(x, y, denom):
    """fp64 loss (sum / denom) and gradient on the bf16 logits ``x`` (any device); infinite logits at their limits."""
    xd, yd = x.double(), y.double()
    inf = torch.isinf(xd)
    xr = torch.where(inf, torch.sign(xd) * 1e4, xd).requires_grad_(True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(xr, yd, reduction="sum") / denom
    loss.backward()
    agree = torch.where(xd > 0, yd == 1, yd == 0)
    if bool((inf & ~agree).any()):
        loss = torch.full_like(loss, float("inf"))
    return loss.detach(), xr.grad


def _check(got_loss, got_grad, x, y, denom, what):
    """The two bounds of the module docstring; prints the figures before it asserts.  Returns (gradient ratio, loss error / bound)."""
    ref_loss, ref_grad = _reference(x, y, denom)
    mag = torch.full_like(ref_grad, 1.0 / denom)
    got_loss = got_loss.double().reshape(())
    if bool(torch.isinf(ref_loss)):
        loss_ratio = 0.0 if float(got_loss) == float("inf") else float("inf")
    else:
        loss_ratio = float((got_loss - ref_loss).abs() / (LOSS_REL * ref_loss.abs()))
    err = (got_grad.double() - ref_grad).abs()
    bound = ulp_bf16(ref_grad) + 2.0 ** -22 / denom
    print("%s: gradient worst ratio %.3f, loss %.9g ref %.9g ratio %.3f" % (what, float((err / bound).max()), float(got_loss),
                                                                            float(ref_loss), loss_ratio))
    ratio = assert_within(got_grad, ref_grad, mag, 1, 2.0 ** -14, what + " gradient")      # (2^-14 * 2^-8 / denom = 2^-22 / denom)
    assert loss_ratio <= 1.0, (what, float(got_loss), float(ref_loss), loss_ratio)
    return ratio, loss_ratio


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("scale", [1, 3, 20])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_per_element_vs_fp64(cuda, shape, scale, soft):
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    lf = BCEWithLogitsLoss()
    for infs in (True, False):
        x, y = _case(shape, scale, soft, 11 + 7 * scale + soft, infs)
        x, y = x.to(cuda).requires_grad_(True), y.to(cuda)
        loss = lf(x, y)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        loss.backward()
        assert x.grad.dtype == torch.bfloat16 and bool(torch.isfinite(x.grad.float()).all())
        assert int(lf._state[0]) == 0 and int(lf._state[1]) == 0
        _check(loss.detach(), x.grad, x.detach(), y, shape[0] * shape[1], "%s x%d %s%s" % (shape, scale, "soft" if soft else "0/1",
                                                                                       "" if infs else " (no inf)"))
        with torch.no_grad():                                   # (fit.evaluate's route: the same launch, no graph)
            assert torch.equal(lf(x, y), loss.detach())


def test_nan_propagates(cuda):
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    x, y = _case((32, 3), 3, False, 5, infs=False)
    x[4, 1] = float("nan")
    x, y = x.to(cuda).requires_grad_(True), y.to(cuda)
    loss = BCEWithLogitsLoss()(x, y)
    loss.backward()
    g = x.grad.float()
    assert bool(torch.isnan(loss)) and bool(torch.isnan(g[4, 1])) and int(torch.isnan(g).sum()) == 1


def test_non_unit_incoming_gradient(cuda):
    """(loss * 0.5).backward(): 0.5 x the gradient, to one more bf16 rounding."""
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    x, y = _case((300, 65), 3, True, 3)
    y = y.to(cuda)
    x1, x2 = x.to(cuda).requires_grad_(True), x.to(cuda).requires_grad_(True)
    lf = BCEWithLogitsLoss()
    lf(x1, y).backward()
    (lf(x2, y) * 0.5).backward()
    want = 0.5 * x1.grad.double()
    assert_within(x2.grad, want, torch.zeros_like(want), 1, 0.0, "0.5 x gradient")


def test_sum_and_target_gather_inside(cuda):
    """bliss_bce_logits_sum (the output layer's `fc_self + h_neigh` and the gather of the batch's targets taken into the loss
    kernel) == the plain kernel on the materialised sum and targets: same loss bits, same gradient bits, delivered to both
    addends."""
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    gen = torch.Generator().manual_seed(7)
    n, c, V = 256, 100, 5000
    a = (torch.randn(n, c, generator=gen) * 3).bfloat16().to(cuda).requires_grad_(True)
    b = (torch.randn(n, c, generator=gen) * 3).bfloat16().to(cuda).requires_grad_(True)
    table = (torch.rand(V, c, generator=gen) < 0.1).float().to(cuda)
    ids = torch.randperm(V, generator=gen)[:n].to(torch.int32).to(cuda)
    lf = BCEWithLogitsLoss()
    l1 = lf.backward_from_parts(a, b, table, ids)
    ga, gb = a.grad.clone(), b.grad.clone()
    a.grad = b.grad = None
    l2 = lf.backward_from(a + b, table[ids.long()])
    assert l1.dtype == torch.float32 and torch.equal(l1, l2)
    assert torch.equal(ga, a.grad) and torch.equal(gb, b.grad) and torch.equal(ga, gb)
    _check(l1, ga, (a + b).detach(), table[ids.long()], n * c, "folded sum and gather")


def _masked(a, b, table, ids, lo, n_dev, denom, state):
    from bliss_gnn_amd import _lib
    cap, C = a.shape
    dx = torch.full((cap, C), 9.0, dtype=torch.bfloat16, device=a.device)
    rows = torch.empty(cap, dtype=torch.float32, device=a.device)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib.bliss_bce_logits_masked(a.data_ptr(), a.stride(0), 0 if b is None else b.data_ptr(), 0 if b is None else b.stride(0),
                                                table.data_ptr(), table.shape[0], ids.data_ptr(), lo, cap, n_dev.data_ptr(), denom, C,
                                                rows.data_ptr(), dx.data_ptr(), dx.stride(0), loss.data_ptr(), state.data_ptr(),
                                                state.data_ptr() + 4, torch.cuda.current_stream().cuda_stream), "bliss_bce_logits_masked")
    torch.cuda.synchronize()
    return loss, dx


def test_masked_kernel(cuda):
    """bliss_bce_logits_masked: the rows at and beyond the device-side count get exactly +0 gradient rows and no loss, even when they
    hold NaN logits and another rank's node ids; the divisor is `denom`; the valid rows are held per element to the fp64 bounds;
    an id outside the table raises the error bit and its row counts for nothing; two ranks' launches with the global divisor add
    up to the one launch over the whole batch."""
    gen = torch.Generator().manual_seed(3)
    cap, n, C, lo, n_table = 96, 61, 41, 1000, 500
    denom = float(512 * C)
    a = (torch.randn(cap, C, generator=gen) * 3).bfloat16()
    b = (torch.randn(cap, C, generator=gen) * 3).bfloat16()
    a[n:] = float("nan")
    a, b = a.to(cuda), b.to(cuda)
    table = (torch.rand(n_table, C, generator=gen) < 0.1).float().to(cuda)
    ids = torch.randint(lo, lo + n_table, (cap,), generator=gen).to(torch.int32)
    ids[n:] = 7                                                   # (padding: another rank's node)
    ids = ids.to(cuda)
    n_dev = torch.tensor([n], dtype=torch.int32, device=cuda)
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    for second in (b, None):
        loss, dx = _masked(a, second, table, ids, lo, n_dev, denom, state)
        assert int(state[0]) == 0 and int(state[1]) == 0
        assert not dx[n:].view(torch.int16).any()
        x = a[:n] if second is None else (a[:n] + second[:n])
        _check(loss, dx[:n], x, table[ids[:n].long() - lo], denom, "masked form" + ("" if second is None else " with two addends"))
    # an id outside the table: the error bit, a zero row, no loss
    bad = ids.clone()
    bad[5] = lo + n_table
    bad[9] = lo - 1
    loss_bad, dx_bad = _masked(a, b, table, bad, lo, n_dev, denom, state)
    assert int(state[0]) == 0 and int(state[1]) == 2                # (BLISS_ERR_CAP_CAND)
    state.zero_()
    assert not dx_bad[5].view(torch.int16).any() and not dx_bad[9].view(torch.int16).any()
    keep = torch.ones(n, dtype=torch.bool, device=cuda)
    keep[5] = keep[9] = False
    x = (a[:n] + b[:n])
    _check(loss_bad, dx_bad[:n][keep], x[keep], table[ids[:n].long() - lo][keep], denom, "masked form without the two refused rows")
    # two ranks' worth of rows with the global divisor == the whole batch in one launch
    n1 = 27
    whole, dx_whole = _masked(a, b, table, ids, lo, n_dev, denom, state)
    first, dx1 = _masked(a[:n1].contiguous(), b[:n1].contiguous(), table, ids[:n1].contiguous(), lo,
                         torch.tensor([n1], dtype=torch.int32, device=cuda), denom, state)
    rest, dx2 = _masked(a[n1:].contiguous(), b[n1:].contiguous(), table, ids[n1:].contiguous(), lo,
                        torch.tensor([n - n1], dtype=torch.int32, device=cuda), denom, state)
    assert abs(float(first) + float(rest) - float(whole)) <= LOSS_REL * abs(float(whole))
    assert torch.equal(torch.cat([dx1, dx2]).view(torch.int16), dx_whole.view(torch.int16))


def test_loss_bits_do_not_depend_on_the_launch(cuda):
    """The same inputs launched twice give the same loss and gradient bits, for a launch of one workgroup (4 rows) and for one of
    more workgroups than the grid holds (5000 rows: grid-stride); a few valid rows in a capacity of many workgroups give the loss
    bits of the launch that holds just those rows; the ticket word is zero after every launch."""
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd.nn import _bce_launch
    state = torch.zeros(2, dtype=torch.int32, device=cuda)
    for n, c in ((4, 100), (5000, 100), (300, 65)):
        x, y = _case((n, c), 3, True, 17)
        x, y = x.to(cuda), y.to(cuda)
        x.view(-1)[6:8] = 1.5                                    # (finite loss: the infinite plants out)
        runs = []
        for _ in range(3):
            loss, dx = _bce_launch(x, y, state)
            torch.cuda.synchronize()
            assert int(state[0]) == 0 and int(state[1]) == 0
            runs.append((loss.clone(), dx.clone()))
        assert bool(torch.isfinite(runs[0][0]))
        for l, d in runs[1:]:
            assert torch.equal(l.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(d.view(torch.int16), runs[0][1].view(torch.int16))
    # 7 valid rows among 3000 capacity rows (750 workgroups) against a launch of exactly those 7 rows (2 workgroups)
    cap, n, c = 3000, 7, 100
    x, y = _case((cap, c), 3, True, 19, infs=False)
    x, y = x.to(cuda), y.to(cuda)
    ids = torch.arange(cap, dtype=torch.int32, device=cuda)
    denom = float(n * c)
    big, _ = _masked(x, None, y, ids, 0, torch.tensor([n], dtype=torch.int32, device=cuda), denom, state)
    small, _ = _masked(x[:n].contiguous(), None, y, ids[:n].contiguous(), 0, torch.tensor([n], dtype=torch.int32, device=cuda), denom, state)
    plain, _ = _bce_launch(x[:n].contiguous(), y[:n].contiguous(), state)
    torch.cuda.synchronize()
    assert int(state[0]) == 0
    assert torch.equal(big.view(torch.int32), small.view(torch.int32)) and torch.equal(big.view(torch.int32).reshape(()), plain.view(torch.int32))


# ------------------------------------------------------------------------------------------------ through the train loops
NODES, EDGES, FEAT, CLS, FAN, BS, LR = 8000, 160000, 64, 16, [400, 200, 100], 64, 0.002


def _setup(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.synth import chung_lu_csc, node_data
    ip, ix, ei = chung_lu_csc(NODES, EDGES, seed=12)
    feats, labels, _ = node_data(NODES, FEAT, CLS, 100, seed=1, multilabel=True)
    assert labels.dtype == torch.float32 and labels.shape == (NODES, CLS)

    def build():
        g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": feats.to(cuda), "labels": labels.to(cuda)})
        g.edata["w"] = bg.normalized_edata(g)
        sampler = bg.PoissonBanditLadiesSampler(FAN, eta=0.1)
        torch.manual_seed(0)
        model = SAGE(FEAT, 32, CLS, 3, torch.relu, 0.0).to(cuda).bfloat16()
        return g, sampler, model
    return build, torch.arange(NODES, dtype=torch.int32, device=cuda)


def test_train_step_fused_vs_torch_loss(cuda, monkeypatch):
    """TrainStep(multilabel=True) on the in-tree loss against the same first step with BLISS_FUSED_BCE=0 (torch's module on bf16
    logits: ~3e-4 relative off the fp64 loss by its own bf16 roundings): losses within 1e-3 relative; the first Adam step moves
    every parameter by ~lr * sign(g), so the parameters land within 2.5 lr of each other."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    from bliss_gnn_amd.train import BatchLoader, TrainStep
    build, ids = _setup(cuda)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("BLISS_FUSED_BCE", fused)
        g, sampler, model = build()
        step = TrainStep(g, sampler, model, lr=LR, multilabel=True)
        assert isinstance(step.loss_fn, BCEWithLogitsLoss) == (fused == "1")
        loader = BatchLoader(ids, BS, seed=5).forever()
        torch.manual_seed(9)
        loss = step(next(loader))
        sampler.check_errors()
        assert step.last["pred"].shape == (BS, CLS)
        outs.append((float(loss), [p.detach().float().clone() for p in model.parameters()],
                     [b.srcdata[bg.NID].clone() for b in step.last["mfgs"]]))
    (la, pa, ka), (lb, pb, kb) = outs
    assert all(torch.equal(x, y) for x, y in zip(ka, kb))                                  # the same first-step blocks
    print("fused %.9g torch %.9g" % (la, lb))
    assert la == la and abs(la - lb) <= 1e-3 * abs(lb)
    for x, y in zip(pa, pb):
        assert float((x - y).abs().max()) <= 2.5 * LR


def test_graphed_step_replay_equals_its_eager_step(cuda):
    """GraphedTrainStep(multilabel=True): the step replayed from its HIP graph == the same static-shape step launched kernel by
    kernel, bit for bit on the losses, the EXP3 rows and the parameters."""
    from bliss_gnn_amd.nn import BCEWithLogitsLoss
    from bliss_gnn_amd.train import BatchLoader, GraphedTrainStep
    build, ids = _setup(cuda)
    outs = []
    for graphed in (True, False):
        g, sampler, model = build()
        step = GraphedTrainStep(g, sampler, model, BS, lr=LR, multilabel=True)
        assert isinstance(step.loss_fn, BCEWithLogitsLoss)
        loader = BatchLoader(ids, BS, seed=5).forever()
        torch.manual_seed(9)
        step.calibrate(loader, steps=3)
        losses = []
        if graphed:
            step.capture(loader, warmup=2)                       # 2 eager static steps + 1 replayed
            losses.append(float(step.loss))
            for _ in range(3):
                losses.append(float(step(next(loader))))
        else:
            for i in range(6):
                loss = step.eager_step(next(loader))
                if i >= 2:
                    losses.append(float(loss))
        sampler.check_errors()
        outs.append((losses, sampler.exp3_weights.cpu().view(torch.int16).clone(), [p.detach().cpu().clone() for p in model.parameters()]))
        step.close()
    print("losses", outs[0][0])
    assert outs[0][0] == outs[1][0] and all(l == l for l in outs[0][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))


def test_pipelined_step_folds_sum_and_gather_into_the_loss(cuda, monkeypatch):
    """PipelinedTrainStep(multilabel=True): the split forward hands the output layer's two addends and the (table, ids) pair to
    backward_from_parts -- every loss launch of the run carries both, the logits sum is never formed -- and computes the loss
    bits, EXP3 rows and parameters of the non-split route (BLISS_SPLIT_FORWARD=0: plain logits, gathered targets)."""
    from bliss_gnn_amd import nn as bnn
    from bliss_gnn_amd.train import BatchLoader, PipelinedTrainStep
    build, ids = _setup(cuda)
    calls = []
    real = bnn._bce_launch

    def spy(x, targets, state, x2=None, label_ids=None):
        calls.append((x2 is not None, label_ids is not None, tuple(targets.shape)))
        return real(x, targets, state, x2=x2, label_ids=label_ids)
    monkeypatch.setattr(bnn, "_bce_launch", spy)
    outs = []
    for split in ("1", "0"):
        monkeypatch.setenv("BLISS_SPLIT_FORWARD", split)
        del calls[:]
        g, sampler, model = build()
        step = PipelinedTrainStep(g, sampler, model, BS, lr=LR, multilabel=True)
        loader = BatchLoader(ids, BS, seed=5).forever()
        torch.manual_seed(9)
        step.calibrate(loader, steps=3)
        step.capture(loader, warmup=1)
        losses = [float(x) for x in step(loader)]
        losses.append(float(step.drain()))
        sampler.check_errors()
        assert calls
        if split == "1":
            assert all(c == (True, True, (NODES, CLS)) for c in calls), calls
        else:
            assert all(c == (False, False, (BS, CLS)) for c in calls), calls
        outs.append((losses, sampler.exp3_weights.cpu().view(torch.int16).clone(), [p.detach().cpu().clone() for p in model.parameters()]))
        step.close()
    print("losses", outs[0][0])
    assert outs[0][0] == outs[1][0] and all(l == l for l in outs[0][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))


def test_static_sharded_step_world_of_one(cuda, monkeypatch):
    """StaticShardedTrainStep(multilabel=True), world of one rank over RCCL: the in-tree masked loss against BLISS_SHARD_FUSED_LOSS=0
    (torch ops in fp32 on the bf16 logits) within 1e-3 relative over the first 3 steps (step 0 from identical parameters; the later
    steps from parameters a few roundings apart); the fused step takes the two addends un-added; replayed from its HIP graph it
    trains exactly like launched kernel by kernel, bit for bit on losses, parameters and EXP3 rows."""
    import torch.distributed as dist
    from bliss_gnn_amd import shard as sh
    from bliss_gnn_amd import shard_static as ss
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.synth import chung_lu_csc, node_data
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29761"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=cuda)
    try:
        ip, ix, ei = chung_lu_csc(NODES, EDGES, seed=12)
        feats, labels, _ = node_data(NODES, FEAT, CLS, 100, seed=1, multilabel=True)
        bounds = sh.partition_by_in_edges(ip, 1)
        gen = torch.Generator().manual_seed(11)
        batches = [torch.randperm(NODES, generator=gen)[:BS].to(torch.int32).to(cuda) for _ in range(8)]
        outs = {}
        for kind in ("fused", "torch", "fused-graph"):
            monkeypatch.setenv("BLISS_SHARD_FUSED_LOSS", "0" if kind == "torch" else "1")
            g = sh.GraphShard.from_global(ip, ix, ei, bounds, 0, device=cuda, ndata={"features": feats, "labels": labels})
            sampler = ss.DenseShardedSampler(g, FAN, eta=0.1, seed=7)
            torch.manual_seed(0)
            model = SAGE(FEAT, 32, CLS, 3, torch.relu, 0.0).to(cuda).bfloat16()
            step = ss.StaticShardedTrainStep(g, sampler, model, BS, lr=LR, multilabel=True)
            it = iter(batches)
            step.calibrate(it, steps=2)
            # (what _loss_backward_step and the output layer dispatch on: the masked launch with the two addends un-added)
            assert step._fused_loss_ok(torch.empty(BS, CLS, dtype=torch.bfloat16, device=cuda)) == (kind != "torch")
            losses = []
            if kind == "fused-graph":
                step.capture(it, warmup=2)                      # batches 2, 3 eagerly, batch 4 by the first replay
                assert step.graph is not None
            else:
                for _ in range(3):
                    step(next(it))
                    losses.append(step.finish()[0])
            for b in it:
                step(b)
                losses.append(step.finish()[0])
            sampler.check_errors()
            outs[kind] = (losses, [p.detach().float().cpu() for p in model.parameters()], sampler.ops.w_pos.cpu().view(torch.int16).clone())
            step.close()
        print("fused", outs["fused"][0], "torch", outs["torch"][0])
        for a, b in list(zip(outs["fused"][0], outs["torch"][0]))[:3]:
            assert a == a and abs(a - b) <= 1e-3 * abs(b)
        assert outs["fused-graph"][0] == outs["fused"][0][3:]
        assert all(torch.equal(a, b) for a, b in zip(outs["fused-graph"][1], outs["fused"][1]))
        assert torch.equal(outs["fused-graph"][2], outs["fused"][2])
    finally:
        dist.destroy_process_group()


def _two_rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from bliss_gnn_amd import shard as sh
    from bliss_gnn_amd import shard_static as ss
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.synth import chung_lu_csc, node_data
    ip, ix, ei = chung_lu_csc(NODES, EDGES, seed=12)
    feats, labels, _ = node_data(NODES, FEAT, CLS, 100, seed=1, multilabel=True)
    bounds = sh.partition_by_in_edges(ip, world)
    g = sh.GraphShard.from_global(ip, ix, ei, bounds, rank, device=dev, ndata={"features": feats, "labels": labels})
    per_rank = BS // world

    def my_batch(si):                                            # every rank contributes the same number of seeds it owns
        gen = torch.Generator().manual_seed(100 + 7 * si + rank)
        return (torch.randperm(g.hi - g.lo, generator=gen)[:per_rank] + g.lo).to(torch.int32).to(dev)
    out = {}
    for kind in ("fused", "torch"):
        os.environ["BLISS_SHARD_FUSED_LOSS"] = "0" if kind == "torch" else "1"
        sampler = ss.DenseShardedSampler(g, FAN, eta=0.1, seed=7)
        torch.manual_seed(0)
        model = SAGE(FEAT, 32, CLS, 3, torch.relu, 0.0).to(dev).bfloat16()
        step = ss.StaticShardedTrainStep(g, sampler, model, per_rank, lr=LR, multilabel=True)
        assert step._fused_loss_ok(torch.empty(per_rank, CLS, dtype=torch.bfloat16, device=dev)) == (kind == "fused")
        losses = []
        for si in range(3):
            step(my_batch(si))
            losses.append(step.finish()[0])
        sampler.check_errors()
        out[kind] = dict(losses=losses, params=[p.detach().float().cpu() for p in model.parameters()])
    torch.save(dict(rank=rank, **out), os.path.join(outdir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_static_sharded_step_two_ranks(cuda):
    """Two ranks on the one GPU (gloo carries the collectives), each with its own shard of the target table: every rank's masked
    launch divides by the GLOBAL batch x classes, so the all-reduced loss is the global mean -- within 1e-3 relative of the torch
    route's over 3 steps -- and the replicas' parameters and losses stay identical."""
    import tempfile
    from test_gpu_shard import _spawn
    with tempfile.TemporaryDirectory() as outdir:
        res = _spawn(_two_rank_worker, 2, outdir)
    for r in res:
        print("rank", r["rank"], "fused", r["fused"]["losses"], "torch", r["torch"]["losses"])
        for a, b in zip(r["fused"]["losses"], r["torch"]["losses"]):
            assert a == a and abs(a - b) <= 1e-3 * abs(b)
    assert res[0]["fused"]["losses"] == res[1]["fused"]["losses"]
    assert all(torch.equal(a, b) for a, b in zip(res[0]["fused"]["params"], res[1]["fused"]["params"]))
