"""CPU suite: the NumPy restatement of the step ledger's rule (tests/ledger_ref.py) against a Python-float replay of
``TrainStep._ema`` / ``num_sampled_*`` (bliss_gnn_amd/train.py), its loss sums, first_bad_step / first_near_step, the epoch reset --
and planted deviations from the rule, each of which changes the record."""
import math

import numpy as np
import pytest

import ledger_ref as ref


def _random_steps(L, n, seed):
    rng = np.random.default_rng(seed)
    caps = np.full((L, 3), 2 ** 30, dtype=np.int32)
    out = []
    for t in range(n):
        c = np.zeros((L, 10), dtype=np.int32)
        c[:, 0] = rng.integers(1, 2000, L)
        c[:, 3] = rng.integers(1, 400000, L)
        c[:, 4] = rng.integers(0, 3000000, L)
        c[:, 1] = rng.integers(0, 2 ** 30, L)
        out.append((int(np.array([rng.uniform(0.0, 4.0)], dtype=np.float32).view(np.uint32)[0]), ref.F32, c))
    return caps, out


@pytest.mark.parametrize("L", [1, 3, 8])
def test_size_averages_are_trainsteps_python_floats_bit_for_bit(L):
    """TrainStep._ema over 300 random steps in plain Python floats (blocks input-most first = sampling order reversed), and its
    num_sampled_nodes / num_sampled_edges expression, against the restatement's cum_* words."""
    caps, steps = _random_steps(L, 300, seed=L)
    w, led = 0.99, ref.Ledger(L)
    cum_nodes, cum_edges, num_steps = [0.0] * (L + 1), [0.0] * L, 0
    for bits, dtype, c in steps:
        led.step(bits, dtype, c, caps, w, 0.85)
        num_steps += 1                                                            # train.py TrainStep._ema
        for i in range(L):
            n = L - 1 - i
            cum_nodes[i] = cum_nodes[i] * w + int(c[n, 3])
            cum_edges[i] = cum_edges[i] * w + int(c[n, 4])
        cum_nodes[L] = cum_nodes[L] * w + int(c[0, 0])
        d = led.as_dict()
        assert d["steps_total"] == num_steps
        for i in range(L):
            assert d["cum_nodes"][L - 1 - i].hex() == cum_nodes[i].hex() and d["cum_edges"][L - 1 - i].hex() == cum_edges[i].hex()
            want = cum_nodes[i] * (1 - w) / (1 - w ** num_steps)                  # num_sampled_nodes
            assert (d["cum_nodes"][L - 1 - i] * (1 - w) / (1 - w ** d["steps_total"])).hex() == want.hex()
        assert d["cum_out"].hex() == cum_nodes[L].hex()
    assert d["hw_K"] == [max(int(c[n, 3]) for _, _, c in steps) for n in range(L)]
    assert d["hw_E"] == [max(int(c[n, 1]) for _, _, c in steps) for n in range(L)]
    assert d["near"] == 0 and d["err"] == 0 and d["first_bad_step"] == -1 and d["first_near_step"] == -1


def test_loss_sums_widen_bf16_and_fp32_exactly_and_add_in_step_order():
    import torch
    caps, steps = ref.planted_steps(3)
    led, tot, cnt, bad = ref.Ledger(3), 0.0, 0, 0
    for t, (bits, dtype, c) in enumerate(steps[:21]):                            # (the finite ones)
        led.step(bits, dtype, c, caps, 0.99, 0.85)
        x = (torch.tensor([bits], dtype=torch.int16).view(torch.bfloat16) if dtype == ref.BF16
             else torch.tensor([bits], dtype=torch.int32).view(torch.float32))[0]
        tot += float(x); cnt += 1                                                # fit's eager loop: tot += float(step(seeds))
        assert led.as_dict()["loss_last"] == float(x) and led.as_dict()["loss_sum"].hex() == tot.hex()
    assert led.steps_epoch == cnt == 21 and led.nonfinite == 0
    for bits, dtype, c in steps[21:]:
        led.step(bits, dtype, c, caps, 0.99, 0.85)
    assert led.nonfinite == 2 and math.isnan(float(led.loss_sum)) and led.steps_total == 40


@pytest.mark.parametrize("L", [1, 3, 8])
def test_first_steps_sticky_words_and_the_resets(L):
    caps, steps = ref.planted_steps(L)
    led = ref.Ledger(L)
    for t, (bits, dtype, c) in enumerate(steps):
        led.step(bits, dtype, c, caps, 0.99, 0.85)
        assert led.first_bad_step == (17 if t >= 17 else -1) and led.err == (0 if t < 17 else 8 if t < 23 else 12)
        assert led.first_near_step == (29 if t >= 29 else -1) and led.near == int(t >= 29)     # at the limit (t = 11): no warning
    before = led.as_dict()
    led.reset_epoch()
    after = led.as_dict()
    assert (after["steps_epoch"], after["loss_sum"], after["nonfinite"]) == (0, 0.0, 0)
    for k in before:
        if k not in ("steps_epoch", "loss_sum", "nonfinite", "loss_last"):
            assert after[k] == before[k], k
    assert after["steps_total"] == 40
    led.rearm()
    assert (led.near, led.first_near_step, led.err, led.first_bad_step) == (0, -1, 12, 17)
    assert len(led.to_bytes()) == ref.ledger_bytes(L) and ref.ledger_bytes(L) % 8 == 0
    led.step(*steps[0][:2], steps[0][2], caps, 0.99, 0.85)
    assert led.steps_epoch == 1 and led.steps_total == 41 and led.first_bad_step == 17


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_a_planted_fault_changes_the_record(fault):
    assert len(ref.FAULTS) >= 4
    caps, steps = ref.planted_steps(3)
    if fault in ("fma", "w_after"):
        caps, steps = _random_steps(3, 300, seed=7)
    good, bad = ref.Ledger(3), ref.Ledger(3)
    for bits, dtype, c in steps:
        good.step(bits, dtype, c, caps, 0.99, 0.85)
        bad.step(bits, dtype, c, caps, 0.99, 0.85, fault=fault)
    assert not np.array_equal(good.words(), bad.words())
    if fault == "ge":
        assert bad.first_near_step == 11 and good.first_near_step == 29
    if fault == "err_overwrite":
        assert bad.err == 4 and good.err == 12
