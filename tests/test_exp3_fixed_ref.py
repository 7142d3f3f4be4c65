"""Pins the CPU reference of tests/exp3_fixed_ref.py and what its case builders promise (no GPU): the GPU suite
(test_gpu_exp3_fixed_point.py) compares the kernels of csrc/exp3.hip with this reference bit for bit, so a disagreement
there has to point at the kernel."""
import random
from fractions import Fraction

import pytest
import torch

import exp3_fixed_ref as R
from oracle import bliss_oracle as bo
from oracle import numerics as nx


def test_value_and_nearest_bf16_against_torch():
    pats = torch.arange(0, 0x7f80, dtype=torch.int64)
    as_double = R.bf(pats).double()
    for b in list(range(0, 0x7f80, 97)) + [1, 0x7f, 0x80, 0x81, R.ONE, R.TOP, 0x7f7f]:
        assert float(R.value(b)) == float(as_double[b])              # exact: a bf16 is a double
        assert R.nearest_bf16(R.value(b)) == b
    assert R.value(0x8001) == -R.value(1) and R.value(1) == Fraction(1, 2 ** 133)
    # halfway between neighbours goes to the even pattern, a hair to either side to the nearer one
    for b in (0, 1, 0x7f, 0x80, R.ONE - 1, R.ONE, R.ONE + 1, 0x437e, 0x437f):
        lo, hi = R.value(b), R.value(b + 1)
        mid, eps = (lo + hi) / 2, (hi - lo) / 1024
        assert R.nearest_bf16(mid) == (b if b % 2 == 0 else b + 1)
        assert R.nearest_bf16(mid - eps) == b and R.nearest_bf16(mid + eps) == b + 1
    # and torch's own float -> bf16 rounding agrees on random doubles that are exact floats
    rng = random.Random(3)
    for _ in range(2000):
        f = torch.tensor([rng.getrandbits(31)], dtype=torch.int32).view(torch.float32)
        if not torch.isfinite(f) or float(f) > 3.38e38:
            continue
        assert R.nearest_bf16(Fraction(float(f))) == int(R.bits_of(f.bfloat16())[0])


def test_totals_of_part_b_round_like_the_oracle():
    totals = R.totals_b()
    assert len(totals) == 4 * 12 * 5 + 8 + 2 + R.B_RANDOM == 2250 and totals == R.totals_b()
    differ = [t for t in totals if t and R.nearest_bf16(Fraction(t, 2 ** 64)) != int(nx.bf16_bits(nx.int_to_bf16(t, 64).reshape(1))[0])]
    assert not differ, differ[:5]
    assert R.nearest_bf16(0) == 0 and R.nearest_bf16(Fraction(1 << 64, 2 ** 64)) == R.ONE
    # what the list promises: ties with an even and an odd q, the carry into the next binade, the msb <= 7 branch
    kinds = set()
    for t in totals[:240]:
        msb = t.bit_length() - 1
        q, rem, half = t >> (msb - 7), t & ((1 << (msb - 7)) - 1), 1 << (msb - 8)
        kinds.add(("tie" if rem == half else "off", q & 1, q == 255 and rem >= half))
    assert {("tie", 0, False), ("tie", 1, False), ("tie", 1, True), ("off", 0, False), ("off", 1, True)} <= kinds
    assert sum(t.bit_length() <= 8 for t in totals if t) >= 5


def test_encodings_carry_their_total():
    rng = random.Random(1)
    for t in R.totals_b()[::37] + [-1, -(1 << 70)]:
        assert R.limb_value(R.encode_canonical(t)) == t
        s = R.encode_scattered(t, rng)
        assert R.limb_value(s) == t
        assert int(s.abs().max()) < 2 ** 56 and int(s.abs().max()) > 2 ** 40 and bool((s < 0).any()) and bool((s > 0).any())
        assert int((s.view(R.SLOTS, 3).abs().sum(1) > 0).sum()) == R.SLOTS                  # every replica takes part


def test_exact_sum_is_the_oracles_row_sum_on_the_rows_of_part_a():
    row = R.row_a()
    assert row.numel() == 2 * (R.TOP + 1) and int(row[0]) == 0 and int(row[R.TOP]) == R.TOP == int(row[R.TOP + 1])
    assert R.exact_sum(row) == nx.row_exact_sum(R.bf(row)) == 2 * sum(R.term(b) for b in range(R.TOP + 1))
    for n in R.ROW_A_LENGTHS:
        part = R.spread(row, n)
        assert part.numel() == n and R.exact_sum(part) == nx.row_exact_sum(R.bf(part))
    big = torch.full((R.ROW_A_BIG,), R.TOP, dtype=torch.int64)
    assert R.exact_sum(big) == nx.row_exact_sum(R.bf(big)) == R.ROW_A_BIG * (0xff << 80)
    assert R.exact_sum(big) >> 64 >= 2 ** 32                         # the top limb passes 32 bits
    # the contract at the bottom: per-term truncation below 2^-64; 2^24 is the first value refused
    assert R.term(0) == 0 and R.term(1) == 0 and R.term(0x1f80) == 1 and R.term(0x1f7f) == 0       # 2^-64 and its predecessor
    assert R.term(0x1fc0) == 1 and R.term(0x2040) == 3                                             # 1.5 * 2^-64 -> 1, 3 * 2^-64
    assert R.value(R.TOP) == 2 ** 24 - 2 ** 16 and R.value(R.TOP + 1) == 2 ** 24
    assert sum(R.term(b) == 0 for b in range(R.TOP + 1)) == 0x1f80


@pytest.mark.parametrize("norm", R.NORMS_C)
def test_rows_of_part_c_keep_every_class(norm):
    nb = R.norm_bits(norm)
    assert R.nearest_bf16(Fraction(R.norm_total(nb), 2 ** 64)) == nb
    for row in (R.row_c(nb), R.interleaved_c(nb)):
        q = R.quotient(R.bf(row), nb)
        assert bool(R.below_2_24(q).all()) and row.numel() > 4000
    row = R.row_c(nb)
    cls = R.classes_c(row, nb)
    for name, mask in cls.items():
        must = R.subnormal_quotient_possible(nb) if name == "subnormal_quotient" else True
        assert bool(mask.any()) == must, (norm, name)
    # the interleaved row: every word pairs an element of the two-at-a-time class with a zero or subnormal one, both orders
    il = R.interleaved_c(nb)
    pair = R.classes_c(il, nb)["pair"].view(-1, 2)
    low = (il < 0x80).view(-1, 2)
    assert bool((pair ^ low).all()) and bool((pair[:, 0] != pair[:, 1]).all())
    assert bool(pair[:, 0].any()) and bool(pair[:, 1].any()) and bool((il == 0).any())
    if norm in R.SMALL_NORMS_C:
        oor = R.out_of_range_c(nb)
        qq = R.quotient(R.bf(oor), nb).float()
        assert bool(torch.isfinite(qq).all()) and int((qq >= 2.0 ** 24).sum()) == 1 and float(qq[300]) >= 2.0 ** 24


def test_chained_reference_moves_and_settles():
    steps = R.chained_reference(R.row_a(), 3)
    assert steps[0][0] != R.ONE and not torch.equal(steps[0][1], R.row_a())
    assert len({nb for nb, _ in steps}) >= 2                            # the norm of a later call is not that of the first


def test_cases_of_part_d():
    row, pos, fac = R.apply_case()
    assert pos.unique().numel() == pos.numel() > 38000 and set(R.bits_of(fac).tolist()) == set(R.bits_of(torch.tensor(R.FACTORS_D).bfloat16()).tolist())
    new = R.bf(row)[pos.long()] * fac
    old_t = torch.tensor([R.term(int(b)) > 0 for b in row[pos.long()]])
    new_t = torch.tensor([R.term(int(b)) > 0 for b in R.bits_of(new)])
    assert bool((old_t & ~new_t).any())                                 # a weight drops below 2^-64 ...
    assert bool(((R.bits_of(new) < 0x80) & (row[pos.long()] >= 0x80)).any())     # ... becomes subnormal or zero ...
    assert bool((R.bits_of(new) == 0).any()) and bool((R.bits_of(new) >= 0x4b00).any())   # ... and the top binade is reached
    rows, lists, want = R.ranks_case()
    (p00, _), (p10, _) = lists[0][0], lists[1][0]
    assert len(set(p00.tolist()) & set(p10.tolist())) > 1000            # identical positions in both ranks
    assert bool(((p00[1:] - p00[:-1]) == 1).any())                       # neighbours: two bf16 in one 32-bit word
    assert not torch.equal(want, rows)


def test_update_cases_reach_the_rounding_points():
    cases = R.update_cases()
    assert len(cases) == sum(len(v) for v in R.E_LISTS.values()) + R.E_COMBOS
    seen = dict(posinf=False, nan=False, clamp=False, exp0=False, nonfinite=False)
    for delta, (full, finite) in R.update_blocks().items():
        assert int(full.is_case.sum()) == sum(c["delta"] == delta for c in cases) and full.B < 40000
        deg = full.indptr[1:] - full.indptr[:-1]
        assert set(deg.tolist()) == set(R.E_LISTS["k_i"])                 # the block in-degrees are real
        assert set(full.g_indptr.diff()[full.dst_nid].tolist()) == set(R.E_LISTS["n_i"])
        rewards, ex, row, tr = full.reference()
        seen["posinf"] |= bool(torch.isposinf(tr["alpha2_over_k"].float()).any())
        seen["nan"] |= bool(torch.isnan(rewards.float()).any())
        seen["clamp"] |= bool((tr["d_r_unclamped"].float() > 1).any())
        unchanged = (R.bits_of(ex) == R.ONE) & (R.bits_of(row[full.pos]) == R.bits_of(full.w_old))
        seen["exp0"] |= bool((unchanged & (tr["d_r"].float() == 0)).any())
        seen["nonfinite"] |= bool((~torch.isfinite(row.float())).any())
        # the degree roundings the lists are there for: the bf16 ties and the int -> float -> bf16 double rounding
        k_bf = deg.to(torch.int32).bfloat16().float()
        assert {257: 256.0, 383: 384.0, 385: 384.0, 1025: 1024.0}.items() <= dict(zip(deg.tolist(), k_bf.tolist())).items()
        n_bf = full.g_indptr.diff().to(torch.int32).bfloat16().float().tolist()
        assert n_bf == [1.0, 3.0, 256.0, 65536.0, 2.0 ** 24, 2.0 ** 25, 2.0 ** 25]
        assert R.value(R.nearest_bf16(2 ** 25 + 2 ** 17 + 1)) == 2 ** 25 + 2 ** 18          # rounded once it would be this
        # the neutralised block is the same block, and its reference row is finite and below 2^24
        frow = finite.reference()[2]
        assert torch.equal(finite.indptr, full.indptr) and torch.equal(finite.pos, full.pos) and bool(R.below_2_24(frow).all())
        keep = torch.isfinite(row.float())
        assert torch.equal(R.bits_of(frow)[keep], R.bits_of(row)[keep])
    assert all(seen.values()), seen


def test_copied_update_statements_are_the_oracles():
    _, finite = R.update_blocks()[0.01]
    rewards, ex, row, _ = finite.reference()
    new_row, norm, tr = bo.exp3_update_row(finite.csc(), finite.oblock(), finite.row, rewards, delta=0.01)
    assert torch.equal(R.bits_of(tr["exp_rewards"]), R.bits_of(ex))
    nb = R.nearest_bf16(Fraction(R.exact_sum(row), 2 ** 64))
    assert int(R.bits_of(norm.reshape(1))[0]) == nb
    assert torch.equal(R.bits_of(new_row), R.bits_of(R.quotient(row, nb)))


def test_degrees_of_part_f():
    assert sum(R.DEGREES_F) == 69127
    g = bo.CSC(torch.tensor((0,) + R.DEGREES_F, dtype=torch.int64).cumsum(0), torch.zeros(sum(R.DEGREES_F), dtype=torch.int32))
    w = bo.normalized_edata(g)
    assert len(set(R.bits_of(w).tolist())) >= 9                           # 127/129, 255/257, 383/385, 1023/1025 round in pairs
