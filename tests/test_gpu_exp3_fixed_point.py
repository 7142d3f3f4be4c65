"""The EXP3 exact row sum and its bf16 norm (csrc/exp3.hip) at the edges of the fixed point, through the C ABI, against
the CPU reference of tests/exp3_fixed_ref.py (pinned by test_exp3_fixed_ref.py).  Every comparison is an equality of bits
or of Python ints.

  A  k_row_sum / row_digits                       test_row_sum_*
  B  limbs_to_bf16                                test_norm_rounding_of_every_total
  C  the sum the F.normalize pass installs        test_normalize_pass_*, test_three_chained_*, test_*_rows_*, test_exp3_step_*
  D  the incremental digit deltas                 test_apply_*
  E  the reward chain at its rounding points      test_update_chain_*
  F  normalized_edata, the exp3_weights setter    test_normalized_edata_*, test_setter_*"""
import ctypes as C
import random
from fractions import Fraction

import pytest
import torch

import exp3_fixed_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0x4049          # 3.140625: what surrounds a row under test
I16, I32, I64 = torch.int16, torch.int32, torch.int64


def _lib():
    from bliss_gnn_amd import _lib
    return _lib


def _call(name, *args):
    lib = _lib()
    lib.check(getattr(lib.lib, name)(*args), name)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _on_device(bits, off, dev):
    """The patterns as a bf16 row that starts ``off`` elements past a 16-byte boundary, guard patterns on both sides.
    Returns (whole buffer, the row as a view of it)."""
    n = bits.numel()
    buf = torch.full((off + n + 11,), GUARD, dtype=I64)
    buf[off:off + n] = bits
    w = R.bf(buf).to(dev)
    assert w.data_ptr() % 16 == 0
    return w, w[off:off + n]


def _guards_intact(w, off, n):
    b = R.bits_of(w)
    return bool((b[:off] == GUARD).all()) and bool((b[off + n:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------------------------------------------------
def test_row_sum_of_every_pattern_below_2_24(cuda):
    """value(row_sum) == sum(floor(x * 2^64)): zero, subnormals, values below 2^-64 (truncated to 0), mantissas that straddle
    two digits, the unreduced top digit; ascending then descending, off 16-byte alignment, short rows."""
    row = R.row_a()
    rows = [(row, off // 2) for off in R.ROW_A_BYTE_OFFSETS] + [(R.spread(row, n), 0) for n in R.ROW_A_LENGTHS]
    rows += [(R.spread(row, 65), 1), (row[:1], 5)]
    keep, sums = [], []
    for bits, off in rows:
        w, r = _on_device(bits, off, cuda)
        rs = torch.full((3 * R.SLOTS,), 0x5a5a5a5a5a, dtype=I64, device=cuda)          # bliss_row_sum starts from zero itself
        _call("bliss_row_sum", r.data_ptr(), r.numel(), rs.data_ptr(), _st())
        keep.append(w)
        sums.append(rs)
    torch.cuda.synchronize()
    for (bits, off), rs in zip(rows, sums):
        assert R.limb_value(rs) == R.exact_sum(bits), (bits.numel(), off)


def test_row_sum_carries_past_32_bits_in_the_top_limb(cuda):
    w = R.bf(torch.full((R.ROW_A_BIG,), R.TOP, dtype=I64)).to(cuda)
    rs = torch.zeros(3 * R.SLOTS, dtype=I64, device=cuda)
    _call("bliss_row_sum", w.data_ptr(), w.numel(), rs.data_ptr(), _st())
    torch.cuda.synchronize()
    assert R.limb_value(rs) == R.ROW_A_BIG * R.term(R.TOP) == R.exact_sum(w.cpu())
    top = rs.cpu().view(R.SLOTS, 3)[:, 2]
    assert int(top.sum()) >= 2 ** 32 and int((top != 0).sum()) == R.SLOTS               # all replicas carry it


# ---------------------------------------------------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------------------------------------------------
def test_norm_rounding_of_every_total(cuda):
    """limbs_to_bf16 through bliss_exp3_normalize_global on the row [1.0]: the norm is the bf16 NEAREST to total / 2^64
    (ties to even, the carry into the next binade, tiny and huge totals), whether the total sits canonically in replica 0
    or is scattered over all replicas with mixed signs and digits far outside 32 bits."""
    totals = R.totals_b()
    rng = random.Random(9)
    enc = [R.encode_canonical(t) for t in totals] + [R.encode_scattered(t, rng) for t in totals] + [R.encode_canonical(-1)]
    tot = totals + totals + [-1]
    N = len(enc)
    limbs = torch.stack(enc).to(cuda)
    rows = torch.full((N, 8), GUARD, dtype=I64)
    col = torch.arange(N) % 8
    rows[torch.arange(N), col] = R.ONE
    rows = R.bf(rows).to(cuda)
    row_sum = torch.full((N, 3 * R.SLOTS), 7, dtype=I64, device=cuda)
    scratch = torch.zeros(N, 98, dtype=I64, device=cuda)
    norm_out = torch.full((N,), -1.0, dtype=R.BF, device=cuda)
    st = _st()
    p_l, p_w, p_rs, p_sc, p_no = limbs.data_ptr(), rows.data_ptr(), row_sum.data_ptr(), scratch.data_ptr(), norm_out.data_ptr()
    fn, check = _lib().lib.bliss_exp3_normalize_global, _lib().check
    for i in range(N):
        check(fn(p_w + 2 * (8 * i + int(col[i])), 1, p_rs + 8 * 96 * i, p_l + 8 * 96 * i, p_sc + 8 * 98 * i, p_no + 2 * i, st),
              "bliss_exp3_normalize_global")
    torch.cuda.synchronize()

    memo = {}
    want_norm = torch.tensor([memo.setdefault(t, R.nearest_bf16(Fraction(t, 2 ** 64))) if t >= 0 else 0 for t in tot])
    got_norm, sc = R.bits_of(norm_out), scratch.cpu()
    bad = torch.nonzero(got_norm != want_norm).flatten().tolist()
    assert not bad, [(hex(tot[i]), hex(int(got_norm[i])), hex(int(want_norm[i])), "scattered" if i >= len(totals) else "canonical") for i in bad[:8]]
    assert torch.equal(sc[:, 0] & 0xffff, want_norm)
    skip = want_norm == R.ONE
    assert torch.equal((sc[:, 0] >> 16) & 1, skip.to(I64)) and int(skip.sum()) >= 4
    assert int(sc[:, 1:].abs().sum()) == 0                                                # ticket and staging sums back at zero

    # the element: 1.0 / max(norm, 1e-12) by torch's bf16 division; everything around it untouched
    want_el = torch.where(skip, R.bf([R.ONE]), R.bf([R.ONE]) / R.bf(want_norm).clamp_min(1e-12))
    got = R.bits_of(rows)
    assert torch.equal(got[torch.arange(N), col], R.bits_of(want_el))
    got[torch.arange(N), col] = GUARD
    assert bool((got == GUARD).all())
    # its exact sum, and no error bit, whenever it is below 2^24 (an element of 2^24 or more is refused: FIXED_RANGE)
    ok = R.below_2_24(want_el)
    err = sc[:, 0] >> 20
    neg = N - 1
    assert int(err[neg]) & R.ERR_FIXED_RANGE and int(got_norm[neg]) == 0                   # a negative total: norm 0, flagged
    ok[neg] = False
    assert bool((err[ok] == 0).all()) and int(ok.sum()) > N // 2
    assert bool((err[~ok] == R.ERR_FIXED_RANGE).all())
    rs, el_bits = row_sum.cpu(), R.bits_of(want_el).tolist()
    for i in range(N):
        if skip[i]:
            assert bool((rs[i] == 7).all()), i                                             # norm 1.0: nothing is touched
        elif ok[i]:
            assert R.limb_value(rs[i]) == R.term(el_bits[i]), (i, hex(tot[i]))


# ---------------------------------------------------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------------------------------------------------
def _normalize_global(bits, nb, off, dev, limbs=None):
    """One bliss_exp3_normalize_global call on the row; returns what it left behind."""
    w, r = _on_device(bits, off, dev)
    limbs = (R.encode_canonical(R.norm_total(nb)) if limbs is None else limbs).to(dev)
    row_sum = torch.full((3 * R.SLOTS,), 7, dtype=I64, device=dev)
    scratch = torch.zeros(98, dtype=I64, device=dev)
    norm_out = torch.full((1,), -1.0, dtype=R.BF, device=dev)
    _call("bliss_exp3_normalize_global", r.data_ptr(), r.numel(), row_sum.data_ptr(), limbs.data_ptr(), scratch.data_ptr(),
          norm_out.data_ptr(), _st())
    torch.cuda.synchronize()
    return dict(buf=w, row=R.bits_of(r), off=off, n=bits.numel(), row_sum=row_sum.cpu(), scratch=scratch.cpu(), norm=int(R.bits_of(norm_out)[0]))


def _check_pass(res, bits, nb, tag, err=0):
    want = R.bits_of(R.quotient(R.bf(bits), nb))
    assert res["norm"] == nb and int(res["scratch"][0]) & 0xffff == nb, tag
    assert (int(res["scratch"][0]) >> 16) & 1 == int(nb == R.ONE), tag
    bad = torch.nonzero(res["row"] != want).flatten()
    assert bad.numel() == 0, (tag, [(hex(int(bits[i])), hex(int(res["row"][i])), hex(int(want[i]))) for i in bad[:6].tolist()])
    assert int(res["scratch"][0]) >> 20 == err, (tag, int(res["scratch"][0]) >> 20)
    assert int(res["scratch"][1:].abs().sum()) == 0, tag                                  # ticket and staging sums back at zero
    assert _guards_intact(res["buf"], res["off"], res["n"]), tag
    if nb == R.ONE:
        assert bool((res["row_sum"] == 7).all()), tag                                     # skipped: the sum is not touched
    elif err == 0:
        assert R.limb_value(res["row_sum"]) == R.exact_sum(want), tag


@pytest.mark.parametrize("norm", R.NORMS_C)
def test_normalize_pass_installs_the_exact_sum(cuda, norm):
    """After the one-launch F.normalize pass: the row is torch's quotient AND row_sum is the exact sum of that row, whether an
    element went through the seven LDS counters (two at a time), the table with the general digits, or the division."""
    nb = R.norm_bits(norm)
    for kind, bits in (("all", R.row_c(nb)), ("interleaved", R.interleaved_c(nb))):
        for off in R.OFFSETS_C:
            _check_pass(_normalize_global(bits, nb, off, cuda), bits, nb, (norm, kind, off))


@pytest.mark.parametrize("norm", R.LENGTH_NORMS_C)
def test_normalize_pass_short_rows_and_workgroup_counts(cuda, norm):
    """One to four workgroups, rows with no full 16-byte vector, a head and a tail around the vectors."""
    nb = R.norm_bits(norm)
    full = R.row_c(nb)
    for n in R.LENGTHS_C:
        for off in (0, 3):
            bits = R.spread(full, n)
            _check_pass(_normalize_global(bits, nb, off, cuda), bits, nb, (norm, n, off))


@pytest.mark.parametrize("norm", R.SMALL_NORMS_C)
def test_normalize_pass_flags_a_quotient_of_2_24(cuda, norm):
    nb = R.norm_bits(norm)
    bits = R.out_of_range_c(nb)
    _check_pass(_normalize_global(bits, nb, 0, cuda), bits, nb, norm, err=R.ERR_FIXED_RANGE)


def test_three_chained_normalize_calls(cuda):
    """bliss_exp3_normalize three times on one row: the norm of call k+1 comes from the sum call k installed."""
    bits = R.row_a()
    w, r = _on_device(bits, 1, cuda)
    row_sum = R.encode_canonical(R.exact_sum(bits)).to(cuda)
    scratch = torch.zeros(98, dtype=I64, device=cuda)
    norm_out = torch.full((1,), -1.0, dtype=R.BF, device=cuda)
    for k, (nb, want) in enumerate(R.chained_reference(bits, 3)):
        _call("bliss_exp3_normalize", r.data_ptr(), r.numel(), row_sum.data_ptr(), scratch.data_ptr(), norm_out.data_ptr(), _st())
        torch.cuda.synchronize()
        assert int(R.bits_of(norm_out)[0]) == nb, (k, hex(nb))
        assert torch.equal(R.bits_of(r), want), k
        assert R.limb_value(row_sum) == R.exact_sum(want), k
        sc = scratch.cpu()
        assert int(sc[0]) == nb | (int(nb == R.ONE) << 16) and int(sc[1:].abs().sum()) == 0, k
    assert _guards_intact(w, 1, bits.numel())


def _exp3_block(**kw):
    rec = _lib().Exp3Block()
    for k, v in kw.items():
        setattr(rec, k, v)
    return rec


def test_normalize_global_rows_three_rows_in_one_launch(cuda):
    """bliss_exp3_normalize_global_rows, limb_stride 100: every row ends as its single-row call does."""
    n, stride = 6149, 100
    nbs = [R.norm_bits(x) for x in R.LENGTH_NORMS_C]
    rows = [R.spread(R.row_c(nb), n) for nb in nbs]
    limbs = torch.full((3 * stride,), 0x123456789abc, dtype=I64)                          # (what lies between the rows' limbs is not read)
    for i, nb in enumerate(nbs):
        limbs[i * stride:i * stride + 96] = R.encode_scattered(R.norm_total(nb), random.Random(i))
    limbs = limbs.to(cuda)
    dev = [_on_device(b, off, cuda) for b, off in zip(rows, (0, 1, 5))]
    row_sum = torch.full((3, 96), 7, dtype=I64, device=cuda)
    scratch = torch.zeros(3, 98, dtype=I64, device=cuda)
    norm_out = torch.full((3,), -1.0, dtype=R.BF, device=cuda)
    recs = (_lib().Exp3Block * 3)(*[_exp3_block(w_pos=dev[i][1].data_ptr(), row_sum=row_sum[i].data_ptr(), scratch=scratch[i].data_ptr(),
                                                norm_out=norm_out[i:].data_ptr()) for i in range(3)])
    _call("bliss_exp3_normalize_global_rows", recs, 3, n, limbs.data_ptr(), stride, _st())
    torch.cuda.synchronize()
    for i, (nb, off) in enumerate(zip(nbs, (0, 1, 5))):
        res = dict(buf=dev[i][0], row=R.bits_of(dev[i][1]), off=off, n=n, row_sum=row_sum[i].cpu(), scratch=scratch[i].cpu(),
                   norm=int(R.bits_of(norm_out)[i]))
        _check_pass(res, rows[i], nb, ("rows", i))


# ---------------------------------------------------------------------------------------------------------------------
# E (and the two-block step of C, which runs on the same blocks)
# ---------------------------------------------------------------------------------------------------------------------
class _DevBlock:
    """An exp3_fixed_ref.UpdateBlock on the device."""

    def __init__(self, blk, dev, row=None):
        i32 = lambda t: t.to(I32).to(dev)
        self.blk = blk
        self.g_indptr = blk.g_indptr.to(dev)
        self.graph = _lib().Graph(self.g_indptr.data_ptr(), 0, 0, blk.g_indptr.numel() - 1, blk.E)
        self.indptr, self.src, self.dst, self.pos, self.dst_nid = i32(blk.indptr), i32(blk.src), i32(blk.dst), i32(blk.pos), i32(blk.dst_nid)
        self.q, self.node_prob, self.embed_norm, self.alpha, self.edge_w = (t.to(dev) for t in (blk.q_ij, blk.node_prob, blk.embed_norm, blk.alpha, blk.edge_w))
        self.row0 = blk.row if row is None else row
        self.buf, self.row = _on_device(R.bits_of(self.row0), 1, dev)
        self.row_sum = R.encode_canonical(R.exact_sum(self.row0)).to(dev)
        self.n_edges = torch.tensor([blk.B], dtype=I32, device=dev)
        self.rewards = torch.full((blk.B,), -1.0, dtype=R.BF, device=dev)
        self.factor = torch.full((blk.B,), -1.0, dtype=R.BF, device=dev)
        self.err = torch.zeros(1, dtype=I32, device=dev)


def _run_update(blk, dev, through_edge_w):
    d = _DevBlock(blk, dev)
    _call("bliss_exp3_update", C.byref(d.graph), d.edge_w.data_ptr() if through_edge_w else 0, d.row.data_ptr(), d.row_sum.data_ptr(),
          d.indptr.data_ptr(), d.src.data_ptr(), d.dst.data_ptr(), d.pos.data_ptr(), d.q.data_ptr(), d.node_prob.data_ptr(),
          d.embed_norm.data_ptr(), 0 if through_edge_w else d.alpha.data_ptr(), d.dst_nid.data_ptr(), blk.dst_nid.numel(),
          d.n_edges.data_ptr(), blk.B, float(torch.tensor(blk.delta, dtype=torch.float32)), d.rewards.data_ptr(), d.factor.data_ptr(), 1,
          d.err.data_ptr(), _st())
    torch.cuda.synchronize()
    return d


def _first_diffs(blk, ok, got, want):
    return [(i, hex(int(R.bits_of(got)[i])), hex(int(R.bits_of(want)[i])),
             {k: float(getattr(blk, k)[i]) for k in ("alpha", "q_ij", "embed_norm", "node_prob", "w_old")},
             int(blk.indptr.diff()[blk.dst[i]]), int(blk.g_indptr.diff()[blk.dst_nid[blk.dst[i]]]))
            for i in torch.nonzero(~ok).flatten()[:5].tolist()]


@pytest.mark.parametrize("through_edge_w", [False, True], ids=["alpha_in", "edge_w"])
@pytest.mark.parametrize("delta", R.E_LISTS["delta"])
def test_update_chain_at_its_rounding_points(cuda, delta, through_edge_w):
    """rewards, factors and new weights of k_exp3_update have the reference's bits with every operand of the chain at its
    edges (zeros, tiny and huge values, the bf16 ties of the two degrees, the int -> float -> bf16 double rounding of the
    graph in-degree); the non-finite flag follows the reference; on the finite cases the incremental sum is exact."""
    full, finite = R.update_blocks()[delta]
    for blk, all_finite in ((full, False), (finite, True)):
        rewards, ex, row, _ = blk.reference()
        d = _run_update(blk, cuda, through_edge_w)
        for name, got, want in (("rewards", d.rewards.cpu(), rewards), ("factor", d.factor.cpu(), ex), ("weight", d.row.cpu()[blk.pos], row[blk.pos])):
            ok = R.same_bits_or_nan(got, want)
            assert bool(ok.all()), (name, int((~ok).sum()), _first_diffs(blk, ok, got, want))
        assert bool(R.same_bits_or_nan(d.row.cpu(), row).all()) and _guards_intact(d.buf, 1, blk.E)
        err = int(d.err.item())
        ref_nonfinite = not bool(torch.isfinite(row.float()).all())
        assert ref_nonfinite == (not all_finite)
        assert bool(err & R.ERR_NONFINITE) == ref_nonfinite, err
        if all_finite:
            assert err == 0
            assert R.limb_value(d.row_sum) == R.exact_sum(row)


def test_exp3_step_two_blocks_update_then_normalize(cuda):
    """bliss_exp3_step with two blocks (one reads alpha through edge_w[pos], one from its own array): each row ends with the
    bits of update-then-F.normalize and with the exact sum of those bits."""
    _, blk = R.update_blocks()[0.01]
    row1 = blk.row.clone()
    row1[blk.row == 2.0 ** -12] = 2.0 ** -3
    ds = [_DevBlock(blk, cuda), _DevBlock(blk, cuda, row=row1)]
    scratch = torch.zeros(2, 98, dtype=I64, device=cuda)
    norm_out = torch.full((2,), -1.0, dtype=R.BF, device=cuda)
    err = torch.zeros(1, dtype=I32, device=cuda)
    recs = (_lib().Exp3Block * 2)(*[_exp3_block(
        w_pos=d.row.data_ptr(), row_sum=d.row_sum.data_ptr(), scratch=scratch[i].data_ptr(), norm_out=norm_out[i:].data_ptr(),
        blk_indptr=d.indptr.data_ptr(), blk_src=d.src.data_ptr(), blk_dst=d.dst.data_ptr(), blk_pos=d.pos.data_ptr(), q_ij=d.q.data_ptr(),
        node_prob=d.node_prob.data_ptr(), embed_norm=d.embed_norm.data_ptr(), alpha_or_null=d.alpha.data_ptr() if i else 0,
        dst_nid=d.dst_nid.data_ptr(), n_edges_dev=d.n_edges.data_ptr(), rewards_out=d.rewards.data_ptr(), edges_bound=blk.B) for i, d in enumerate(ds)])
    _call("bliss_exp3_step", C.byref(ds[0].graph), ds[0].edge_w.data_ptr(), recs, 2, float(torch.tensor(0.01, dtype=torch.float32)), err.data_ptr(), _st())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for i, d in enumerate(ds):
        rewards, _, row, _ = blk.reference(row=d.row0)
        nb = R.nearest_bf16(Fraction(R.exact_sum(row), 2 ** 64))
        assert nb != R.ONE
        assert bool(R.same_bits_or_nan(d.rewards.cpu(), rewards).all()), i
        res = dict(buf=d.buf, row=R.bits_of(d.row), off=1, n=blk.E, row_sum=d.row_sum.cpu(), scratch=scratch[i].cpu(), norm=int(R.bits_of(norm_out)[i]))
        _check_pass(res, R.bits_of(row), nb, ("step", i))


# ---------------------------------------------------------------------------------------------------------------------
# D
# ---------------------------------------------------------------------------------------------------------------------
def _apply(bits, pos, fac, n_live, dev, start_sum=None):
    w, r = _on_device(bits, 1, dev)
    row_sum = R.encode_canonical(R.exact_sum(bits) if start_sum is None else start_sum).to(dev)
    err = torch.zeros(1, dtype=I32, device=dev)
    pos_d, fac_d, n_dev = pos.to(I32).to(dev), fac.to(dev), torch.tensor([n_live], dtype=I32, device=dev)
    _call("bliss_exp3_apply", r.data_ptr(), row_sum.data_ptr(), pos_d.data_ptr(), fac_d.data_ptr(), n_dev.data_ptr(), pos.numel(), err.data_ptr(), _st())
    torch.cuda.synchronize()
    return w, r, row_sum, int(err.item())


def test_apply_deltas_across_digit_boundaries(cuda):
    """digits(new) - digits(old) where a weight crosses a 32-bit digit boundary, drops below 2^-64, becomes subnormal or
    zero, or sits in the top binade below 2^24; the entries past the live count are not applied."""
    bits, pos, fac = R.apply_case()
    n_live = pos.numel() - 100
    w, r, row_sum, err = _apply(bits, pos, fac, n_live, cuda)
    want = R.bf(bits)
    live = pos[:n_live].long()
    want[live] = want[live] * fac[:n_live]
    assert torch.equal(R.bits_of(r), R.bits_of(want))
    assert torch.equal(R.bits_of(r)[pos[n_live:].long()], bits[pos[n_live:].long()])      # past the count: untouched
    assert R.limb_value(row_sum) == R.exact_sum(want)
    assert err == 0 and _guards_intact(w, 1, bits.numel())


@pytest.mark.parametrize("w_old,factor,flag", [(2.0 ** 23, 2.0, R.ERR_FIXED_RANGE), (3e38, 3.0, R.ERR_NONFINITE)])
def test_apply_flags_what_the_sum_cannot_hold(cuda, w_old, factor, flag):
    bits = R.bits_of(torch.tensor([0.5, w_old, 0.25], dtype=torch.float32).bfloat16())
    w, r, row_sum, err = _apply(bits, torch.tensor([1]), torch.tensor([factor]).bfloat16(), 1, cuda, start_sum=0)    # (3e38 has no digits)
    assert err & flag, err
    assert torch.equal(R.bits_of(r), R.bits_of(R.bf(bits) * torch.tensor([1.0, factor, 1.0]).bfloat16()))


def test_apply_ranks_two_ranks_against_the_sequential_product(cuda):
    """apply_updates_ranks, two ranks and two blocks: identical positions in both ranks, neighbours that share a 32-bit word;
    against the products taken rank after rank on the CPU and the exact sum of the result."""
    import bliss_gnn_amd as bg
    rows, lists, want = R.ranks_case()
    E = rows.shape[1]
    g = bg.Graph(torch.tensor([0, E], dtype=I64, device=cuda), torch.zeros(E, dtype=I32, device=cuda))
    bounds = [9100, 9100]
    offs, tot = [0, bounds[0]], sum(bounds)
    n_fac = (tot + 1) // 2
    n_pad = (tot + n_fac + 2 + 3) // 4 * 4
    gath = torch.zeros(2 * n_pad, dtype=I32)
    for r in range(2):
        base = gath[r * n_pad:(r + 1) * n_pad]
        for b in range(2):
            p, f = lists[r][b]
            n = p.numel()
            assert n < bounds[b]
            base[offs[b]:offs[b] + n] = p
            base[tot:tot + n_fac].view(R.BF)[offs[b]:offs[b] + n] = f
            base[tot + n_fac + b] = n
    s = bg.PoissonBanditLadiesSampler([10, 10], eta=0.1)
    s._bind(g)
    s.exp3_weights = R.bf(rows).to(cuda)
    s.apply_updates_ranks([0, 1], gath.to(cuda), n_pad, 2, offs, [2 * tot + o for o in offs], [tot + n_fac, tot + n_fac + 1], bounds)
    torch.cuda.synchronize()
    s.check_errors()
    assert torch.equal(R.bits_of(s._w_pos), want)
    for b in range(2):
        assert R.limb_value(s._row_sum[b]) == R.exact_sum(want[b]), b
    assert int(s._apply_bar.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# F
# ---------------------------------------------------------------------------------------------------------------------
def test_normalized_edata_at_the_degree_roundings(cuda):
    from oracle import bliss_oracle as bo
    indptr = torch.tensor((0,) + R.DEGREES_F, dtype=I64).cumsum(0)
    E = int(indptr[-1])
    want = bo.normalized_edata(bo.CSC(indptr, torch.zeros(E, dtype=I32)))
    ip = indptr.to(cuda)
    out = R.bf(torch.full((E + 8,), GUARD, dtype=I64)).to(cuda)
    g = _lib().Graph(ip.data_ptr(), 0, 0, len(R.DEGREES_F), E)
    _call("bliss_normalized_edata", C.byref(g), out.data_ptr(), _st())
    torch.cuda.synchronize()
    assert torch.equal(R.bits_of(out[:E]), R.bits_of(want))
    assert bool((R.bits_of(out[E:]) == GUARD).all())


def _bound_sampler(E, dev):
    import bliss_gnn_amd as bg
    g = bg.Graph(torch.tensor([0, E], dtype=I64, device=dev), torch.zeros(E, dtype=I32, device=dev))
    s = bg.PoissonBanditLadiesSampler([10, 10], eta=0.1)
    s._bind(g)
    return s


@pytest.mark.parametrize("bad", [-2.0 ** -130, float("inf"), float("nan"), 2.0 ** 24, -1.0])
def test_setter_refuses_what_the_row_sum_cannot_hold(cuda, bad):
    """exp3_weights = ... is where outside weights enter the state; bliss_row_sum has no error word, so a weight that is
    negative, non-finite or 2^24 and more has to be refused there (it used to give a silently wrong sum)."""
    s = _bound_sampler(300, cuda)
    w = torch.full((2, 300), 0.25, dtype=R.BF, device=cuda)
    w[1, 77] = bad
    with pytest.raises(ValueError):
        s.exp3_weights = w


def test_setter_takes_the_largest_weight_and_sums_exactly(cuda):
    s = _bound_sampler(300, cuda)
    w = torch.full((2, 300), 2.0 ** 24 - 2.0 ** 16, dtype=R.BF)
    w[1, ::3] = 2.0 ** -64
    w[1, 1::3] = 0.0
    w[1, 5] = -0.0
    s.exp3_weights = w.to(cuda)
    torch.cuda.synchronize()
    assert torch.equal(R.bits_of(s.exp3_weights), R.bits_of(w))
    for l in range(2):
        assert R.limb_value(s._row_sum[l]) == R.exact_sum(w[l].abs()), l
    assert R.limb_value(s._row_sum[0]) == 300 * (0xff << 80)
