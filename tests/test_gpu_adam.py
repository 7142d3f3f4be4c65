"""GPU suite: the one-launch Adam (csrc/optim.hip: k_adam, bliss_adam_step; optim.Adam) per element against fp64, one step at
a time from planted states, at the tensor sizes and tensor lists where the workgroup-to-tensor mapping can slip.

The yardstick is bounds.adam_terms in float64 on the same bf16 (p, g, m, v), with lr, the betas, eps and the weight decay
rounded to the fp32 values the C ABI receives and the step count taken from state[0]:

    |got - ref| <= 1 ulp_bf16(ref) + k 2^-24 mag          for every element of p', exp_avg' and exp_avg_sq'

k_ulp = 1 for all three: each stored value is rounded once, half a bf16 spacing of an fp32 value that may sit one binade above
ref.  The magnitudes are the formulas on the absolute values of their terms (bounds.adam_terms), and k counts the fp32
roundings in front of the store, each 2^-24 relative to the magnitude of what it rounds (-ffp-contract=off: nothing fuses):

  exp_avg' = m + (gw - m)(1 - b1),  gw = g + wd p.   1 - b1 is exact in fp32 (b1 in [1/2, 1]).  wd p and the sum: 2, relative
    to |g| + wd |p|;  gw - m: 1;  the product: 1;  the final sum: 1, relative to mag_m itself.  With (1 - b1)(|g| + wd |p| +
    |m|) <= mag_m: k = 5.  mag_m = |m| + (1 - b1)(|g| + wd |p| + |m|) is what makes a first moment that crosses zero testable:
    m + (g - m) 0.1 may cancel to nothing, and its fp32 error does not shrink with it.
  exp_avg_sq' = b2 v + (1 - b2) gw^2.   gw carries 2 (as above), its square twice that: 4;  the square, the two products and the
    sum: 4.  k = 8 on mag_v = b2 v + (1 - b2)(|g| + wd |p|)^2, which is v' itself unless g and wd p cancel.
  p' = p - lr / bc1 * (m' / denom),  denom = sqrt(v') / sqrt(bc2) + eps,  bc = 1 - b^t,  t = state[0] + 1.
    powf is good to 2 ulp (4 units) of b^t and the subtraction adds 1 relative to bc: bc carries C(b, t) = 1 + 4 b^t / (1 - b^t)
    -- 37 for b1 at t = 1, 4001 for b2 at t = 1 (2^-24 / (t 1e-3) of cancellation, as a count of units), 1 once b^t has died
    away (t = 1e5).  m': 5.  denom: half of v' (4), sqrt (2), sqrt(bc2) (C(b2, t) / 2 + 2), the division (3), + eps (1).  lr / bc1:
    C(b1, t) + 3.  m' / denom: 3.  The product and the final subtraction: 2.  k = 25 + C(b1, t) + C(b2, t) / 2 on
    mag_p = |p| + lr / bc1 * mag_m / denom * (mag_v / v'): the update evaluated on magnitudes, equal to |p| + |update| unless
    m' or g + wd p cancels.
  With v = 0 and g = 0 the denominator is eps alone (exact); with v ~ 1e-12 and g ~ 1e-6 every value stays a normal fp32 and bf16
  number (v' >= 5e-13).

A tensor of no elements has no storage (a null data pointer); bliss_adam_step used to refuse the whole list for it.  It now
accepts null pointers where numel is 0; test_single_steps_from_planted_states has such a tensor in the middle of its list and
test_tensor_list_boundaries one at the end.

Measured on the MI355X, worst ratio to the bound over every case of test_single_steps_from_planted_states, by step count before
the update -- p' / exp_avg' / exp_avg_sq':
    0: 0.492 / 0.500 / 0.500    1: 0.496 / 0.500 / 0.500    6: 0.499 / 0.500 / 0.500    999 and 99 999: 0.500 / 0.500 / 0.500
i.e. every stored value is the correctly rounded bf16 of the fp64 value up to the rounding's own half ulp.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

from bounds import ADAM_SIZES, adam_case, adam_k, adam_terms, assert_within   # noqa: E402

B1, B2, EPS = 0.9, 0.999, 1e-8


def _planted(cases, step, lr, wd, cuda, grads=None):
    """An optimiser over the tensors of ``cases`` [(p, g, m, v) on the CPU] with its device state written directly: state[0] =
    step, exp_avg = m, exp_avg_sq = v.  ``grads``: what to hang on .grad instead of g (None entries: no gradient)."""
    from bliss_gnn_amd.optim import Adam
    ps = [torch.nn.Parameter(p.to(cuda)) for p, _, _, _ in cases]
    opt = Adam(ps, lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd)
    opt._state[0] = float(step)
    for i, (prm, (_, g, m, v)) in enumerate(zip(ps, cases)):
        gi = g.to(cuda) if grads is None else grads[i]
        if gi is not None and gi.dtype != prm.dtype and hasattr(prm, "grad_dtype"):
            prm.grad_dtype = None                                # (torch refuses a gradient of another dtype otherwise)
        prm.grad = gi
        opt.state[prm]["exp_avg"].copy_(m.to(cuda))
        opt.state[prm]["exp_avg_sq"].copy_(v.to(cuda))
    return ps, opt


def _ticket(opt):
    return int(opt._state.view(torch.int32)[2])


def _check(ps, opt, cases, step, lr, wd, what, worst=None):
    k = adam_k(step, B1, B2)
    for i, (prm, (p, g, m, v)) in enumerate(zip(ps, cases)):
        ref = adam_terms(p.to(prm.device), g.to(prm.device), m.to(prm.device), v.to(prm.device), step, lr, B1, B2, EPS, wd)
        st = opt.state[prm]
        for j, (name, got) in enumerate((("p", prm.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"]))):
            r = assert_within(got, ref[2 * j], ref[2 * j + 1], *k[name], "%s tensor %d %s %s'" % (what, i, tuple(p.shape), name))
            if worst is not None:
                worst[name] = max(worst.get(name, 0.0), r)


@pytest.mark.parametrize("v0", [0.0, 1e-12, 1e-4])
@pytest.mark.parametrize("g_scale", [1.0, 1e-2, 1e-6, 0.0])
@pytest.mark.parametrize("step", [0, 1, 6, 999, 99999])
def test_single_steps_from_planted_states(cuda, step, g_scale, v0):
    """One step from a planted state, for both learning rates, the three weight decays and first moments with the gradient's sign
    or against it, over tensors of 2047, 2048, 2049, 1, 4096, 4097, 0 and 256 x 602 elements in one list: every element of p,
    exp_avg and exp_avg_sq within its bound, the step count up by exactly 1, the ticket word 0."""
    worst = {}
    for m_sign in (1.0, -1.0):
        cases = [adam_case(shape, g_scale, m_sign, v0, 100 + si) for si, shape in enumerate(ADAM_SIZES)]
        for lr in (2e-3, 2e-5):
            for wd in (0.0, 0.01, 0.1):
                ps, opt = _planted(cases, step, lr, wd, cuda)
                opt.step()
                assert opt.step_count == step + 1 and _ticket(opt) == 0
                _check(ps, opt, cases, step, lr, wd, "step %d g %g v %g m %+d lr %g wd %g" % (step, g_scale, v0, m_sign, lr, wd), worst)
    print("step %d g %g v %g: worst p %.3f m %.3f v %.3f" % (step, g_scale, v0, worst["p"], worst["m"], worst["v"]))


def test_two_steps_in_a_row_count_two(cuda):
    """The count the kernel keeps on the device rises by exactly 1 per call, and the second step's bias corrections follow it."""
    cases = [adam_case(shape, 1e-2, -1.0, 1e-4, 300 + si) for si, shape in enumerate(ADAM_SIZES)]
    ps, opt = _planted(cases, 6, 2e-3, 0.01, cuda)
    opt.step()
    assert opt.step_count == 7 and _ticket(opt) == 0
    mid = [(p.detach().cpu().clone(), c[1], opt.state[p]["exp_avg"].cpu().clone(), opt.state[p]["exp_avg_sq"].cpu().clone())
           for p, c in zip(ps, cases)]
    opt.step()
    assert opt.step_count == 8 and _ticket(opt) == 0
    _check(ps, opt, mid, 7, 2e-3, 0.01, "second step")


def test_tensor_list_boundaries(cuda):
    """32 tensors (BLISS_ADAM_MAX_TENSORS) of 1 .. 3000 elements, 2047 / 2048 / 2049 among them, the last of 0 elements; a 33rd is
    refused at construction.  A parameter in the middle without a gradient keeps its p, exp_avg and exp_avg_sq bits while its
    neighbours are updated correctly (the list the kernel sees then has 31 entries and other workgroup offsets)."""
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd.optim import Adam
    assert _lib.ADAM_MAX_TENSORS == 32
    sizes = [(i * 193 + 7) % 3000 + 1 for i in range(32)]
    sizes[3], sizes[4], sizes[5], sizes[17], sizes[30], sizes[31] = 2047, 2048, 2049, 1, 3000, 0
    cases = [adam_case((s,), 1e-2, -1.0, 1e-4, 500 + i) for i, s in enumerate(sizes)]
    ps, opt = _planted(cases, 6, 2e-3, 0.01, cuda)
    opt.step()
    assert opt.step_count == 7 and _ticket(opt) == 0
    _check(ps, opt, cases, 6, 2e-3, 0.01, "32 tensors")
    with pytest.raises(NotImplementedError):
        Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16, device=cuda)) for _ in range(33)], lr=2e-3)
    # a parameter in the middle (and the first, and the one before the empty last) without a gradient
    for missing in ([16], [0, 4, 30]):
        grads = [None if i in missing else c[1].to(cuda) for i, c in enumerate(cases)]
        ps, opt = _planted(cases, 6, 2e-3, 0.01, cuda, grads=grads)
        opt.step()
        assert opt.step_count == 7 and _ticket(opt) == 0
        keep = [i for i in range(32) if i not in missing]
        _check([ps[i] for i in keep], opt, [cases[i] for i in keep], 6, 2e-3, 0.01, "without a gradient on %s" % missing)
        for i in missing:
            st = opt.state[ps[i]]
            assert torch.equal(ps[i].detach().cpu().view(torch.int16), cases[i][0].view(torch.int16))
            assert torch.equal(st["exp_avg"].cpu().view(torch.int16), cases[i][2].view(torch.int16))
            assert torch.equal(st["exp_avg_sq"].cpu().view(torch.int16), cases[i][3].view(torch.int16))
    # no gradient anywhere: nothing happens, the count included
    ps, opt = _planted(cases, 6, 2e-3, 0.01, cuda, grads=[None] * 32)
    opt.step()
    assert opt.step_count == 6 and _ticket(opt) == 0


def test_gradients_in_fp32_or_not_contiguous_are_converted(cuda):
    """A gradient that arrives in fp32, or as a transposed view, is converted to contiguous bf16 (and left on .grad so); the
    step is the step on bf16(g)."""
    shapes = [(256, 602), (2049,), (41, 256)]
    cases = [adam_case(s, 1e-2, 1.0, 1e-4, 700 + i) for i, s in enumerate(shapes)]
    gen = torch.Generator().manual_seed(9)
    g32 = torch.randn(shapes[0], generator=gen) * 1e-2                       # fp32, not representable in bf16
    gt = (torch.randn(shapes[2][1], shapes[2][0], generator=gen) * 1e-2).bfloat16()
    grads = [g32.to(cuda), cases[1][1].to(cuda), gt.to(cuda).t()]
    assert not grads[2].is_contiguous()
    ps, opt = _planted(cases, 6, 2e-3, 0.01, cuda, grads=grads)
    opt.step()
    assert all(p.grad.dtype == torch.bfloat16 and p.grad.is_contiguous() for p in ps)
    cases[0] = (cases[0][0], g32.bfloat16(), cases[0][2], cases[0][3])
    cases[2] = (cases[2][0], gt.t().contiguous(), cases[2][2], cases[2][3])
    _check(ps, opt, cases, 6, 2e-3, 0.01, "converted gradients")


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4097])
def test_surrounding_memory_is_untouched(cuda, n):
    """p, exp_avg and exp_avg_sq as interior (contiguous) slices of larger buffers with sentinels on both sides, two such tensors
    in the list: every sentinel keeps its bits, the slices are updated correctly."""
    from bliss_gnn_amd.optim import Adam
    PAD = 4096
    cases = [adam_case((n,), 1e-2, -1.0, 1e-4, 800 + i) for i in range(2)]
    bufs = [[torch.full((n + 2 * PAD,), s, dtype=torch.bfloat16, device=cuda) for s in (-5.0, 3.0, 11.0, 13.0)] for _ in cases]
    ps = []
    for (p, g, m, v), (bp, bm, bv, bg) in zip(cases, bufs):
        bp[PAD:PAD + n], bm[PAD:PAD + n], bv[PAD:PAD + n], bg[PAD:PAD + n] = p.to(cuda), m.to(cuda), v.to(cuda), g.to(cuda)
        ps.append(torch.nn.Parameter(bp[PAD:PAD + n]))
        assert ps[-1].data_ptr() == bp.data_ptr() + 2 * PAD
    opt = Adam(ps, lr=2e-3, betas=(B1, B2), eps=EPS, weight_decay=0.01)
    opt._state[0] = 6.0
    for prm, (bp, bm, bv, bg) in zip(ps, bufs):
        prm.grad = bg[PAD:PAD + n]
        opt.state[prm]["exp_avg"], opt.state[prm]["exp_avg_sq"] = bm[PAD:PAD + n], bv[PAD:PAD + n]
    opt.step()
    assert opt.step_count == 7 and _ticket(opt) == 0
    _check(ps, opt, cases, 6, 2e-3, 0.01, "interior slices of %d" % n)
    for (_, g, _, _), row in zip(cases, bufs):
        for buf, s in zip(row, (-5.0, 3.0, 11.0, 13.0)):
            assert bool((buf[:PAD] == s).all()) and bool((buf[PAD + n:] == s).all())
        assert torch.equal(row[3][PAD:PAD + n].cpu().view(torch.int16), g.view(torch.int16))          # the gradient is read only


def test_captured_step_follows_the_learning_rate_on_replay(cuda):
    """One step() captured in a torch.cuda.graph and replayed three times, with param_groups[0]['lr'] changed and sync_lr() called
    between the replays, equals three eager steps with the same rates bit for bit -- parameters, both moments and the step
    count (learning rate and count live on the device: the graph holds neither)."""
    rates = [2e-3, 2e-5, 7e-4]
    shapes = [(2049,), (256, 602), (1,), (4097,)]
    cases = [adam_case(s, 1e-2, -1.0, 1e-4, 900 + i) for i, s in enumerate(shapes)]
    ps_e, opt_e = _planted(cases, 6, rates[0], 0.01, cuda)
    for lr in rates:
        opt_e.param_groups[0]["lr"] = lr
        opt_e.step()
    ps_g, opt_g = _planted(cases, 6, rates[0], 0.01, cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    torch.cuda.synchronize()
    assert opt_g.step_count == 6                                 # (the capture executed nothing)
    for lr in rates:
        opt_g.param_groups[0]["lr"] = lr
        opt_g.sync_lr()
        graph.replay()
    torch.cuda.synchronize()
    assert opt_g.step_count == opt_e.step_count == 9 and _ticket(opt_g) == 0
    for a, b in zip(ps_e, ps_g):
        assert torch.equal(a.detach().view(torch.int16), b.detach().view(torch.int16))
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_e.state[a][key].view(torch.int16), opt_g.state[b][key].view(torch.int16))
    # and the eager steps are the right ones: the third against fp64 from the state after two
    ps_c, opt_c = _planted(cases, 6, rates[0], 0.01, cuda)
    for lr in rates[:2]:
        opt_c.param_groups[0]["lr"] = lr
        opt_c.step()
    mid = [(p.detach().cpu().clone(), c[1], opt_c.state[p]["exp_avg"].cpu().clone(), opt_c.state[p]["exp_avg_sq"].cpu().clone())
           for p, c in zip(ps_c, cases)]
    _check(ps_g, opt_g, mid, 8, rates[2], 0.01, "third replay")
