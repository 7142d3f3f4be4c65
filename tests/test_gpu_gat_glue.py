"""GPU suite (-m gpu): csrc/gat_glue.hip forward and backward against the NumPy restatement
(tests/gat_glue_ref.py) and, at p = 0, bit for bit against torch's bf16 tensor ops on the device; the edge-wise head mean.

Against the restatement the keyed mask (which elements are zero) must agree exactly.  The values may differ where ELU ran: the
device takes expm1 / exp in fp32, the restatement in fp64, so a stored ELU value can land on the neighbouring bf16 number (one
spacing, at most 2^-7 of its magnitude); a head mean passes that on once, the final rounding and the dropout product each add
one more spacing: |got - want| <= 3 * 2^-7 * scale * (largest |value| that enters the element).  At p = 0 torch's own kernels
are the exact reference (torch.equal).

Every operand row at or past the live count is NaN and every buffer the launch allocates is pre-filled with NaN: rows past the
count must come out as exact zeros and no NaN may reach a live row.  Planted faults these cases catch: the mask index taken
with the capacity's row stride, or the head mean's width, instead of the logical width (mask mismatch at (4, 256) and (1, 7));
the add left unrounded before ELU (torch.equal at p = 0); the 16-byte path taken at D = 7 (misaligned rows: wrong values); the
zero fill of padding rows skipped (NaN stays); the ELU derivative taken from the output (torch.equal of the backward)."""
import numpy as np
import pytest
import torch

import gat_glue_ref as ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [(1, 7, True), (2, 8, False), (2, 8, True), (4, 256, False), (4, 256, True)]
ROWS = [(rows, live) for rows in (1, 33, 65) for live in sorted({0, 1, rows - 1, rows})]


@pytest.fixture
def nan_empty(monkeypatch):
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float("nan"))
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)


def _np(t):
    return t.detach().float().cpu().numpy()


def _dev(a, cuda, live):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(BF)
    t[live:] = float("nan")
    return t.to(cuda)


def _close(got, want, mag, scale, what):
    bound = 3 * 2.0 ** -7 * float(scale) * mag + 2.0 ** -130
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / bound).max()), int((err > 0).sum()))
    assert np.array_equal(got == 0, want == 0) or (np.abs(want[(got == 0) != (want == 0)]) < 2.0 ** -120).all(), what + ": mask"
    return int((err > 0).sum())


@pytest.mark.parametrize("rows,live", ROWS)
@pytest.mark.parametrize("H,D,mean", SHAPES)
def test_glue_forward_and_backward(cuda, nan_empty, H, D, mean, rows, live):
    from bliss_gnn_amd import nn as bnn
    rng = np.random.default_rng(1000 * H + 10 * D + rows + live + int(mean))
    HD, width = H * D, (D if mean else H * D)
    rst = ref.rbf(rng.standard_normal((rows, HD)).astype(np.float32) * 2)
    res = ref.rbf(rng.standard_normal((rows, HD)).astype(np.float32))
    dout = ref.rbf(rng.standard_normal((rows, width)).astype(np.float32))
    n_dev = torch.tensor([live], dtype=torch.int32, device=cuda)
    mag_f = np.abs(rst) + np.abs(res) + 1.0                                     # |x| bounds |ELU(x)| (and 1 where x < 0)
    mag_out = mag_f.reshape(rows, H, D).max(1) if mean else mag_f
    for p in (0.0, 0.25):
        state = bnn.gat_drop_state(5, cuda) if p > 0 else None
        seed = state["seed"] if p > 0 else 0
        a, b = _dev(rst, cuda, live).requires_grad_(True), _dev(res, cuda, live).requires_grad_(True)
        out, pre = bnn.gat_glue(a, b, H, D, act=bnn.GLUE_ACT_ELU, head_mean=mean, p=p, state=state, rows_dev=n_dev.data_ptr(), want_pre=True)
        out.backward(_dev(dout, cuda, live))
        torch.cuda.synchronize()
        if p > 0:
            assert int(state["ctr"][0]) == 1                                    # the launch counter moved on behind the launch
        w_out, w_pre = ref.glue_fwd(rst, res, H, D, 1, mean, p=p, seed=seed, ctr=0, n_live=live)
        w_din = ref.glue_bwd(dout, rst, res, H, D, 1, mean, p=p, seed=seed, ctr=0, n_live=live)
        scale = float(ref.drop_scale(p)) if p > 0 else 1.0
        for name, got, want, mag in (("out", out, w_out, mag_out * scale), ("pre", pre, w_pre, mag_out),
                                     ("d rst", a.grad, w_din, np.tile(np.abs(dout) * scale, (1, H)) if mean else np.abs(dout) * scale)):
            g = _np(got)
            assert g.shape == want.shape and not g[live:].any(), (name, p, "rows past the count must be exact zeros")
            diff = _close(g[:live], want[:live], mag[:live], 1.0, "%s p=%g" % (name, p))
            print("GLUE", H, D, mean, rows, live, p, name, "elements off the restatement:", diff)
        assert torch.equal(a.grad.view(torch.int16), b.grad.view(torch.int16))   # the residual's pass-through
        if p == 0:                                                              # torch's bf16 ops on the device, live rows
            ta, tb = a.detach()[:live].clone().requires_grad_(True), b.detach()[:live].clone().requires_grad_(True)
            y = torch.nn.functional.elu(ta + tb).view(live, H, D)
            z = y.mean(1) if mean else y.flatten(1)
            z.backward(_dev(dout, cuda, rows)[:live])
            if H <= 2 or not mean:                                              # (above two heads mean(1)'s fp32 order is torch's own)
                assert torch.equal(out[:live], z.detach()) and torch.equal(pre[:live], z.detach()), "forward bits"
                assert torch.equal(a.grad[:live], ta.grad), "backward bits"


@pytest.mark.parametrize("rows,live", ROWS)
@pytest.mark.parametrize("width", [7, 24, 602])
def test_dropout_only_mode(cuda, nan_empty, width, rows, live):
    """feat_drop on gathered feature rows: mask and scale of the restatement, exact (no transcendental on the way)."""
    from bliss_gnn_amd import nn as bnn
    rng = np.random.default_rng(width + rows + live)
    x = ref.rbf(rng.standard_normal((rows, width)).astype(np.float32))
    g = ref.rbf(rng.standard_normal((rows, width)).astype(np.float32))
    n_dev = torch.tensor([live], dtype=torch.int32, device=cuda)
    state = bnn.gat_drop_state(2, cuda)
    xd = _dev(x, cuda, live).requires_grad_(True)
    for launch in range(2):                                                     # the second launch draws with counter 1
        xd.grad = None
        out = bnn.gat_feat_drop(xd, 0.1, state, rows, n_dev.data_ptr())
        out.backward(_dev(g, cuda, live))
        want, _ = ref.glue_fwd(x, None, 1, width, 0, False, p=0.1, seed=state["seed"], ctr=launch, n_live=live)
        dwant = ref.glue_bwd(g, None, None, 1, width, 0, False, p=0.1, seed=state["seed"], ctr=launch, n_live=live)
        assert np.array_equal(_np(out), want) and np.array_equal(_np(xd.grad), dwant), launch
    assert int(state["ctr"][0]) == 2


@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("B,live", [(1, 1), (300, 0), (300, 299), (300, 300), (5000, 4097)])
def test_edge_head_mean_is_bounded_and_leaves_the_tail(cuda, H, B, live):
    from bliss_gnn_amd import nn as bnn
    rng = np.random.default_rng(H + B)
    e = ref.rbf(rng.standard_normal((B, H)).astype(np.float32) * 3)
    ed = _dev(e, cuda, live)
    n_dev = torch.tensor([live], dtype=torch.int32, device=cuda)
    real = torch.empty
    try:
        torch.empty = lambda *a, **kw: real(*a, **kw).fill_(7.0)                # the tail keeps what the buffer held
        out = bnn.gat_head_mean(ed, B, n_dev.data_ptr())
    finally:
        torch.empty = real
    got = _np(out)
    assert np.array_equal(got[:live], ref.head_mean(e)[:live]) and (got[live:] == 7.0).all()
    if H <= 2:
        assert torch.equal(out[:live], ed[:live].mean(1))
