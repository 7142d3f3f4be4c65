"""GPU suite (-m gpu): ``nn._GatLinear`` -- fc_src / res_fc of a GATv2 layer on the MFMA tile kernels in
output-column blocks of 256 -- forward, ``dW`` (``db``) and ``dX`` element by element against float64 on the same bf16 operands,
with the bound and constants of the SAGE MFMA edge-shape tests (tests/bounds.py):

    |got - ref| <= k_ulp * ulp_bf16(ref) + k_mag * 2^-8 * mag
    forward  dense_k(in + 1 bias);   dX  dense_k(H*D (+ H*D of the second Linear));   dW, db  dense_k(rows + 80 chunks).

Shapes: in_feats 100 (a K tail short of a 64-slab), 602, 1024; H*D 288 (one full block of 256 columns and a ragged one), 1024
(four blocks: dX walks sixteen 64-row slabs of W), 7; rows 1, 33, 65 with live counts {0, 1, rows - 1, rows} on the device.
Operand rows at or past the count are NaN, the buffers the node allocates are pre-filled with NaN: live results must not see
them, rows past the count must be exact zeros.

Planted faults each test catches (wrong numbers inside valid memory):
  forward  a column block's bias (or W) slice taken one block off -- columns 256 .. 287 of H*D = 288 get block 0's bias;
           the second argument set of a launch given the first set's row count (rows n2 .. n1 of res_fc's output not zero);
  dW, db   a column block's gradient written to block 0's rows of dW (rows 256 .. of dW stay NaN); the row bound of the
           destination problem taken from the source count (res_fc's dW sees NaN rows);
  dX       the last k-block (64-row slab of W) dropped: at H*D = 288 the slab 256 .. 287 carries a ninth of every sum, far above
           the bound; the second Linear's product added on rows past its own count (NaN)."""
import pytest
import torch

from bounds import assert_within, dense_k, dgrad_terms, gemm_terms, wgrad_terms

pytestmark = pytest.mark.gpu
BF, NAN = torch.bfloat16, float("nan")
SHAPES = [(100, 288), (602, 1024), (1024, 7), (1024, 1024), (100, 7), (602, 288)]
ROWS = [(rows, live) for rows in (1, 33, 65) for live in sorted({0, 1, rows - 1, rows})]


@pytest.fixture
def nan_empty(monkeypatch):
    real = torch.empty

    def nan_empty(*a, **kw):
        t = real(*a, **kw)
        if t.is_cuda and t.is_floating_point():
            t.fill_(NAN)
        return t

    monkeypatch.setattr(torch, "empty", nan_empty)


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF)


def _padded(t, live, cuda):
    t = t.clone()
    t[live:] = NAN
    return t.to(cuda)


def _zeros_past(t, live):
    return not bool(t[live:].contiguous().view(torch.int16).any())


@pytest.mark.parametrize("rows,live", ROWS)
@pytest.mark.parametrize("fin,HD", SHAPES)
def test_gat_linear_pair_per_element(cuda, nan_empty, fin, HD, rows, live):
    """fc_src over ``rows`` source rows (``live`` of them live) and res_fc over the first ``rows2`` of them (``live2`` live), both
    with a bias, in shared launches; then all gradients of one backward."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(10000 * fin + 10 * HD + rows + live)
    rows2, live2 = max(1, (rows + 1) // 2), min(live, max(0, (rows + 1) // 2 - (1 if live < rows else 0)))
    x = _rand(gen, rows, fin)
    w1, b1 = _rand(gen, HD, fin, scale=fin ** -0.5), _rand(gen, HD)
    w2, b2 = _rand(gen, HD, fin, scale=fin ** -0.5), _rand(gen, HD)
    d1, d2 = _rand(gen, rows, HD), _rand(gen, rows2, HD)
    xd = _padded(x, live, cuda).requires_grad_(True)
    p = [t.to(cuda).requires_grad_(True) for t in (w1, b1, w2, b2)]
    n1 = torch.tensor([live], dtype=torch.int32, device=cuda)
    n2 = torch.tensor([live2], dtype=torch.int32, device=cuda)
    y1, y2 = bnn.gat_linear(xd, p[0], p[1], rows, n1.data_ptr(), p[2], p[3], rows2, n2.data_ptr())
    torch.autograd.backward([y1, y2], [_padded(d1, live, cuda), _padded(d2, live2, cuda)])
    torch.cuda.synchronize()
    X, W1, B1, W2, B2, D1, D2 = (t.to(cuda) for t in (x, w1, b1, w2, b2, d1, d2))
    case = "in %d HD %d rows %d/%d, %d/%d" % (fin, HD, live, rows, live2, rows2)
    assert y1.shape == (rows, HD) and y2.shape == (rows2, HD) and _zeros_past(y1, live) and _zeros_past(y2, live2), case + ": padding rows"
    r = {}
    r["y1"] = assert_within(y1[:live], *gemm_terms(X[:live], W1, bias=B1), *dense_k(fin + 1), case + " fc_src")
    r["y2"] = assert_within(y2[:live2], *gemm_terms(X[:live2], W2, bias=B2), *dense_k(fin + 1), case + " res_fc")
    for name, w, b, d, n in (("1", p[0], p[1], D1, live), ("2", p[2], p[3], D2, live2)):
        dw, mdw, db, mdb = wgrad_terms(d, X, n)
        r["dW" + name] = assert_within(w.grad, dw, mdw, *dense_k(n + 80), case + " dW" + name)
        r["db" + name] = assert_within(b.grad, db, mdb, *dense_k(n + 80), case + " db" + name)
    assert xd.grad.shape == (rows, fin) and _zeros_past(xd.grad, live), case + ": padding rows of dX"
    ref, mag = dgrad_terms(D1[:live], W1, D2[:live], W2, m2=live2) if live else (torch.zeros(0, fin), torch.zeros(0, fin))
    fused = bnn._dgrad_fits(HD, HD)
    # two launches and a bf16 add when both operands do not fit the LDS: one more stored rounding on the path
    r["dX"] = assert_within(xd.grad[:live], ref, mag, *dense_k(2 * HD, 0.0 if fused else 1.0), case + " dX")
    for k, v in r.items():
        print("RATIO %s %s %.3f" % (case, k, v))


@pytest.mark.parametrize("rows,live", ROWS)
@pytest.mark.parametrize("fin,HD", [(100, 288), (1024, 1024), (602, 7)])
def test_gat_linear_single_no_bias(cuda, nan_empty, fin, HD, rows, live):
    """The model's own configuration (bias=False, no res_fc on the input layer): one Linear, an odd trailing launch."""
    from bliss_gnn_amd import nn as bnn
    gen = torch.Generator().manual_seed(fin + HD + rows + live)
    x, w, d = _rand(gen, rows, fin), _rand(gen, HD, fin, scale=fin ** -0.5), _rand(gen, rows, HD)
    xd, wd = _padded(x, live, cuda).requires_grad_(True), w.to(cuda).requires_grad_(True)
    n1 = torch.tensor([live], dtype=torch.int32, device=cuda)
    y, none = bnn.gat_linear(xd, wd, None, rows, n1.data_ptr())
    assert none is None
    y.backward(_padded(d, live, cuda))
    X, W, D = x.to(cuda), w.to(cuda), d.to(cuda)
    case = "single in %d HD %d rows %d/%d" % (fin, HD, live, rows)
    assert _zeros_past(y, live) and _zeros_past(xd.grad, live)
    assert_within(y[:live], *gemm_terms(X[:live], W), *dense_k(fin), case + " y")
    dw, mdw, _, _ = wgrad_terms(D, X, live)
    assert_within(wd.grad, dw, mdw, *dense_k(live + 80), case + " dW")
    if live:
        assert_within(xd.grad[:live], *dgrad_terms(D[:live], W), *dense_k(HD), case + " dX")
    # an exact-size call (no device count) on the live rows alone gives the same bits: no row's result depends on the capacity
    if live:
        x2, w2 = X[:live].clone().requires_grad_(True), W.clone().requires_grad_(True)
        y2, _ = bnn.gat_linear(x2, w2, None, live)
        y2.backward(D[:live].contiguous())
        assert torch.equal(y2, y[:live]) and torch.equal(x2.grad, xd.grad[:live]) and torch.equal(w2.grad, wd.grad)
