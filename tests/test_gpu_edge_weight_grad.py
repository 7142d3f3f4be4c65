"""GPU suite (-m gpu): edge weights that require a gradient get one from the aggregation functions, the layers in front of them
and the fused hidden SAGE layer (bliss::sddmm).  Before this, ``w.grad`` stayed None without a word.

The functions (weighted_aggregate sum and mean, gcn_aggregate, max_aggregate, update_all(u_mul_e, sum | mean | max)) on
bounds.edge_shape_spec(), exact-size and capacity-padded, dim 64 and 41: ``w.grad`` is within ``sddmm_ref.k(dim)`` =
bounds.dense_k(dim + 2) of the fp64 autograd of a torch ``index_add_`` restatement (both operands of the dot product, the given
bf16 d out and h, are exact here, so only the kernel's own dim + 2 fp32 operations and its one rounding count; max is routed by the
project's own winner table, whose choice the forward suites check), equal bit for bit to the exact-size run on a padded block and
+0 past the live edges; ``out`` and ``h.grad`` have the bits of the same call with weights that require nothing.

The layers through their ``forward`` (activation None, so the upstream gradient g reaches the aggregation's surroundings exactly):
the dot product's operands are now stored bf16 results of dense products, each within 2^-9 of its own magnitude, so the bound is
dense_k(dim + 2, stored) on mag = coef * sum_c magG[dst, c] * magX[src, c] with the operands' MAGNITUDES (|g| |W| summed):
  SAGEConv mean, aggregate first: G = g W_neigh stored (1) + its out_feats fp32 terms; X = h exact.
  SAGEConv mean, fc_neigh first:  X = h W_neigh^T stored (1) + in_feats terms; G = g exact.
  SAGEConv pool: X = relu(fc_pool(h)), a product and a bias add (2); G = g W_neigh (1); in + out terms.
  SAGEGCNConv (aggregate first): as the first, coefficient 1 / (deg + 1).
  GraphConv "library": X = h * out_deg^-1/2, the norm rounded to bf16 (1) and the product (1); G = (g * in_deg^-1/2) W^T: the norm
  (1), the scaled g (1), the product (1): 5 + out_feats terms.
_SageAggDual: sddmm_ref.k_agg_dual(dim, out_feats) on the same magnitude, mask and 1 / (1 - p) from the layer's stored output.
One case on integers ({-1, 0, 1}, power-of-two degrees) equals fp64: every intermediate is exact."""
import pytest
import torch

import bounds
import sddmm_ref as ref

pytestmark = pytest.mark.gpu

KINDS = ("sum", "mean", "gcn", "max", "ua_sum", "ua_mean", "ua_max")
MODE = {"sum": ref.SUM, "mean": ref.MEAN, "gcn": ref.SELF, "max": ref.MAX}


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _call(kind, blk, h, w):
    from bliss_gnn_amd import function as fn
    from bliss_gnn_amd import nn as bnn
    if kind == "sum" or kind == "mean":
        return bnn.weighted_aggregate(blk, h, w, mean=(kind == "mean"))
    if kind == "gcn":
        return bnn.gcn_aggregate(blk, h, w)
    if kind == "max":
        return bnn.max_aggregate(blk, h, w)
    red = {"ua_sum": fn.sum, "ua_mean": fn.mean, "ua_max": fn.max}[kind]
    with blk.local_scope():
        blk.srcdata["h"], blk.edata["w"] = h, w
        blk.update_all(fn.u_mul_e("h", "w", "m"), red("m", "o"))
        return blk.dstdata["o"]


def _restated_gw(spec, mode, h, w, g, arg):
    """fp64 autograd of the index_add_ restatement on the live part: d (out . g) / d w."""
    dev = h.device
    src, dst = spec.src.to(dev), spec.dst.to(dev)
    h64, g64 = h[: spec.K].double(), g[: spec.S].double()
    w64 = w[: spec.B].detach().double().requires_grad_()
    m = w64[:, None] * h64[src]
    if mode == ref.MAX:                                        # routed by the project's own winner table
        m = m * (arg[: spec.S].long()[dst] == torch.arange(spec.B, device=dev)[:, None])
    out = torch.zeros(spec.S, h.shape[1], dtype=torch.float64, device=dev).index_add_(0, dst, m)
    deg = spec.in_degrees().to(dev).double()
    if mode == ref.MEAN:
        out = out / deg.clamp(min=1)[:, None]
    elif mode == ref.SELF:
        out = (out + h64[: spec.S]) / (deg + 1)[:, None]
    return torch.autograd.grad((out * g64).sum(), w64)[0]


def _inputs(spec, blk, dim, seed):
    gen = torch.Generator().manual_seed(seed)
    dev = blk.device
    h = torch.randn(blk.num_src_nodes(), dim, generator=gen).bfloat16().to(dev)
    w = (torch.rand(blk.num_edges(), generator=gen) + 0.25).bfloat16().to(dev)
    g = torch.randn(blk.num_dst_nodes(), dim, generator=gen).bfloat16().to(dev)
    return h, w, g


@pytest.fixture(scope="module")
def edge(cuda):
    spec = bounds.edge_shape_spec()
    return spec, bounds.to_block(spec, cuda), bounds.padded_block(spec, cuda)


def _function_case(spec, blk, kind, dim, w_dtype, padded, seed):
    from bliss_gnn_amd.nn import max_aggregate
    mode = MODE[kind.replace("ua_", "")]
    h0, w0, g = _inputs(spec, blk, dim, seed)
    h, w = h0.clone().requires_grad_(), w0.to(w_dtype).clone().requires_grad_()
    out = _call(kind, blk, h, w)
    out.backward(g)
    assert w.grad is not None, kind + ": the edge weights got no gradient"                 # fails before bliss::sddmm
    assert w.grad.dtype == w_dtype and w.grad.shape == w.shape
    h2 = h0.clone().requires_grad_()
    out2 = _call(kind, blk, h2, w0)
    out2.backward(g)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(h.grad), _bits(h2.grad)), kind
    arg = max_aggregate(blk, h0, w0, return_arg=True)[1] if mode == ref.MAX else None
    want = _restated_gw(spec, mode, h0, w0, g, arg)
    _, mag = ref.terms(spec, g[: spec.S], h0[: spec.K], mode, None if arg is None else arg[: spec.S])
    r = bounds.assert_within(w.grad[: spec.B], want, mag, *ref.k(dim), (kind, dim, padded))
    if padded:
        assert not bool(_bits(w.grad[spec.B:]).any()), kind
    return r, w.grad.detach()


@pytest.mark.parametrize("kind", KINDS)
def test_functions_give_the_edge_weights_their_gradient(edge, kind):
    spec, exact, pad = edge
    for dim in (64, 41):
        r0, gw0 = _function_case(spec, exact, kind, dim, torch.bfloat16, False, 5 * dim)
        # the padded block's operands differ past the live rows only: same generator, longer tensors -> other values; so the
        # padded run is compared with ITS restatement, and with the exact-size run of the same live operands below
        r1, gw1 = _function_case(spec, pad, kind, dim, torch.bfloat16, True, 5 * dim + 1)
        print(kind, dim, r0, r1)


def test_padded_run_has_the_bits_of_the_exact_size_run(edge):
    spec, exact, pad = edge
    for kind in ("mean", "gcn", "max"):
        hp, wp, gp = _inputs(spec, pad, 64, 3)
        got = []
        for blk, (h0, w0, g) in ((pad, (hp, wp, gp)), (exact, (hp[: spec.K].clone(), wp[: spec.B].clone(), gp[: spec.S].clone()))):
            h, w = h0.requires_grad_(), w0.requires_grad_()
            _call(kind, blk, h, w).backward(g)
            got.append(w.grad)
        assert torch.equal(_bits(got[0][: spec.B]), _bits(got[1])) and not bool(_bits(got[0][spec.B:]).any()), kind


def test_fp32_leaf_gets_its_gradient_through_the_cast(edge):
    spec, exact, _ = edge
    r, gw = _function_case(spec, exact, "mean", 64, torch.float32, False, 9)
    assert torch.equal(gw, gw.bfloat16().float())              # the bf16 kernel result, widened


def test_integers_equal_fp64(cuda):
    spec = bounds.from_degrees([1, 2, 4, 8, 16, 32, 64, 128], 64, seed=2)
    blk = bounds.to_block(spec, cuda)
    gen = torch.Generator().manual_seed(4)
    ri = lambda *s: torch.randint(-1, 2, s, generator=gen).bfloat16().to(cuda)
    h0, g = ri(spec.K, 64), ri(spec.S, 64)
    w0 = torch.ones(spec.B, dtype=torch.bfloat16, device=cuda)
    for kind in ("sum", "mean"):
        w = w0.clone().requires_grad_()
        _call(kind, blk, h0, w).backward(g)
        want = _restated_gw(spec, MODE[kind], h0, w0, g, None)
        assert torch.equal(w.grad.double(), want), kind


# ------------------------------------------------------------------------------------------------ the layers
def _layer_ref(kind, spec, layer, h, g, arg, dev):
    """(gw fp64, mag, (k_ulp, k_mag)) of a layer's edge-weight gradient: the formulas of the module docstring."""
    src, dst = spec.src.to(dev), spec.dst.to(dev)
    deg = spec.in_degrees().to(dev).double()
    h64, g64 = h.double(), g.double()
    P = lambda name: getattr(layer, name).weight.detach().double()
    one = torch.ones(spec.B, dtype=torch.float64, device=dev)
    keep, coef = None, one
    if kind in ("mean_agg_first", "gcn"):
        W = P("fc_neigh")
        G, mG, X, mX = g64 @ W, g64.abs() @ W.abs(), h64, h64.abs()
        coef = 1.0 / (deg.clamp(min=1) if kind == "mean_agg_first" else deg + 1)[dst]
        stored = 1.0 + W.shape[0] * 2.0 ** -16
    elif kind == "mean_lin_first":
        W = P("fc_neigh")
        G, mG, X, mX = g64, g64.abs(), h64 @ W.t(), h64.abs() @ W.abs().t()
        coef = 1.0 / deg.clamp(min=1)[dst]
        stored = 1.0 + W.shape[1] * 2.0 ** -16
    elif kind == "pool":
        W, Wp, bp = P("fc_neigh"), P("fc_pool"), layer.fc_pool.bias.detach().double()
        G, mG = g64 @ W, g64.abs() @ W.abs()
        X, mX = torch.relu(h64 @ Wp.t() + bp), h64.abs() @ Wp.abs().t() + bp.abs()
        keep = arg.long()[dst] == torch.arange(spec.B, device=dev)[:, None]
        stored = 3.0 + (W.shape[0] + Wp.shape[1]) * 2.0 ** -16
    else:                                                      # GraphConv "library", aggregate first
        W = layer.weight.detach().double()                     # [in, out]
        ns = torch.bincount(src, minlength=spec.K).double().clamp(min=1).pow(-0.5)
        nd = deg.clamp(min=1).pow(-0.5)
        G, mG = (g64 * nd[:, None]) @ W.t(), (g64.abs() * nd[:, None]) @ W.abs().t()
        X, mX = h64 * ns[:, None], h64.abs() * ns[:, None]
        stored = 5.0 + W.shape[1] * 2.0 ** -16
    t, m = G[dst] * X[src], mG[dst] * mX[src]
    if keep is not None:
        t, m = t * keep, m * keep
    return t.sum(1) * coef, m.sum(1) * coef, bounds.dense_k(G.shape[1] + 2, stored=stored)


@pytest.mark.parametrize("kind", ("mean_agg_first", "mean_lin_first", "pool", "gcn", "graphconv"))
def test_layers_give_the_edge_weights_their_gradient(edge, kind):
    from bliss_gnn_amd import nn as bnn
    spec, blk, _ = edge
    dev = blk.device
    torch.manual_seed(11)
    fin, fout = (64, 32) if kind == "mean_lin_first" else (32, 64)
    if kind == "gcn":
        layer = bnn.SAGEGCNConv(fin, fout)
    elif kind == "graphconv":
        layer = bnn.GraphConv(fin, fout, allow_zero_in_degree=True, transforms="library")
    else:
        layer = bnn.SAGEConv(fin, fout, "pool" if kind == "pool" else "mean")
    layer = layer.to(dev).bfloat16()
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(spec.K, fin, generator=gen).bfloat16().to(dev)
    w0 = (torch.rand(spec.B, generator=gen) + 0.25).bfloat16().to(dev)
    g = torch.randn(spec.S, fout, generator=gen).bfloat16().to(dev)
    w = w0.clone().requires_grad_()
    out = layer(blk, h, edge_weight=w)
    out.backward(g)
    assert w.grad is not None and w.grad.dtype == torch.bfloat16 and w.grad.shape == (spec.B,)
    out2 = layer(blk, h, edge_weight=w0)
    assert torch.equal(_bits(out), _bits(out2))
    arg = None
    if kind == "pool":
        with torch.no_grad():
            arg = bnn.max_aggregate(blk, torch.relu(layer.fc_pool(h)), w0, return_arg=True)[1]
    want, mag, k = _layer_ref(kind, spec, layer, h, g, arg, dev)
    print(kind, bounds.assert_within(w.grad, want, mag, *k, kind))


@pytest.mark.parametrize("library", (False, True))
@pytest.mark.parametrize("feats,p", [(64, 0.0), (64, 0.1), (256, 0.0), (256, 0.1)])
def test_sage_agg_dual_gives_the_edge_weights_their_gradient(edge, monkeypatch, feats, p, library):
    from bliss_gnn_amd import nn as bnn
    if library:
        monkeypatch.setenv("BLISS_SAGE_MFMA_BWD", "0")
    spec, exact, pad = edge
    for blk, padded in ((exact, False), (pad, True)):
        dev = blk.device
        gen = torch.Generator().manual_seed(feats + padded)
        sc = (2.0 / (2 * feats)) ** 0.5
        wn, ws = ((torch.randn(feats, feats, generator=gen) * sc).bfloat16().to(dev).requires_grad_() for _ in range(2))
        b = (torch.randn(feats, generator=gen) * 0.1).bfloat16().to(dev).requires_grad_()
        h0, w0, g = _inputs(spec, blk, feats, 21 + padded)
        ctr = torch.zeros(2 + 64, dtype=torch.int64, device=dev)
        rows_dev = blk._counts_dev.data_ptr() if padded else 0

        def run(wt):
            hh = h0.clone().requires_grad_()
            ctr.zero_()
            out, _ = bnn.sage_agg_dual(blk, hh, wt, wn, ws, b, True, p, ctr, 5, rows_dev)
            wn.grad = ws.grad = b.grad = None
            out.backward(g)
            return out.detach(), hh.grad

        w = w0.clone().requires_grad_()
        out, gh = run(w)
        assert w.grad is not None and w.grad.dtype == torch.bfloat16
        out2, gh2 = run(w0)
        assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(gh), _bits(gh2))
        S, K, B = spec.S, spec.K, spec.B
        src, dst = spec.src.to(dev), spec.dst.to(dev)
        d = g[:S].double() * (out[:S] > 0) / (1.0 - p)         # the layer's own stored output is the mask
        W = wn.detach().double()
        G, mG = d @ W, d.abs() @ W.abs()
        coef = 1.0 / spec.in_degrees().to(dev).double().clamp(min=1)[dst]
        X = h0[:K].double()
        want, mag = (G[dst] * X[src]).sum(1) * coef, (mG[dst] * X[src].abs()).sum(1) * coef
        r = bounds.assert_within(w.grad[:B], want, mag, *ref.k_agg_dual(feats, feats), (feats, p, library, padded))
        assert not bool(_bits(w.grad[B:]).any())
        print(feats, p, library, padded, r)


def test_captured_forward_and_backward_replays(edge):
    """weighted_aggregate(mean) forward + backward on the padded block under torch.cuda.graph, replayed twice with new values
    copied into the static tensors: each replay equals the eager exact-size run on [0, B) and is +0 beyond."""
    from bliss_gnn_amd.nn import weighted_aggregate
    spec, exact, pad = edge
    hs, ws, gs = _inputs(spec, pad, 64, 40)
    hs.requires_grad_(), ws.requires_grad_()
    pad.transposed()

    def step():
        out = weighted_aggregate(pad, hs, ws, mean=True)
        return torch.autograd.grad(out, [hs, ws], gs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        gh_s, gw_s = step()
    for seed in (41, 42):
        h1, w1, g1 = _inputs(spec, pad, 64, seed)
        with torch.no_grad():
            hs.copy_(h1), ws.copy_(w1), gs.copy_(g1)
        gr.replay()
        he, we = h1[: spec.K].clone().requires_grad_(), w1[: spec.B].clone().requires_grad_()
        weighted_aggregate(exact, he, we, mean=True).backward(g1[: spec.S])
        assert torch.equal(_bits(gw_s[: spec.B]), _bits(we.grad)) and not bool(_bits(gw_s[spec.B:]).any()), seed
        assert torch.equal(_bits(gh_s[: spec.K]), _bits(he.grad)), seed


def test_opcheck_schema_and_fake(edge):
    from bliss_gnn_amd import ops  # noqa: F401  (registers the ops)
    spec, blk, _ = edge
    a, b = ref.operands(spec, 41, 1, blk.device)
    torch.library.opcheck(torch.ops.bliss.sddmm.default, (blk.src, blk.dst, blk.indptr, a, b, None, None, ref.MEAN, False),
                          test_utils=("test_schema", "test_faketensor"))


def test_second_derivative_is_refused(edge):
    spec, blk, _ = edge
    from bliss_gnn_amd.nn import weighted_aggregate
    h, w, g = _inputs(spec, blk, 8, 2)
    w.requires_grad_()
    out = weighted_aggregate(blk, h, w, mean=False)
    gw, = torch.autograd.grad(out, [w], g.requires_grad_(), create_graph=True)
    with pytest.raises(NotImplementedError, match="bliss::sddmm"):
        gw.float().sum().backward()
