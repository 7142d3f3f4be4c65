"""GPU suite: GATv2 and SpMM message passing, forward and backward, element by element against float64 at the shapes where the
kernels go wrong -- zero / one / chunk-edge / segment-edge in-degrees, a 47-segment hub, thousands of shared rows, both
branches of k_gat_segments, every kernel specialisation, capacity padding -- with the bound of tests/bounds.py:

    |got - ref| <= k_ulp * ulp_bf16(ref) + k_mag * 2^-8 * mag,     mag = the reference on absolute values, per element.

The leaves are feat = fc_src(h) [K, H*D] bf16 and attn: the layer's GEMMs stay out of the kernels' error.  Every test prints
``RATIO <case> <tensor> <largest |got - ref| / bound>`` (pytest -s) for the margin table of DESIGN.md 3.

Constants (bounds.GAT_K), derived from where the kernels round (csrc/gat_fused.hip, csrc/gat.hip), for inputs whose logits
have sum_d |attn| |lrelu(x)| <= 1 (bounds.gat_inputs makes it so and each test asserts it):
  e       (1, 2):  three bf16 roundings per term (el + er, leaky_relu, * attn: 1.5 * 2^-8 of the term), an fp32 sum, one
                   rounding at the store (k_ulp).
  rst     (1, 9):  a carries the logits' error twice (its own and its row's sum: 2 * 2 * 2^-8) and four roundings of its own
                   (e - max, exp, the bf16 sum, the division: 4 * 2^-8), the dropout multiply 0.5; fp32 products and sums.
  d feat  (1, 18) on rows >= S: d e = a (da - t) takes a's 8 * 2^-8 on (da - t) and again through t, da's two roundings
                   (the dot product, the dropout scale) and d e's own: 8 + 9 + 0.5 = 17.5.  The aggregation's term a_drop g
                   carries 8.5.  (1, 19) on rows < S: d feat = rbf(rbf(d el) + rbf(d er)), two more roundings of 0.5 each.
  d attn  (1, 18): the same d e, fp32 sums, the final bf16 conversion.  (d er is not returned: it is inside d feat's
                   destination rows.)  bounds.gat_k gives the constants for larger logits (the layer-level tests).
SpMM (bounds.SPMM_K): only the store rounds (k_ulp 1; fp32 output: 0) and the fp32 sum of at most 16 384 terms moves it by
at most n 2^-24 <= 0.25 * 2^-8 of its magnitude (k_mag 0.25; mean: two more fp32 roundings of 1/deg)."""
import itertools

import pytest
import torch

from bounds import (GAT_K, GCN_K, SPMM_K, SPMM_MAX_ROW, assert_within, edge_shape_spec, gat_autograd, gat_inputs, gat_terms,
                    loud_segments, many_hubs_spec, padded_block, row_count_spec, spmm_band_spec, spmm_terms, to_block)

pytestmark = pytest.mark.gpu
SLOPE = 0.2
_SPECS = {}


def _spec(name):
    if name not in _SPECS:
        _SPECS[name] = {"edge": edge_shape_spec, "hubs": many_hubs_spec, "r16384": lambda: row_count_spec(16384),
                        "r16385": lambda: row_count_spec(16385), "band100k": lambda: spmm_band_spec(100000, 21),
                        "band210k": lambda: spmm_band_spec(210000, 22)}[name]()
    return _SPECS[name]


def _report(case, ratios):
    for k, v in ratios.items():
        print("RATIO %s %s %.3f" % (case, k, v))


def _state(dev):
    return dict(ctr=torch.zeros(2, dtype=torch.int64, device=dev), ticket=torch.zeros(1, dtype=torch.int32, device=dev),
                seed=0x1234567, err=torch.zeros(1, dtype=torch.int32, device=dev), row_ws=None)


def _assert_clean(st):
    """The fused kernels' error word is zero and every per-row meeting word was returned to zero."""
    assert int(st["err"].item()) == 0, "error word 0x%x" % int(st["err"].item())
    assert st["row_ws"] is None or not bool((st["row_ws"] != 0).any()), "row_ws left non-zero"


def _specialisation(H, D):
    from bliss_gnn_amd.nn import _gat_fused_on
    if not _gat_fused_on(H, D):
        return "separate"
    if D % 4 == 0:
        return "HG%d" % H if D == 256 and H in (1, 2, 4) else "vec4"
    return "scalar"


def run_fused(blk, feat, attn, g, H, D, p=0.0, st=None):
    from bliss_gnn_amd.nn import _GatFusedMP
    st = st or _state(feat.device)
    f, a = feat.clone().requires_grad_(True), attn.clone().requires_grad_(True)
    rst, e = _GatFusedMP.apply(f, a, blk, H, D, SLOPE, p, st)
    _assert_clean(st)
    saved = rst.grad_fn.saved_tensors
    rst.backward(g)
    _assert_clean(st)
    return dict(e=e.detach(), rst=rst.detach(), d_feat=f.grad, d_attn=a.grad.reshape(-1), a=saved[2], ad=saved[3])


def run_separate(blk, feat, attn, g, H, D):
    from bliss_gnn_amd.nn import _EdgeSoftmax, _GatAggregate, _GatLogits
    f, a = feat.clone().requires_grad_(True), attn.clone().requires_grad_(True)
    e = _GatLogits.apply(f, a, blk, H, D, SLOPE)
    rst = _GatAggregate.apply(_EdgeSoftmax.apply(e, blk, H), f, blk, H, D)
    rst.backward(g)
    return dict(e=e.detach(), rst=rst.detach(), d_feat=f.grad, d_attn=a.grad.reshape(-1))


def check_gat(spec, got, feat, attn, g, H, D, case, mask=None, p=0.0, S=None, K=None, B=None):
    """got (rows / edges beyond the spec's true S, K, B ignored) vs fp64 autograd, per element, with GAT_K."""
    dev = feat.device
    S, K, B = spec.S, spec.K, spec.B
    src, dst = spec.src.to(dev), spec.dst.to(dev)
    feat, g = feat[:K], g[:S]
    ref_e, ref_rst, ref_df, ref_da = gat_autograd(src, dst, S, feat, attn, H, D, g, mask=mask, p=p)
    T = gat_terms(src, dst, S, feat, attn, H, D, g, mask=mask, p=p)
    assert float(T["mag_e"].max()) <= 1.0, "the constants assume logits of magnitude <= 1"
    r = {}
    r["e"] = assert_within(got["e"][:B].reshape(B, H), ref_e, T["mag_e"], *GAT_K["e"], case + " e")
    r["rst"] = assert_within(got["rst"][:S].reshape(S, H * D), ref_rst, T["mag_rst"], *GAT_K["rst"], case + " rst")
    df = got["d_feat"][:K]
    r["d_feat_dst"] = assert_within(df[:S], ref_df[:S], T["mag_dfeat"][:S], *GAT_K["d_feat_dst"], case + " d feat (rows < S)")
    r["d_feat_src"] = assert_within(df[S:], ref_df[S:], T["mag_dfeat"][S:], *GAT_K["d_feat_src"], case + " d feat (rows >= S)")
    r["d_attn"] = assert_within(got["d_attn"], ref_da, T["mag_dattn"], *GAT_K["d_attn"], case + " d attn")
    _report(case, r)
    return r


EDGE_HD = [(4, 256), (2, 256), (1, 256), (8, 128), (4, 16), (1, 41), (4, 63), (2, 150), (8, 200)]


@pytest.mark.parametrize("H,D", EDGE_HD)
def test_gat_edge_shape_block_both_paths(cuda, H, D):
    """The edge-shape block (in-degrees 0, 1, 2, 15..17, 63..65, 255..257, 512, 513, 1500, a 12 000-edge hub) through every
    specialisation of the fused kernels (HG4 / HG2 / HG1 at D = 256, vec4, scalar up to its H*D = 256 limit) and through the
    separate kernels; (2, 150) and (8, 200) are beyond the fused limits and must take the separate path."""
    spec = _spec("edge")
    assert spec.B * H * D <= 6e7
    blk = to_block(spec, cuda)
    feat, attn, g = gat_inputs(spec, H, D, 100 + H * D, cuda)
    kind = _specialisation(H, D)
    if (H, D) in ((2, 150), (8, 200)):
        assert kind == "separate"
    else:
        assert kind != "separate"
        check_gat(spec, run_fused(blk, feat, attn, g, H, D), feat, attn, g, H, D, "fused-%s-%dx%d-edge" % (kind, H, D))
    check_gat(spec, run_separate(blk, feat, attn, g, H, D), feat, attn, g, H, D, "separate-%dx%d-edge" % (H, D))


@pytest.mark.parametrize("name", ["hubs", "r16384", "r16385"])
@pytest.mark.parametrize("H,D", [(2, 16), (1, 41)])
def test_gat_shared_rows_and_segment_branches(cuda, name, H, D):
    """Thousands of shared rows (far more virtual workgroups than the chip holds at once: the segment hand-off with partners not
    yet resident) and exactly 16 384 / 16 385 destinations (the one-sweep and two-pass branches of k_gat_segments), vec4 and
    scalar, both paths."""
    spec = _spec(name)
    assert spec.B * H * D <= 6e7
    if name == "hubs":
        assert int((spec.in_degrees() > 256).sum()) >= 1500
        assert int(((spec.in_degrees() + 255) // 256).sum()) > 4000
    blk = to_block(spec, cuda)
    feat, attn, g = gat_inputs(spec, H, D, 7, cuda)
    kind = _specialisation(H, D)
    check_gat(spec, run_fused(blk, feat, attn, g, H, D), feat, attn, g, H, D, "fused-%s-%dx%d-%s" % (kind, H, D, name))
    check_gat(spec, run_separate(blk, feat, attn, g, H, D), feat, attn, g, H, D, "separate-%dx%d-%s" % (H, D, name))


LOUD_CASES = [("edge", "first"), ("edge", "middle"), ("edge", "last"), ("hubs", "cycle"), ("r16384", "cycle"), ("r16385", "cycle")]


@pytest.mark.parametrize("block,which", LOUD_CASES)
@pytest.mark.parametrize("H,D", [(2, 16), (1, 41)])
def test_gat_segment_combine_with_loud_segments(cuda, block, which, H, D):
    """The combine of a shared destination row, on inputs where a lost segment is visible.  With random signs the partial sums
    of one 256-edge segment nearly cancel, so the shared-row cases above could not see a segment dropped from t, from d er or
    from the aggregation.  Here every shared row takes one segment's edges from a dedicated source with 64x the (positive)
    features of the others -- the first, middle or last segment of the 47-segment hub, and segment (row mod G) of every row on
    the many-hubs and 16 384 / 16 385 blocks.  tests/test_bounds.py::test_loud_segment_inputs_of_the_gpu_suite_expose_a_lost_segment
    shows on these very inputs that losing the loud segment of the longest shared row fails GAT_K."""
    spec, loud, _ = loud_segments(_spec(block), which)
    assert spec.B * H * D <= 6e7
    blk = to_block(spec, cuda)
    feat, attn, g = gat_inputs(spec, H, D, 77, cuda, positive=True, loud=loud)
    check_gat(spec, run_fused(blk, feat, attn, g, H, D), feat, attn, g, H, D, "fused-%s-%dx%d-%s-loud-%s" % (_specialisation(H, D), H, D, block, which))


def test_one_state_across_launches_of_different_blocks(cuda):
    """The layer keeps one device state (error word, per-row meeting words) for all its launches: a word left non-zero by one
    launch would corrupt the next launch of another block.  One state through fused forward + backward of five blocks in turn,
    twice over: every result has the bits of the same launch on a fresh state, and the words are zero after each."""
    st = _state(cuda)
    H, D = 2, 16
    names = ["edge", "hubs", "r16385", "r16384", "edge"]
    fresh = {}
    for rnd in range(2):
        for n in names:
            spec = _spec(n)
            blk = to_block(spec, cuda)
            feat, attn, g = gat_inputs(spec, H, D, 3, cuda)
            got = run_fused(blk, feat, attn, g, H, D, st=st)
            if n not in fresh:
                fresh[n] = run_fused(blk, feat, attn, g, H, D)
            for k in ("e", "rst", "d_feat", "d_attn"):
                assert torch.equal(got[k].view(torch.int16), fresh[n][k].view(torch.int16)), (rnd, n, k)


def test_gat_attention_dropout_backward(cuda):
    """p = 0.3 on the edge-shape block (fused: the shared rows included).  The mask is read back from the kernel's outputs
    (a_drop != 0), then forward and backward are checked per element against fp64 autograd under that mask."""
    spec = _spec("edge")
    H, D, p = 4, 16, 0.3
    blk = to_block(spec, cuda)
    feat, attn, g = gat_inputs(spec, H, D, 5, cuda)
    got = run_fused(blk, feat, attn, g, H, D, p=p)
    a, ad = got["a"].float(), got["ad"].float()
    assert bool((a > 0).all())
    keep = ad != 0
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.02
    assert torch.equal(ad[keep], (a[keep] * (1 / (1 - p))).bfloat16().float())
    check_gat(spec, got, feat, attn, g, H, D, "fused-dropout-4x16-edge", mask=keep, p=p)


def test_gat_forward_f32_vs_fp64(cuda):
    """gat_forward_f32 (no intermediate rounding, float results) on the edge-shape block: |got - ref| <= 1e-4 mag per element."""
    from bliss_gnn_amd.nn import gat_forward_f32
    spec = _spec("edge")
    blk = to_block(spec, cuda)
    r = {}
    for H, D in ((4, 16), (1, 41), (4, 256)):
        feat, attn, g = gat_inputs(spec, H, D, 3, cuda)
        e, a, out = gat_forward_f32(blk, feat, attn, H, D, SLOPE)
        T = gat_terms(spec.src.to(cuda), spec.dst.to(cuda), spec.S, feat, attn, H, D)
        r["e-%dx%d" % (H, D)] = assert_within(e, T["e"], T["mag_e"], 0, 1e-4 * 256, "f32 e")
        r["a-%dx%d" % (H, D)] = assert_within(a, T["a"], T["a"], 0, 1e-4 * 256, "f32 a")
        r["rst-%dx%d" % (H, D)] = assert_within(out, T["rst"], T["mag_rst"], 0, 1e-4 * 256, "f32 rst")
    _report("f32-edge", r)


def test_fused_and_spmm_are_deterministic(cuda):
    """Fused forward + backward and SpMM forward + backward twice on the same inputs: identical bits (both are order-fixed by
    design: segment partials in segment order, d attn shares in workgroup order, SpMM chunks through the fix-up in chunk
    order).  The separate path's d attn adds fp32 atomics per workgroup and is exempt."""
    from bliss_gnn_amd.nn import weighted_aggregate
    spec = _spec("edge")
    blk = to_block(spec, cuda)
    for H, D in ((4, 256), (4, 16), (1, 41)):
        feat, attn, g = gat_inputs(spec, H, D, 8, cuda)
        r1, r2 = run_fused(blk, feat, attn, g, H, D), run_fused(blk, feat, attn, g, H, D)
        for k in ("e", "rst", "d_feat", "d_attn"):
            assert torch.equal(r1[k].view(torch.int16), r2[k].view(torch.int16)), (H, D, k)
    h = torch.randn(spec.K, 64, generator=torch.Generator().manual_seed(1)).bfloat16().to(cuda)
    w = torch.rand(spec.B, generator=torch.Generator().manual_seed(2)).bfloat16().to(cuda)
    gout = torch.randn(spec.S, 64, generator=torch.Generator().manual_seed(3)).bfloat16().to(cuda)
    outs = []
    for _ in range(2):
        hd = h.clone().requires_grad_(True)
        o = weighted_aggregate(blk, hd, w, mean=True)
        o.backward(gout)
        outs.append((o.detach().view(torch.int16), hd.grad.view(torch.int16)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_capacity_padded_blocks(cuda):
    """The capacity-padded copy of the edge-shape block (padding edges naming the hub row and the hub source, indptr repeating
    the edge count past the true S, garbage feature rows past the true K): fused GAT values on the true rows equal the unpadded
    block's, padded rows of every output and gradient are exactly zero, SpMM passes its bound, and Block.transposed() on the
    true edges is the stable argsort of src."""
    from bliss_gnn_amd.nn import weighted_aggregate
    spec = _spec("edge")
    S, K, B = spec.S, spec.K, spec.B
    blk, pad = to_block(spec, cuda), padded_block(spec, cuda)
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    assert (S <= 16384) == (Sc <= 16384)
    gen = torch.Generator().manual_seed(4)
    t_indptr, t_edge = pad.transposed()
    src = spec.src
    assert torch.equal(t_edge[:B].cpu().long(), torch.sort(src, stable=True).indices)
    assert torch.equal(t_indptr.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(src, minlength=Kc), 0)]))
    for H, D in ((4, 16), (1, 41), (4, 256)):
        feat, attn, g = gat_inputs(spec, H, D, 6, cuda)
        feat_p = torch.cat([feat, (torch.randn(Kc - K, H * D, generator=gen) * 3).bfloat16().to(cuda)])
        g_p = torch.cat([g, (torch.randn(Sc - S, H * D, generator=gen) * 3).bfloat16().to(cuda)])
        u, q = run_fused(blk, feat, attn, g, H, D), run_fused(pad, feat_p, attn, g_p, H, D)
        assert torch.equal(q["rst"][:S].float(), u["rst"].float()) and torch.equal(q["e"][:B].float(), u["e"].float())
        assert torch.equal(q["d_feat"][:K].float(), u["d_feat"].float()) and torch.equal(q["d_attn"].float(), u["d_attn"].float())
        assert not bool(q["rst"][S:].any()) and not bool(q["d_feat"][K:].any()), "padded rows must be zero"
    dim = 64
    h = torch.randn(Kc, dim, generator=gen).bfloat16().to(cuda)
    w = (torch.rand(Bc, generator=gen) + 0.05).bfloat16().to(cuda)
    gout = torch.randn(Sc, dim, generator=gen).bfloat16().to(cuda)
    r = {}
    for mean, wt in itertools.product((True, False), (True, False)):
        hd = h.clone().requires_grad_(True)
        out = weighted_aggregate(pad, hd, w if wt else None, mean=mean)
        out.backward(gout)
        ref, mag = spmm_terms(src.to(cuda), spec.dst.to(cuda), S, h[:K], w[:B] if wt else None, mean)
        rb, mb = spmm_terms(src.to(cuda), spec.dst.to(cuda), S, gout[:S], w[:B] if wt else None, mean, by_src=True, n_out=K)
        r["out-%d%d" % (mean, wt)] = assert_within(out[:S], ref, mag, *SPMM_K["bf16"], "padded spmm out")
        r["dh-%d%d" % (mean, wt)] = assert_within(hd.grad[:K], rb, mb, *SPMM_K["bf16"], "padded spmm d h")
        assert not bool(out[S:].any()) and not bool(hd.grad[K:].any()), "padded rows must be zero"
    _report("padded-spmm", r)


_MODES = list(itertools.product((True, False), (True, False), (False, True)))       # mean, weighted, fp32 output


@pytest.mark.parametrize("band,name,ec", [(0, "edge", 16), (1, "band100k", 32), (2, "band210k", 64)])
def test_spmm_forward_backward_per_element(cuda, band, name, ec):
    """weighted_aggregate forward and backward in each chunk-length band (< 50 000 edges: 16, 50 000..199 999: 32, >= 200 000:
    64), dim 1, 3, 4, 41, 64, 256, 260, 602, every (mean / sum, weighted / unweighted, bf16 / fp32 output) combination twice
    per band, and for dim % 4 == 0 also h as a column slice 4 bytes off alignment with a row stride != dim (the scalar path)."""
    from bliss_gnn_amd import _lib
    from bliss_gnn_amd.nn import weighted_aggregate
    spec = _spec(name)
    assert int(_lib.lib.bliss_spmm_chunk_edges(spec.B)) == ec
    assert int(spec.in_degrees().max()) <= SPMM_MAX_ROW and int(spec.out_degrees().max()) <= SPMM_MAX_ROW
    assert int(spec.out_degrees().max()) >= 3000
    blk = to_block(spec, cuda)
    src, dst = spec.src.to(cuda), spec.dst.to(cuda)
    gen = torch.Generator().manual_seed(30 + band)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    r = {}
    for i, dim in enumerate((1, 3, 4, 41, 64, 256, 260, 602)):
        hfull = torch.randn(spec.K, dim + 6, generator=gen).bfloat16().to(cuda)
        gout = torch.randn(spec.S, dim, generator=gen).bfloat16().to(cuda)
        layouts = [("contig", hfull[:, :dim].contiguous())]
        if dim % 4 == 0:
            sl = hfull[:, 2:2 + dim]
            assert sl.data_ptr() % 8 == 4 and sl.stride(0) != dim
            layouts.append(("slice", sl))
        for m in (_MODES[(i + band) % 8], _MODES[(i + band + 4) % 8]):
            mean, wt, f32 = m
            for lay, h in layouts:
                hd = h.detach().requires_grad_(True)
                out = weighted_aggregate(blk, hd, w if wt else None, mean=mean, out_fp32=f32)
                out.backward(gout.to(out.dtype))
                ref, mag = spmm_terms(src, dst, spec.S, hd.detach(), w if wt else None, mean)
                rb, mb = spmm_terms(src, dst, spec.S, gout, w if wt else None, mean, by_src=True, n_out=spec.K)
                case = "d%d-%s-%s-%s-%s" % (dim, "mean" if mean else "sum", "w" if wt else "1", "f32" if f32 else "bf16", lay)
                r[case + "-out"] = assert_within(out, ref, mag, *SPMM_K["fp32" if f32 else "bf16"], "spmm out " + case)
                r[case + "-dh"] = assert_within(hd.grad, rb, mb, *SPMM_K["bf16"], "spmm d h " + case)
    _report("spmm-%s-ec%d" % (name, ec), {"max": max(r.values())})


@pytest.mark.parametrize("fin,fout", [(48, 16), (16, 48)])
def test_graphconv_forward_and_feature_gradient(cuda, fin, fout):
    """GraphConv(norm='both') on the edge-shape block with edge weights: forward and d feat per element against fp64 of
    [DGL-recalled] GraphConv with the layer's bf16 weights.  Constants GCN_K = (1, 4): bf16 roundings of the two degree norms
    (1.5 * 0.5 each: the degree's conversion and the power), feat * norm, the GEMM, the SpMM (0.5 + 0.25), * in-degree norm,
    the bias add at the store (k_ulp); the backward rounds at the mirrored points."""
    from bliss_gnn_amd.nn import GraphConv
    spec = _spec("edge")
    blk = to_block(spec, cuda)
    K, S = spec.K, spec.S
    torch.manual_seed(2)
    layer = GraphConv(fin, fout, allow_zero_in_degree=True).to(cuda).bfloat16()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(fout, generator=torch.Generator().manual_seed(9)).bfloat16() * 0.1)
    gen = torch.Generator().manual_seed(3)
    h = torch.randn(K, fin, generator=gen).bfloat16().to(cuda).requires_grad_(True)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    gout = torch.randn(S, fout, generator=gen).bfloat16().to(cuda)
    out = layer(blk, h, edge_weight=w)
    out.backward(gout)
    src, dst = spec.src.to(cuda), spec.dst.to(cuda)
    od = torch.bincount(src, minlength=K).clamp(min=1).double().pow(-0.5)
    idg = torch.bincount(dst, minlength=S).clamp(min=1).double().pow(-0.5)
    W, b, wd = layer.weight.detach().double(), layer.bias.detach().double(), w.double()
    agg = lambda z, ww: torch.zeros(S, z.shape[1], dtype=torch.float64, device=cuda).index_add_(0, dst, z[src] * ww[:, None])
    hr = h.detach().double().requires_grad_(True)
    x = hr * od[:, None]
    ref = (agg(x @ W, wd) if fin > fout else agg(x, wd) @ W) * idg[:, None] + b
    (ref * gout.double()).sum().backward()
    xa = h.detach().double().abs() * od[:, None]
    mag = agg(xa, wd.abs()) @ W.abs() * idg[:, None] + b.abs()
    gt = torch.zeros(K, fout, dtype=torch.float64, device=cuda).index_add_(0, src, (gout.double().abs() * idg[:, None])[dst] * wd.abs()[:, None])
    mag_d = (gt @ W.abs().t()) * od[:, None]
    r = {"out": assert_within(out, ref, mag, *GCN_K, "graphconv out"), "d_feat": assert_within(h.grad, hr.grad, mag_d, *GCN_K, "graphconv d feat")}
    _report("graphconv-%dx%d" % (fin, fout), r)


def test_full_neighbour_hub_block_with_gradients(cuda):
    """The full-neighbour block of test_fused_kernels_on_a_hub_destination (a destination with every one of its >600 in-edges),
    now with the backward: fused and separate, per element."""
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.graph import full_neighbor_block
    from bliss_gnn_amd.synth import chung_lu_csc
    from bounds import Spec
    ip, ix, ei = chung_lu_csc(4000, 200000, seed=9)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda))
    deg = ip[1:] - ip[:-1]
    hub = int(deg.argmax())
    b0 = max(0, hub - 3)
    blk = full_neighbor_block(g, b0, b0 + 8)
    assert int(deg[hub]) > 600
    spec = Spec(blk.num_src_nodes(), blk.num_dst_nodes(), blk.indptr.cpu().long(), blk.src.cpu().long(), blk.dst.cpu().long())
    H, D = 4, 64
    feat, attn, gg = gat_inputs(spec, H, D, 12, cuda)
    check_gat(spec, run_fused(blk, feat, attn, gg, H, D), feat, attn, gg, H, D, "fused-vec4-4x64-fullnbr")
    check_gat(spec, run_separate(blk, feat, attn, gg, H, D), feat, attn, gg, H, D, "separate-4x64-fullnbr")
