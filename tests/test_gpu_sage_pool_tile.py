"""GPU suite: ``SAGEConv(in, out, "pool")`` on the tile kernels -- nn.sage_pool_tile and ``SAGE(..., transforms="tile")``
(DESIGN.md section 32).

Integer-exact (the method of tests/test_gpu_sage_pool.py): on small-integer data every value at a rounding point of the float64
restatement (tests/pool_tile_ref.py) is an integer of magnitude at most 256 -- asserted on the CPU before anything is compared: a
condition of the test, not a tolerance -- so bf16 storage and fp32 accumulation are exact in any summation order and the output,
d_feat and all five parameter gradients must EQUAL the restatement, on the exact-size block and on its capacity-padded copy with
every pad row of every input NaN.

Random data, stage by stage: each stage of the chain is compared per element with the float64 restatement of THAT stage fed the
GPU's own input to it (the node hands its intermediates out through a debug dict), under the constants tests/bounds.py holds:
dense_k with the stage's term count for the dense products (forward: in + 1 bias, the tail 2 in + 1; d_neigh: out; dh: in + out;
weight gradients: rows + 80 chunk partials), SPMM_K["bf16"] for d_z; equality for neigh / arg (the max commutes with the message's
rounding), for d (dout times 1 / (1 - p) = 2 is exact) and for the zeros of the dropout mask.  Never end to end with a tolerance:
an argmax that flips under rounding moves a gradient by its whole size."""
import math

import pytest
import torch

import pool_tile_ref as ptr
import spmm_max_ref as ref
from bounds import (SPMM_K, Spec, assert_within, dense_k, dgrad_terms, edge_shape_spec, gemm_terms, padded_block, to_block,
                    wgrad_terms)
from test_gpu_sage_pool import BS, _graph, _int_spec, _ints

pytestmark = pytest.mark.gpu

GRADS = ("fc_pool.weight", "fc_pool.bias", "fc_neigh.weight", "fc_self.weight", "fc_self.bias")


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _layer(cuda, fin, fout, c=None):
    from bliss_gnn_amd.nn import SAGEConv
    layer = SAGEConv(fin, fout, "pool").to(cuda).bfloat16()
    if c is not None:
        dev = lambda v: v.bfloat16().to(cuda)
        with torch.no_grad():
            layer.fc_pool.weight.copy_(dev(c["Wp"])), layer.fc_pool.bias.copy_(dev(c["bp"])), layer.fc_neigh.weight.copy_(dev(c["Wn"]))
            layer.fc_self.weight.copy_(dev(c["Ws"])), layer.fc_self.bias.copy_(dev(c["bs"]))
    return layer


# ------------------------------------------------------------------------------------------------ the layer, exact integers
# (in, out): the probabilities with which an element of h, W_pool and W_neigh / W_self is kept (else zeroed), the order of
# tests/test_gpu_sage_pool.py::_int_case's generator.  (16, 8), (8, 16): the basic layer; (24, 8): K not a multiple of 16;
# (257, 16): a second fc_pool column block of width 1; (272, 8): two blocks; (602, 8): three blocks, the Reddit width;
# (1000, 8): four blocks, and a tail whose two staged operands pass bliss_tile_gemm's LDS -- the wide entry point
INT_CASES = {(16, 8): (1.0, 0.6, 0.6), (8, 16): (1.0, 0.6, 0.6), (24, 8): (1.0, 0.6, 0.6), (257, 16): (0.5, 0.05, 0.1),
             (272, 8): (0.5, 0.05, 0.1), (602, 8): (0.3, 0.02, 0.05), (1000, 8): (0.3, 0.01, 0.03)}
_INT = {}


def _one_row_spec():
    """S = 1: one destination (itself source 0) with three in-edges among 5 sources."""
    return Spec(5, 1, torch.tensor([0, 3]), torch.tensor([1, 2, 4]), torch.tensor([0, 0, 0]))


def _int_case(fin, fout, relu, spec=None):
    """Integer operands and the float64 restatement (computed once per case); asserts the exactness condition."""
    key = (fin, fout, relu, spec is None)
    if key in _INT:
        return _INT[key]
    spec = _int_spec() if spec is None else spec
    S, K, B = spec.S, spec.K, spec.B
    kh, kp, kw = INT_CASES[(fin, fout)]
    gen = torch.Generator().manual_seed(100 + fin)
    c = dict(h=_ints(gen, (K, fin), -1, 1, kh), w=_ints(gen, (B,), 1, 2), gout=_ints(gen, (S, fout), -1, 1, 0.5),
             Wp=_ints(gen, (fin, fin), -1, 1, kp), bp=_ints(gen, (fin,), -1, 1), Wn=_ints(gen, (fout, fin), -1, 1, kw),
             Ws=_ints(gen, (fout, fin), -1, 1, kw), bs=_ints(gen, (fout,), -2, 2))
    pts = ptr.layer(spec.src, spec.dst, S, c["h"], c["w"], c["Wp"], c["bp"], c["Wn"], c["Ws"], c["bs"], relu=relu, gout=c["gout"], sim=False)
    worst = 0.0
    for k, v in pts.items():
        if k != "arg":
            assert bool((v == v.round()).all()) and float(v.abs().max()) <= 256, (k, float(v.abs().max()))
            worst = max(worst, float(v.abs().max()))
    if spec.S > 1:
        assert float(pts["m"].max()) > 2 and bool((pts["d_z"] != pts["d_a"]).any())      # (weights matter, the ReLU mask matters)
        assert int((pts["arg"] >= 0).sum()) == (S - 1) * fin                              # (one destination without edges)
        if relu:
            assert bool((pts["pre"] < 0).any()) and bool((pts["d"] != c["gout"]).any())   # (the tail's mask matters)
    print("INT-CASE %d -> %d relu=%s largest magnitude %g" % (fin, fout, relu, worst))
    _INT[key] = (spec, c, pts)
    return _INT[key]


def _run_int(cuda, spec, c, relu, padded):
    """The node on the exact-size block, or on bounds.padded_block with the live words set and every pad row of h, the edge
    weights and d out NaN.  Returns (out, d_feat, {parameter gradients}, debug dict)."""
    from bliss_gnn_amd.nn import sage_pool_tile
    S, K, B = spec.S, spec.K, spec.B
    fin, fout = c["Wp"].shape[0], c["Wn"].shape[0]
    layer = _layer(cuda, fin, fout, c)
    if padded:
        blk = padded_block(spec, cuda)
        blk._counts_dev[3] = K                                                             # the live source count (word 3)
        Sc, Kc, Bc = blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()
    else:
        blk, Sc, Kc, Bc = to_block(spec, cuda), S, K, B
    pad = lambda v, n: torch.cat([v, torch.full((n - v.shape[0],) + tuple(v.shape[1:]), float("nan"), dtype=v.dtype)]).bfloat16().to(cuda)
    h = pad(c["h"], Kc).requires_grad_(True)
    dbg = {}
    out, out_norm, in_norm = sage_pool_tile(blk, h, pad(c["w"], Bc), layer, relu, 0.0, None, 0, dbg)
    out.backward(pad(c["gout"], Sc))
    return out.detach(), h.grad, {k: p.grad for k, p in layer.named_parameters()}, dbg


@pytest.mark.parametrize("padded", [False, True], ids=["exact", "padded"])
@pytest.mark.parametrize("fin,fout", list(INT_CASES))
def test_pool_tile_layer_on_integers_equals_the_restatement(cuda, fin, fout, padded):
    from bliss_gnn_amd.nn import _tile_gemm_fits
    for relu in (False, True):                                      # the output layer's form, a hidden layer's
        spec, c, pts = _int_case(fin, fout, relu)
        S, K = spec.S, spec.K
        out, d_feat, grads, dbg = _run_int(cuda, spec, c, relu, padded)
        assert dbg["tail_entry"] == ("bliss_tile_gemm" if _tile_gemm_fits(fin, fin, fout) else "bliss_tile_gemm_wide")
        assert (dbg["tail_entry"] == "bliss_tile_gemm_wide") == (fin == 1000)
        what = "%d -> %d relu=%s %s" % (fin, fout, relu, "padded" if padded else "exact")
        assert torch.equal(out[:S].double().cpu(), pts["out"]), what + " out"
        assert torch.equal(d_feat[:K].double().cpu(), pts["d_feat"]), what + " d_feat"
        assert sorted(grads) == sorted(GRADS)
        for k in GRADS:
            assert grads[k] is not None and torch.equal(grads[k].double().cpu(), pts[k]), what + " " + k
        for k in ("pooled", "neigh", "d", "d_neigh", "d_z"):
            rows = K if k in ("pooled", "d_z") else S
            assert torch.equal(dbg[k][:rows].double().cpu(), pts[k]), what + " " + k
        assert torch.equal(dbg["arg"][:S].cpu(), pts["arg"])
        # pad rows: exactly zero (+0 bits) in out and d_feat; no NaN in anything the layer hands on
        assert not bool(_bits(out[S:]).any()) and not bool(_bits(d_feat[K:]).any()), what + " pad rows"
        for k, t in dict(grads, out=out, d_feat=d_feat).items():
            assert bool(torch.isfinite(t.float()).all()), what + " " + k


def test_pool_tile_layer_with_one_destination(cuda):
    """S = 1 (one 32-row tile with one live row, a weight gradient over one row)."""
    for relu in (False, True):
        spec, c, pts = _int_case(16, 8, relu, _one_row_spec())
        for padded in (False, True):
            out, d_feat, grads, _ = _run_int(cuda, spec, c, relu, padded)
            assert torch.equal(out[:1].double().cpu(), pts["out"]) and torch.equal(d_feat[:spec.K].double().cpu(), pts["d_feat"])
            assert all(torch.equal(grads[k].double().cpu(), pts[k]) for k in GRADS)
            assert not bool(_bits(out[1:]).any()) and not bool(_bits(d_feat[spec.K:]).any())


# ------------------------------------------------------------------------------------------------ random data, stage by stage
_EDGE = []


def _edge():
    if not _EDGE:
        _EDGE.append(edge_shape_spec())
    return _EDGE[0]


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("fin,fout", [(48, 16), (16, 48), (260, 41)])
def test_pool_tile_layer_stage_by_stage(cuda, fin, fout, p):
    from bliss_gnn_amd import ops
    from bliss_gnn_amd.nn import sage_pool_tile
    spec = _edge()
    S, K, B = spec.S, spec.K, spec.B
    blk = to_block(spec, cuda)
    torch.manual_seed(fin)
    layer = _layer(cuda, fin, fout)
    gen = torch.Generator().manual_seed(3 + fin)
    with torch.no_grad():
        layer.fc_pool.bias.copy_((torch.randn(fin, generator=gen) * 0.1).bfloat16())
        layer.fc_self.bias.copy_((torch.randn(fout, generator=gen) * 0.1).bfloat16())
    h = torch.randn(K, fin, generator=gen).bfloat16().to(cuda).requires_grad_(True)
    w = (torch.rand(B, generator=gen) + 0.05).bfloat16().to(cuda)
    gout = torch.randn(S, fout, generator=gen).bfloat16().to(cuda)
    ctr = torch.zeros(2 + 64, dtype=torch.int64, device=cuda) if p > 0 else None
    dbg = {}
    out, out_norm, in_norm = sage_pool_tile(blk, h, w, layer, True, p, ctr, 1234, dbg)
    out.backward(gout)
    out = out.detach()
    Wp, bp, Wn, Ws, bs = (t.detach() for t in (layer.fc_pool.weight, layer.fc_pool.bias, layer.fc_neigh.weight, layer.fc_self.weight,
                                                layer.fc_self.bias))
    hd = h.detach()
    what = "%d -> %d p=%g " % (fin, fout, p)
    r = {}
    # the norms: ops.embed_norm's bits on the same rows
    assert torch.equal(_bits(in_norm), _bits(ops.embed_norm(hd))) and torch.equal(_bits(out_norm), _bits(ops.embed_norm(out)))
    # pooled = relu(fc_pool(h)): in + 1 terms, one rounding
    z, mz = gemm_terms(hd, Wp, bias=bp)
    r["pooled"] = assert_within(dbg["pooled"], z.clamp(min=0), mz, *dense_k(fin + 1), what + "pooled")
    assert bool((dbg["pooled"] >= 0).all()) and bool((dbg["pooled"] == 0).any())
    # neigh, arg: exact on the GPU's pooled
    _, r_neigh, r_arg = ref.forward(spec.src, spec.dst, S, dbg["pooled"].cpu(), w.cpu())
    assert torch.equal(dbg["arg"].cpu(), r_arg) and torch.equal(_bits(dbg["neigh"]), _bits(r_neigh))
    # out: 2 in + 1 terms in one accumulator, ReLU, dropout (the scale 2 is exact), one rounding
    pre, mpre = gemm_terms(dbg["neigh"], Wn, a2=hd, w2=Ws, bias=bs, m2=S)
    scale = 1.0 / (1.0 - p)
    dropped = (out == 0) & (pre.clamp(min=0) * scale - (2.0 ** -8 * mpre * scale * dense_k(2 * fin + 1)[1] + 2.0 ** -133) > 0) if p > 0 \
        else torch.zeros_like(out, dtype=torch.bool)
    want = torch.where(dropped, torch.zeros_like(pre), pre.clamp(min=0) * scale)
    r["out"] = assert_within(out, want, mpre * scale, *dense_k(2 * fin + 1), what + "out")
    assert not bool(_bits(out[dropped]).any())                                       # a dropped element is +0, exactly
    if p > 0:
        live = pre > 2.0 ** -8 * mpre                                               # clearly positive before the dropout
        n, k = int(live.sum()), int((dropped & live).sum())
        assert abs(k - p * n) <= 5 * math.sqrt(n * p * (1 - p)) + 1, (k, n)
    else:
        assert not bool(dropped.any())
    # d: the epilogue backward, exact -- dout * 2 (or dout) where out > 0, else +0
    d = dbg["d"]
    assert torch.equal(_bits(d), _bits(torch.where(out > 0, (gout.float() * scale).bfloat16(), torch.zeros_like(gout))))
    # the tail's weight gradients: S rows (+ 80 chunk partials)
    dwn, mwn, db, mdb = wgrad_terms(d, dbg["neigh"], S)
    dws, mws, _, _ = wgrad_terms(d, hd[:S], S)
    g = {k: q.grad for k, q in layer.named_parameters()}
    r["dWn"] = assert_within(g["fc_neigh.weight"], dwn, mwn, *dense_k(S + 80), what + "dW_neigh")
    r["dWs"] = assert_within(g["fc_self.weight"], dws, mws, *dense_k(S + 80), what + "dW_self")
    r["dbs"] = assert_within(g["fc_self.bias"], db, mdb, *dense_k(S + 80), what + "db_self")
    # d_neigh = d W_neigh: out terms
    r["d_neigh"] = assert_within(dbg["d_neigh"], *dgrad_terms(d, Wn), *dense_k(fout), what + "d_neigh")
    # d_z: the routed backward under the mask pooled > 0, on the GPU's d_neigh, arg and pooled
    rz, mz2 = ptr.masked_backward(spec.src, K, dbg["d_neigh"].cpu(), dbg["arg"].cpu(), dbg["pooled"].cpu(), w.cpu())
    r["d_z"] = assert_within(dbg["d_z"].cpu(), rz, mz2, *SPMM_K["bf16"], what + "d_z")
    plain, _ = ref.backward(spec.src, K, dbg["d_neigh"].cpu(), dbg["arg"].cpu(), w.cpu())
    assert not bool(_bits(dbg["d_z"])[(dbg["pooled"] == 0).cpu()].any())
    assert bool(((plain != 0) & (dbg["pooled"].cpu() == 0)).any()), "the ReLU mask removes nothing on this case"
    # fc_pool's gradients: K rows (+ 80 chunk partials)
    dwp, mwp, dbp, mbp = wgrad_terms(dbg["d_z"], hd, K)
    r["dWp"] = assert_within(g["fc_pool.weight"], dwp, mwp, *dense_k(K + 80), what + "dW_pool")
    r["dbp"] = assert_within(g["fc_pool.bias"], dbp, mbp, *dense_k(K + 80), what + "db_pool")
    # dh = d_z W_pool + d W_self on the first S rows: in + out terms, one accumulator, one rounding
    r["dh"] = assert_within(h.grad, *dgrad_terms(dbg["d_z"], Wp, a2=d, w2=Ws, m2=S), *dense_k(fin + fout), what + "dh")
    print("RATIO pool-tile %s" % what + " ".join("%s %.3f" % kv for kv in r.items()))


@pytest.mark.parametrize("fin,fout", [(272, 8), (602, 16)])
def test_lazy_rows_input_is_bit_equal_to_the_materialised_input(cuda, fin, fout):
    """A LazyRows input: the first launch gathers through ids (both of its column blocks) and writes the rows out; the third
    block of 602, the tail and the backward read that copy.  Everything bit-equal to the same layer on table[ids]."""
    from bliss_gnn_amd.nn import LazyRows, sage_pool_tile
    spec = _int_spec()
    blk = to_block(spec, cuda)
    torch.manual_seed(fin)
    layer = _layer(cuda, fin, fout)
    gen = torch.Generator().manual_seed(11)
    table = torch.randn(500, fin, generator=gen).bfloat16().to(cuda)
    ids = torch.randint(0, 500, (spec.K,), generator=gen).to(torch.int32).to(cuda)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    gout = torch.randn(spec.S, fout, generator=gen).bfloat16().to(cuda)
    got = []
    for x in (LazyRows(table, ids), table[ids.long()].contiguous()):
        layer.zero_grad(set_to_none=True)
        dbg = {}
        out, out_norm, in_norm = sage_pool_tile(blk, x, w, layer, True, 0.0, None, 0, dbg)
        out.backward(gout)
        got.append([out, out_norm, in_norm, dbg["rows"], dbg["pooled"]] + [layer.get_parameter(k).grad for k in GRADS])
    assert torch.equal(_bits(got[0][3]), _bits(table[ids.long()]))
    for a, b in zip(*got):
        assert a is not None and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the model
def _sage(cuda, transforms, agg, feat=None, hidden=16):
    from bliss_gnn_amd.model import SAGE
    from test_gpu_sage_pool import CLASSES, FEAT
    torch.manual_seed(0)
    m = SAGE(FEAT if feat is None else feat, hidden, CLASSES, 3, torch.relu, 0.1, transforms=transforms, aggregator_type=agg).to(cuda).bfloat16()
    m.train()
    return m


def _two_steps(cuda, model):
    from bliss_gnn_amd import fit
    from bliss_gnn_amd.train import TrainStep
    g, perm = _graph(cuda)
    torch.manual_seed(4)
    step = TrainStep(g, fit.make_sampler("labor", [5, 5, 5]), model, lr=0.01)
    return [float(step(perm[i * BS:(i + 1) * BS])) for i in range(2)]


def test_mean_tile_model_has_the_bits_of_auto(cuda):
    a, t = _sage(cuda, "auto", "mean"), _sage(cuda, "tile", "mean")
    assert a._mfma_ok(next(a.parameters())) and t._mfma_path(next(t.parameters())) is True
    la, lt = _two_steps(cuda, a), _two_steps(cuda, t)
    assert all(math.isfinite(x) for x in la) and la == lt
    for (k, p), q in zip(a.named_parameters(), t.parameters()):
        assert torch.equal(_bits(p), _bits(q)), k


def test_pool_tile_model_trains_and_sets_every_embed_norm(cuda):
    """Eager steps move every parameter; every block's embed_norm has ops.embed_norm's bits of that layer's input; forward equals
    forward_last(forward_hidden(...)), and forward_last_parts is None."""
    from bliss_gnn_amd import fit, ops
    m = _sage(cuda, "tile", "pool")
    before = [p.detach().clone() for p in m.parameters()]
    losses = _two_steps(cuda, m)
    assert all(math.isfinite(x) and abs(x) < 1e4 for x in losses), losses
    for (n, p), q in zip(m.named_parameters(), before):
        assert bool(torch.isfinite(p.float()).all()) and not torch.equal(p, q), n
    m.eval()
    g, perm = _graph(cuda)
    _, _, mfgs = fit.make_sampler("labor", [5, 5, 5]).sample_blocks(g, perm[:BS])
    x = mfgs[0].srcdata["features"]
    with torch.no_grad():
        full = m(mfgs, x)
        norms = [b.srcdata["embed_norm"].clone() for b in mfgs]
        hidden = m.forward_hidden(mfgs, mfgs[0].srcdata.lazy("features"))
        assert m.forward_last_parts(mfgs, hidden) is None
        assert torch.equal(_bits(m.forward_last(mfgs, hidden)), _bits(full))
        # the layers' inputs, recomputed layer by layer
        from bliss_gnn_amd.nn import sage_pool_tile
        h = x
        for l, (layer, blk) in enumerate(zip(m.layers, mfgs)):
            assert torch.equal(_bits(norms[l]), _bits(ops.embed_norm(h.contiguous()))), l
            assert torch.equal(_bits(blk.srcdata["embed_norm"]), _bits(norms[l]))
            ew = blk.edata["edge_weights"] if "edge_weights" in blk.edata else None
            h = sage_pool_tile(blk, h, ew, layer, l < 2, 0.0, None, 0)[0]
        assert torch.equal(_bits(h), _bits(full))


def test_tile_models_refuse_layers_past_the_limits_at_the_first_forward(cuda):
    x = torch.zeros(8, 1433, dtype=torch.bfloat16, device=cuda)
    for agg in ("mean", "pool"):
        m = _sage(cuda, "tile", agg, feat=1433)
        with pytest.raises(NotImplementedError, match="layer 0.*in_feats <= 1024"):
            m([None] * 3, x)
    m = _sage(cuda, "tile", "pool", hidden=257)
    with pytest.raises(NotImplementedError, match="layer 0.*out_feats <= 256"):
        m([None] * 3, x[:, :24])
    m = _sage(cuda, "tile", "pool").float()
    with pytest.raises(NotImplementedError, match="bf16"):
        m([None] * 3, x[:, :24])
