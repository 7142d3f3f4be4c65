"""GPU suite: the max-reduce message passing of SAGEConv('pool') (csrc/spmm_max.hip) against the CPU
restatement of tests/spmm_max_ref.py.

Forward: ``out`` bit-equal and ``arg`` equal everywhere -- exact: the only rounding is the message's, and max commutes with it.
Backward: d h per element under bounds.SPMM_K["bf16"] = (1, 0.25): every element is an fp32 sum of a SUBSET of the terms of the
weighted SpMM backward that constant was derived for (rows of at most 16 384 terms, one rounding at the store), each term one
exact fp32 product of two bf16 values."""
import pytest
import torch

import spmm_max_ref as ref
from bounds import SPMM_K, SPMM_MAX_ROW, Spec, assert_within, edge_shape_spec, padded_block, spmm_band_spec, to_block

pytestmark = pytest.mark.gpu
_SPECS = {}


def _spec(name):
    if name not in _SPECS:
        _SPECS[name] = {"edge": edge_shape_spec, "band100k": lambda: spmm_band_spec(100000, 21),
                        "band210k": lambda: spmm_band_spec(210000, 22)}[name]()
    return _SPECS[name]


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _run(blk, h, w, gout):
    """(out, arg, d h) of max_aggregate on the GPU; ``h`` may be a strided view."""
    from bliss_gnn_amd.nn import max_aggregate
    hd = h.detach().requires_grad_(True)
    out, arg = max_aggregate(blk, hd, w, return_arg=True)
    out.backward(gout)
    return out.detach(), arg, hd.grad


def _check(spec, blk, h, w, gout, what):
    """One case against the restatement on the CPU (``blk`` may be the capacity-padded copy of ``spec``: its true rows are
    compared).  Returns the largest d h error / bound and the GPU tensors."""
    out, arg, dh = _run(blk, h, w, gout)
    hc, wc, gc = h.detach().cpu()[:spec.K], None if w is None else w.cpu()[:spec.B], gout.cpu()[:spec.S]
    _, r_out, r_arg = ref.forward(spec.src, spec.dst, spec.S, hc, wc)
    r_dh, r_mag = ref.backward(spec.src, spec.K, gc, r_arg, wc)
    bad = int((arg[:spec.S].cpu() != r_arg).sum())
    assert bad == 0, "%s: arg differs in %d of %d elements" % (what, bad, r_arg.numel())
    assert torch.equal(_bits(out[:spec.S]), _bits(r_out)), what + ": out bits"
    ratio = assert_within(dh[:spec.K].cpu(), r_dh, r_mag, *SPMM_K["bf16"], what + " d h")
    return ratio, (out, arg, dh)


@pytest.mark.parametrize("weighted", [True, False], ids=["w", "1"])
@pytest.mark.parametrize("dim", [1, 3, 4, 41, 64, 260])
def test_edge_shapes(cuda, dim, weighted):
    """The edge-shape block (in-degrees 0, 1, 2, 15..17, 63..65, 255..257, 512, 513, 1500, a 12 000-edge hub, a source with
    > 3000 out-edges, 16 sources that send nothing; chunk band 16); for dim % 4 == 0 also h as a column slice 4 bytes off
    alignment with a row stride != dim (the scalar path)."""
    from bliss_gnn_amd import _lib
    spec = _spec("edge")
    assert int(_lib.lib.bliss_spmm_chunk_edges(spec.B)) == 16
    assert int(spec.in_degrees().max()) <= SPMM_MAX_ROW and 3000 < int(spec.out_degrees().max()) <= SPMM_MAX_ROW
    assert int((spec.out_degrees() == 0).sum()) >= 16 and int(spec.in_degrees().min()) == 0
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(40 + dim)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda) if weighted else None
    hfull = torch.randn(spec.K, dim + 6, generator=gen).bfloat16().to(cuda)
    gout = torch.randn(spec.S, dim, generator=gen).bfloat16().to(cuda)
    layouts = [("contig", hfull[:, :dim].contiguous())]
    if dim % 4 == 0:
        sl = hfull[:, 2:2 + dim]
        assert sl.data_ptr() % 8 == 4 and sl.stride(0) != dim
        layouts.append(("slice", sl))
    for lay, h in layouts:
        r, _ = _check(spec, blk, h, w, gout, "edge d%d %s %s" % (dim, "w" if weighted else "1", lay))
        print("RATIO spmm-max-edge d%d-%s-%s-dh %.3f" % (dim, "w" if weighted else "1", lay, r))


@pytest.mark.parametrize("name,ec", [("band100k", 32), ("band210k", 64)])
def test_chunk_bands(cuda, name, ec):
    """Chunk lengths 32 and 64 (50 000 and 200 000 edges up), dim 64, weighted."""
    from bliss_gnn_amd import _lib
    spec = _spec(name)
    assert int(_lib.lib.bliss_spmm_chunk_edges(spec.B)) == ec
    assert int(spec.in_degrees().max()) <= SPMM_MAX_ROW and int(spec.out_degrees().max()) <= SPMM_MAX_ROW
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(50 + ec)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    h = torch.randn(spec.K, 64, generator=gen).bfloat16().to(cuda)
    gout = torch.randn(spec.S, 64, generator=gen).bfloat16().to(cuda)
    r, _ = _check(spec, blk, h, w, gout, name)
    print("RATIO spmm-max-%s dh %.3f" % (name, r))


def _tie_spec():
    """Row 0: 5 edges, row 1: 40 edges from the 40 distinct sources 3..42 (edges 5..44: chunks 0, 1 and 2 of 16), row 2: 3 edges,
    row 3: none.  Rows 0 and 2 draw from sources 43..49."""
    degs = torch.tensor([5, 40, 3, 0])
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), degs.cumsum(0)])
    src = torch.cat([torch.tensor([43, 44, 45, 46, 47]), torch.arange(3, 43), torch.tensor([48, 49, 43])])
    dst = torch.repeat_interleave(torch.arange(4), degs)
    return Spec(50, 4, indptr, src, dst)


@pytest.mark.parametrize("dim", [8, 5])
def test_tie_across_chunk_boundaries_goes_to_the_first_edge(cuda, dim):
    """40 identical source rows feed one destination whose edges span three chunks: arg is the row's first edge in every
    column, with weights (all 1.5) and without, and d h of that row's sources is non-zero only in the first one's row."""
    spec = _tie_spec()
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(7)
    h = torch.randn(spec.K, dim, generator=gen).bfloat16()
    h[3:43] = h[3]
    gout = (torch.randn(spec.S, dim, generator=gen).abs() + 0.5).bfloat16().to(cuda)
    for w in (None, torch.full((spec.B,), 1.5).bfloat16().to(cuda)):
        _, (out, arg, dh) = _check(spec, blk, h.to(cuda), w, gout, "tie row")
        assert bool((arg[1] == 5).all()), arg[1].tolist()
        assert bool((dh[3] != 0).all()) and not bool(dh[4:43].any())
        assert bool((arg[3] == -1).all()) and not bool(out[3].any())


def test_rounded_tie_goes_to_the_first_edge(cuda):
    """w = (1.0, 1.0078125) on h = (1.0, 0.99609375): the fp32 products are 1.0 and 1.00388..., both messages are bf16 1.0, so
    the first edge wins; comparing unrounded products would pick the second."""
    spec = Spec(2, 1, torch.tensor([0, 2]), torch.tensor([0, 1]), torch.tensor([0, 0]))
    blk = to_block(spec, cuda)
    h = torch.tensor([[1.0, 1.0, 1.0, 1.0], [0.99609375, 0.99609375, 2.0, 0.5]]).bfloat16().to(cuda)
    w = torch.tensor([1.0, 1.0078125]).bfloat16().to(cuda)
    assert float(w[1].float() * h[1, 0].float()) > 1.0
    gout = torch.ones(1, 4).bfloat16().to(cuda)
    _, (out, arg, dh) = _check(spec, blk, h, w, gout, "rounded tie")
    assert arg[0].tolist() == [0, 0, 1, 0] and out[0, :2].tolist() == [1.0, 1.0]
    assert dh[:, 0].tolist() == [1.0, 0.0]


def test_block_without_edges(cuda):
    """No edges at all (a full-neighbour chunk of isolated nodes): no chunk is launched, the fix-ups clear every row."""
    z = torch.zeros(0, dtype=torch.int64)
    spec = Spec(4, 3, torch.zeros(4, dtype=torch.int64), z, z)
    blk = to_block(spec, cuda)
    h = torch.ones(4, 8).bfloat16().to(cuda)
    _, (out, arg, dh) = _check(spec, blk, h, None, torch.ones(3, 8).bfloat16().to(cuda), "no edges")
    assert not bool(_bits(out).any()) and bool((arg == -1).all()) and not bool(_bits(dh).any())


def test_capacity_padded_block(cuda):
    """bounds.padded_block of the edge-shape block with garbage h rows past K and garbage gout rows past S: the true rows have
    the unpadded block's bits, padded output rows are zero with arg -1, d h rows past K are zero."""
    spec = _spec("edge")
    S, K, B = spec.S, spec.K, spec.B
    blk, pad = to_block(spec, cuda), padded_block(spec, cuda)
    Sc, Kc, Bc = pad.num_dst_nodes(), pad.num_src_nodes(), pad.num_edges()
    gen = torch.Generator().manual_seed(8)
    for dim in (64, 41):
        h = torch.randn(Kc, dim, generator=gen).bfloat16()
        h[K:] = (torch.randn(Kc - K, dim, generator=gen) * 1e4).bfloat16()
        gout = torch.randn(Sc, dim, generator=gen).bfloat16()
        gout[S:] = float("nan")
        w = (torch.rand(Bc, generator=gen) + 0.05).bfloat16()
        w[B:] = 1e6
        h, gout, w = h.to(cuda), gout.to(cuda), w.to(cuda)
        u_out, u_arg, u_dh = _run(blk, h[:K], w[:B], gout[:S])
        p_out, p_arg, p_dh = _run(pad, h, w, gout)
        assert torch.equal(_bits(p_out[:S]), _bits(u_out)) and torch.equal(p_arg[:S], u_arg) and torch.equal(_bits(p_dh[:K]), _bits(u_dh))
        assert not bool(_bits(p_out[S:]).any()) and bool((p_arg[S:] == -1).all()) and not bool(_bits(p_dh[K:]).any())
        _check(spec, pad, h, w, gout, "padded d%d" % dim)


def test_two_runs_give_identical_bits(cuda):
    spec = _spec("band100k")
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(9)
    h = torch.randn(spec.K, 64, generator=gen).bfloat16().to(cuda)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    gout = torch.randn(spec.S, 64, generator=gen).bfloat16().to(cuda)
    a, b = _run(blk, h, w, gout), _run(blk, h, w, gout)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))


def test_update_all_with_fn_max(cuda):
    """``update_all(fn.u_mul_e | fn.copy_u, fn.max)`` writes max_aggregate's tensor into dstdata; the per-head GAT branch and an
    unknown reduce keep refusing."""
    from bliss_gnn_amd import function as fn
    from bliss_gnn_amd.nn import max_aggregate
    spec = _spec("edge")
    blk = to_block(spec, cuda)
    gen = torch.Generator().manual_seed(10)
    h = torch.randn(spec.K, 12, generator=gen).bfloat16().to(cuda)
    w = (torch.rand(spec.B, generator=gen) + 0.05).bfloat16().to(cuda)
    blk.srcdata["h"], blk.edata["w"] = h, w
    blk.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "neigh"))
    assert torch.equal(_bits(blk.dstdata["neigh"]), _bits(max_aggregate(blk, h, w)))
    blk.update_all(fn.copy_u("h", "m"), fn.max("m", "neigh1"))
    assert torch.equal(_bits(blk.dstdata["neigh1"]), _bits(max_aggregate(blk, h, None)))
    blk.srcdata["h3"], blk.edata["w3"] = h.view(spec.K, 3, 4), w.view(-1, 1, 1).expand(-1, 3, 1).contiguous()
    with pytest.raises(NotImplementedError):
        blk.update_all(fn.u_mul_e("h3", "w3", "m"), fn.max("m", "bad"))
    with pytest.raises(NotImplementedError, match="max"):
        blk.update_all(fn.copy_u("h", "m"), fn._Reduce("min", "m", "bad"))
