"""GPU suite (-m gpu): the recurrent neighbour aggregation of csrc/lstm.hip through nn.lstm_aggregate and torch.ops.bliss.lstm_agg
(DESIGN.md section 37), at the smallest shapes at which the kernels can go wrong: T = bliss_lstm_tile_rows(), n_dst in
{1, T - 1, T, T + 1, 2 T + 5}, degrees from [0, 1, 2, 3, 15, 16, 17, 33, 70] (a tile whose rows all have degree 0, a tile whose last row
alone is the longest, a block without edges, parallel edges, sources that are no destinations: lstm_agg_ref.degree_cases),
D in {1, 5, 8, 40, 64, 256}, weighted and not, h aligned and as a column slice of a wider matrix.

Acceptance, for each of out, d h, d W_ih, d W_hh, d b_ih, d b_hh, d w, on the cases with at least 32 destinations that have edges:

    max |kernel - truth64| <= max |chain_bf16 - truth64|

on the same bf16-valued inputs -- the right side is the error of the bf16 arithmetic a DGL model runs today, computed per case at test
time from the reference alone; no further margin.  tests/test_lstm_agg_ref.py holds the model of the kernel's rounding points to the
same inequality on the same cases.  Exact checks on every case: rows without edges are +0; two runs give the same bits; with w
requiring nothing, out and d h have the bits of the run where it does; with degree at most 1 everywhere d W_hh is exactly 0; a
capacity-padded block with NaN planted past the live counts gives the bits of the exact-size block and +0 beyond in everything the
kernels write -- out, hprev, dgate, d P, d w -- (on the op: the input projection and its gradients are library GEMMs over all rows,
and so are d W_hh and d b, which are held to one bf16 step of the exact-size block's)."""
import functools

import pytest
import torch

import bounds
import lstm_agg_ref as ref
from bliss_gnn_amd import _lib

pytestmark = pytest.mark.gpu

T = _lib.lib.bliss_lstm_tile_rows()
CASES = ref.degree_cases(T)


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(name, D, weighted):
    """The block, the inputs and the two references of a case, computed once and left unchanged."""
    degs = CASES[name]
    spec = ref.make_spec(degs, 3)
    inp, gout = ref.make_inputs(spec, D, ref.input_seed(name, D), weighted)
    truth = chain = None
    if ref.asserted(degs):
        truth, chain = ref.truth64(spec, inp, gout), ref.chain_bf16(spec, inp, gout)
    return spec, inp, gout, truth, chain


def _lstm(cuda, inp, D):
    lstm = torch.nn.LSTM(D, D, batch_first=True).to(cuda).bfloat16()
    with torch.no_grad():
        for name, key in (("weight_ih_l0", "W_ih"), ("weight_hh_l0", "W_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(lstm, name).copy_(inp[key].to(cuda))
    return lstm


def _run(cuda, blk, spec, inp, gout, D, sliced=False, w_grad=True):
    """One forward and backward of nn.lstm_aggregate; every result as float64 on the CPU, and the raw bf16 tensors."""
    from bliss_gnn_amd.nn import lstm_aggregate
    lstm = _lstm(cuda, inp, D)
    hb = inp["h"].bfloat16().to(cuda)
    if sliced:                                               # columns 1 .. D of a wider matrix: no row is 16- or 8-byte aligned
        wide = torch.zeros(spec.K, D + 3, dtype=torch.bfloat16, device=cuda)
        wide[:, 1:D + 1] = hb
        leaf = wide.requires_grad_()
        h = leaf[:, 1:D + 1]
    else:
        leaf = hb.clone().requires_grad_()
        h = leaf
    w = None
    if inp["w"] is not None:
        w = inp["w"].bfloat16().to(cuda).requires_grad_(w_grad)
    out = lstm_aggregate(blk, h, lstm, w)
    out.backward(gout.bfloat16().to(cuda))
    dh = leaf.grad[:, 1:D + 1] if sliced else leaf.grad
    raw = {"out": out.detach(), "dh": dh, "dW_ih": lstm.weight_ih_l0.grad, "dW_hh": lstm.weight_hh_l0.grad,
           "db_ih": lstm.bias_ih_l0.grad, "db_hh": lstm.bias_hh_l0.grad}
    if w is not None and w_grad:
        raw["dw"] = w.grad
    assert all(v is not None and v.dtype == torch.bfloat16 for v in raw.values())
    return raw


@pytest.mark.parametrize("weighted", [False, True], ids=["copy_u", "u_mul_e"])
@pytest.mark.parametrize("D", ref.DIMS)
@pytest.mark.parametrize("name", list(CASES))
def test_lstm_aggregate(cuda, name, D, weighted):
    spec, inp, gout, truth, chain = _case(name, D, weighted)
    blk = bounds.to_block(spec, cuda)
    deg = spec.in_degrees()
    runs = {"aligned": _run(cuda, blk, spec, inp, gout, D), "sliced": _run(cuda, blk, spec, inp, gout, D, sliced=True)}
    for how, raw in runs.items():
        assert raw["out"].shape == (spec.S, D) and raw["dh"].shape == (spec.K, D)
        assert not _bits(raw["out"])[(deg == 0).to(cuda)].any(), "a row without edges is +0"
        assert all(bool(torch.isfinite(v.float()).all()) for v in raw.values())
        if int(deg.max()) <= 1:
            assert not raw["dW_hh"].any(), "no second step anywhere: no recurrent gradient"
        if truth is not None:
            figures = {k: (ref.max_err(raw[k].double().cpu(), truth[k]), ref.max_err(chain[k], truth[k])) for k in ref.TENSORS if k in truth}
            print(name, D, weighted, how, {k: "%.3g / %.3g" % v for k, v in figures.items()})
            for k, (got, bound) in figures.items():
                assert got <= bound, (how, k, got, bound)
    # two runs give the same bits
    again = _run(cuda, blk, spec, inp, gout, D)
    for k, v in runs["aligned"].items():
        assert torch.equal(_bits(v), _bits(again[k])), k
    # edge weights that require nothing: nothing else moves
    if weighted:
        plain = _run(cuda, blk, spec, inp, gout, D, w_grad=False)
        assert "dw" not in plain
        for k in ("out", "dh", "dW_ih", "dW_hh", "db_ih", "db_hh"):
            assert torch.equal(_bits(plain[k]), _bits(runs["aligned"][k])), k


def _op(cuda, blk, p, w, lstm, gout):
    """torch.ops.bliss.lstm_agg forward and backward on ``p``: what the kernels write (out, hprev, dgate, dp, dw) and the two
    library reductions over it (dW_hh, db)."""
    from bliss_gnn_amd import ops
    from bliss_gnn_amd.nn import _aggregate_operands
    p = p.clone().requires_grad_()
    w = None if w is None else w.clone().requires_grad_()
    _h, wq, counts, _ti, _te = _aggregate_operands(blk, p, w)
    t_indptr, t_edge = blk.transposed()
    out, gates, cell, hprev = ops.lstm_agg(blk.indptr, blk.src, wq, p, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
                                           blk.num_dst_nodes(), counts, True, t_indptr, t_edge)
    lstm.zero_grad()
    out.backward(gout)
    with torch.no_grad():
        dgate, _dp = ops.lstm_agg_t(blk.indptr, None, None, None if wq is None else wq.detach(), gout, lstm.weight_hh_l0.detach(), gates, cell,
                                    p.shape[0], counts)
    return {"out": out.detach(), "hprev": hprev, "dgate": dgate, "dp": p.grad, "dw": None if w is None else w.grad,
            "dW_hh": lstm.weight_hh_l0.grad.clone(), "db_ih": lstm.bias_ih_l0.grad.clone(), "db_hh": lstm.bias_hh_l0.grad.clone()}


@pytest.mark.parametrize("weighted", [False, True], ids=["copy_u", "u_mul_e"])
@pytest.mark.parametrize("D", [5, 64, 256])
@pytest.mark.parametrize("name", ["mixed", "zero_tile", "last_longest"])
def test_padded_block_with_nan_past_the_live_counts(cuda, name, D, weighted):
    spec, inp, gout, _t, _c = _case(name, D, weighted)
    S, K, B = spec.S, spec.K, spec.B
    lstm = _lstm(cuda, inp, D)
    nan = float("nan")
    p = (inp["h"] @ inp["W_ih"].t()).bfloat16().to(cuda)
    g = gout.bfloat16().to(cuda)
    w = None if inp["w"] is None else inp["w"].bfloat16().to(cuda)
    exact = _op(cuda, bounds.to_block(spec, cuda), p, w, lstm, g)
    blk = bounds.padded_block(spec, cuda)
    Sc, Kc, Bc = blk.num_dst_nodes(), blk.num_src_nodes(), blk.num_edges()
    assert Sc > S and Kc > K and Bc > B
    pp = torch.full((Kc, 4 * D), nan, dtype=torch.bfloat16, device=cuda)
    pp[:K] = p
    gp = torch.full((Sc, D), nan, dtype=torch.bfloat16, device=cuda)
    gp[:S] = g
    wp = None
    if w is not None:
        wp = torch.full((Bc,), nan, dtype=torch.bfloat16, device=cuda)
        wp[:B] = w
    got = _op(cuda, blk, pp, wp, lstm, gp)
    for k, live in (("out", S), ("hprev", B), ("dgate", B), ("dp", K), ("dw", B)):
        if exact[k] is None:
            continue
        assert torch.equal(_bits(got[k][:live]), _bits(exact[k])), k
        assert not _bits(got[k][live:]).any(), k + " is +0 past the live count"
    # d W_hh = dgate^T hprev and d b = the column sums of dgate are library reductions over the edge capacity: the same terms (bit
    # for bit, above) and exact zeros behind them, summed in fp32 in an order that may depend on the length, rounded once -- so
    # within one bf16 step of each other, and never NaN
    for k in ("dW_hh", "db_ih", "db_hh"):
        a, b = got[k].float(), exact[k].float()
        assert bool(torch.isfinite(a).all()) and bool(((a - b).abs() <= 2.0 ** -7 * b.abs().clamp_min(2.0 ** -20)).all()), k
