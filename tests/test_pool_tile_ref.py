"""CPU suite for SAGEConv('pool') on the tile kernels: the masked max backward's restatement
(tests/pool_tile_ref.py) against a plain loop on the hand block of tests/test_spmm_max_ref.py, the argument refusals of
bliss_spmm_max_bwd_relu (no launch is made), and the Python surface of ``transforms="tile"`` that needs no GPU."""
import ctypes as C

import pytest
import torch

import pool_tile_ref as ptr
import spmm_max_ref as ref
from test_spmm_max_ref import _hand_block


def _hand_act(K):
    """act [K, 3] over the hand block's 9 sources: +0.0, -0.0, a small positive normal value (2^-100), negatives and ordinary
    positives; source 3, which wins row 4's column 0, holds the small value there."""
    act = torch.tensor([[1.0, 0.0, 2.0], [-0.0, 3.0, 2.0 ** -100], [0.5, -2.0, -0.0], [2.0 ** -100, 0.0, 1.0], [0.0, 4.0, 0.5],
                        [7.0, -0.0, 1.0], [-1.5, 0.75, 0.0], [0.125, -9.0, 1.0], [-0.0, 5.0, -5.0]]).bfloat16()
    assert act.shape == (K, 3) and float(act[1, 2]) == 2.0 ** -100
    return act


@pytest.mark.parametrize("weighted", [True, False])
def test_masked_restatement_equals_the_plain_loop(weighted):
    h, src, dst, indptr, w = _hand_block()
    w = w if weighted else None
    S, K = 6, h.shape[0]
    _, _, arg = ref.forward(src, dst, S, h, w)
    gout = (torch.arange(S * 3, dtype=torch.float32).reshape(S, 3) - 4.0).bfloat16()
    act = _hand_act(K)
    gz, mag = ptr.masked_backward(src, K, gout, arg, act, w)
    want = torch.zeros(K, 3, dtype=torch.float64)
    for i in range(S):
        for c in range(3):
            e = int(arg[i, c])
            if e >= 0 and float(act[int(src[e]), c]) > 0:
                want[int(src[e]), c] += (float(w[e]) if weighted else 1.0) * float(gout[i, c])
    assert torch.equal(gz, want) and bool((mag >= gz.abs()).all())
    plain, _ = ref.backward(src, K, gout, arg, w)
    masked = ~(act.double() > 0)
    assert bool((plain[masked] != 0).any()) and bool((gz != plain).any()), "the mask must change something on this block"
    # both zeros mask, and a masked element is +0 (no sign bit), whatever the sign of the sum it replaces
    zeros = act.float() == 0
    assert int(zeros.sum()) >= 6 and bool((gz[zeros] == 0).all())
    assert not bool(torch.signbit(gz[masked]).any())
    assert bool(torch.signbit(act[zeros].float()).any()) and not bool(torch.signbit(act[zeros].float()).all())
    assert float(act[3, 0]) == 2.0 ** -100 and gz[3, 0] == plain[3, 0] and plain[3, 0] != 0     # a small positive value passes


def test_layer_restatement_backward_is_autograd_of_its_forward():
    """The written-out backward of pool_tile_ref.layer (sim=False) against float64 autograd through the same forward with the
    recorded arg (the max is differentiated as the gather it ends as)."""
    h, src, dst, indptr, w = _hand_block()
    S, K, fin, fout = 6, h.shape[0], 3, 2
    gen = torch.Generator().manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    Wp, bp, Wn, Ws, bs, gout = mk(fin, fin), mk(fin), mk(fout, fin), mk(fout, fin), mk(fout), mk(S, fout)
    keep = torch.rand(S, fout, generator=gen) < 0.7
    pts = ptr.layer(src, dst, S, h, w, Wp, bp, Wn, Ws, bs, relu=True, p=0.25, keep=keep, gout=gout, sim=False)
    leaves = [t.clone().requires_grad_(True) for t in (h.double(), Wp, bp, Wn, Ws, bs)]
    H, WP, BP, WN, WS, BS = leaves
    pooled = (H @ WP.t() + BP).clamp(min=0)
    arg = pts["arg"].long()
    msg = w.double()[arg.clamp(min=0)] * pooled[src[arg.clamp(min=0)], torch.arange(fin).expand(S, fin)]
    neigh = torch.where(arg >= 0, msg, torch.zeros((), dtype=torch.float64))
    neigh = neigh + (pts["neigh"] - neigh).detach()             # the message's rounding, differentiated as the identity
    out = (neigh @ WN.t() + H[:S] @ WS.t() + BS).clamp(min=0) * keep.double() / 0.75
    assert torch.allclose(out, pts["out"], rtol=1e-12, atol=0)
    out.backward(gout)
    for got, name in zip(leaves, ("d_feat", "fc_pool.weight", "fc_pool.bias", "fc_neigh.weight", "fc_self.weight", "fc_self.bias")):
        assert torch.allclose(got.grad, pts[name], rtol=1e-9, atol=1e-12), name


def test_relu_entry_point_refuses_bad_arguments_before_any_launch():
    """Every BLISS_EINVAL case of bliss_spmm_max_bwd, plus act == NULL and act_stride < dim -- validated on the host."""
    from bliss_gnn_amd import _lib
    lib, E = _lib.lib, _lib.EINVAL
    assert "bliss_spmm_max_bwd_relu" in _lib.SIGNATURES and hasattr(lib, "bliss_spmm_max_bwd_relu")
    assert len(_lib.SIGNATURES["bliss_spmm_max_bwd_relu"]) == len(_lib.SIGNATURES["bliss_spmm_max_bwd"]) + 2
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    bwd = lambda ti=p, te=p, src=p, dst=p, w=p, g=p, gs=8, arg=p, as_=8, act=p, acs=8, n=4, nd=0, nnz=8, dim=8, gh=p, hs=8, part=p: \
        lib.bliss_spmm_max_bwd_relu(ti, te, src, dst, w, g, gs, arg, as_, act, acs, n, nd, nnz, dim, gh, hs, part, 0)
    assert bwd(ti=0) == E and bwd(te=0) == E and bwd(src=0) == E and bwd(dst=0) == E and bwd(g=0) == E and bwd(arg=0) == E and bwd(gh=0) == E
    assert bwd(n=-1) == E and bwd(nnz=-1) == E and bwd(dim=0) == E and bwd(dim=-4) == E
    assert bwd(gs=7) == E and bwd(as_=7) == E and bwd(hs=7) == E
    assert lib.bliss_spmm_chunk_edges(17) == 16 and bwd(nnz=17, part=0) == E
    assert bwd(act=0) == E and bwd(acs=7) == E
    assert bwd(act=0, n=0) == E                                 # (before the empty-block return as well)
    names = [lib.bliss_prof_kernel_name(i).decode() for i in range(lib.bliss_prof_kernel_count())]
    assert names[-2:] == ["k_spmm_max_bwd_relu", "k_spmm_max_bwd_relu_fixup"] and names.index("k_spmm_max_bwd") == 26


def test_sage_tile_spelling_constructs_on_the_cpu():
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.train import _live_refusal
    assert SAGE.SAGE_TRANSFORMS == ("auto", "wide", "tile")
    pool = SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="tile", aggregator_type="pool")
    mean = SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="tile", aggregator_type="mean")
    assert pool._pool_tile and not mean._pool_tile and len(list(pool.parameters())) == 15 and len(list(mean.parameters())) == 9
    with pytest.raises(ValueError, match="transforms"):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="tiles", aggregator_type="pool")
    with pytest.raises(NotImplementedError, match="pool"):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="wide", aggregator_type="pool")
    # a CPU fp32 model: the first forward refuses, naming what the path takes; nothing falls back to the library path
    for m in (pool, mean):
        with pytest.raises(NotImplementedError, match="bf16.*GPU"):
            m([None, None, None], torch.zeros(5, 24))
        why = _live_refusal(m)
        assert why is not None
    assert "bf16" in _live_refusal(pool) and "GPU" in _live_refusal(pool)
    assert "MFMA path" in _live_refusal(SAGE(24, 16, 4, 3, torch.relu, 0.1, aggregator_type="pool"))


def test_tile_refusal_names_the_reason():
    """The refusals that do not depend on where the tensors live are ordered behind the bf16 / GPU check, so they are read here
    through a stand-in for a bf16 GPU tensor."""
    import torch.nn as nn
    from bliss_gnn_amd.model import SAGE

    class _Gpu:
        is_cuda, dtype, device = True, torch.bfloat16, "cuda:0"

    def why(model):
        model.parameters = lambda: iter(())          # (no parameter is looked at: the stand-in plays the features)
        return model.tile_refusal(_Gpu())

    mk = lambda *a, **kw: SAGE(*a, transforms="tile", aggregator_type="pool", **kw)
    assert why(mk(24, 16, 4, 3, torch.relu, 0.1)) is None
    assert why(mk(24, 16, 4, 3, nn.ReLU(), 0.1)) is None
    assert "ReLU" in why(mk(24, 16, 4, 3, torch.tanh, 0.1))
    m = mk(24, 16, 4, 3, torch.relu, 0.1)
    m.dropout = nn.Identity()
    assert "nn.Dropout" in why(m)
    m = mk(24, 16, 4, 3, torch.relu, 0.1)
    m.layers[1].feat_drop = nn.Dropout(0.5)
    assert "layer 1" in why(m)
    m = mk(24, 16, 4, 3, torch.relu, 0.1)
    m.layers[2].fc_self = nn.Linear(16, 4, bias=False)
    assert "layer 2" in why(m) and "bias" in why(m)
    assert "layer 0" in why(mk(1433, 16, 4, 3, torch.relu, 0.1)) and "1024" in why(mk(1433, 16, 4, 3, torch.relu, 0.1))
    assert "layer 0" in why(mk(24, 257, 4, 3, torch.relu, 0.1)) and "out_feats <= 256" in why(mk(24, 257, 4, 3, torch.relu, 0.1))
    assert "layer 2" in why(mk(24, 16, 300, 3, torch.relu, 0.1)) and "16 -> 300" in why(mk(24, 16, 300, 3, torch.relu, 0.1))


@pytest.mark.parametrize("env", ["BLISS_SAGE_MFMA", "BLISS_SAGE_MFMA_BWD"])
def test_tile_refusal_under_the_library_switches(env, monkeypatch):
    from bliss_gnn_amd.model import SAGE
    monkeypatch.setenv(env, "0")
    m = SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="tile", aggregator_type="pool")
    assert env + "=0" in m.tile_refusal(torch.zeros(1))


def test_tail_entry_point_follows_the_size_formula():
    """nn._tile_gemm_fits is csrc/sage.hip's LDS formula: 32 rows of each operand at stride round16(k) + 8 and a 256 x 72 slab of
    W in bf16 against 160 KiB.  One operand always fits at k <= 1024; two fit up to 976 + 976."""
    from bliss_gnn_amd.nn import _tile_gemm_fits
    lds = lambda k1, k2: 2 * (32 * ((((k1 + 15) & ~15) + 8) + ((((k2 + 15) & ~15) + 8) if k2 else 0)) + 256 * 72)
    for k1, k2 in [(1024, 0), (602, 602), (976, 976), (977, 977), (1024, 1024), (1024, 256), (16, 16)]:
        assert _tile_gemm_fits(k1, k2) == (lds(k1, k2) <= 160 * 1024), (k1, k2)
    assert _tile_gemm_fits(1024) and _tile_gemm_fits(602, 602) and _tile_gemm_fits(976, 976) and not _tile_gemm_fits(977, 977)
