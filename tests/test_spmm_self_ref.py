"""CPU: the restatement of SAGEConv 'gcn' message passing (tests/spmm_self_ref.py) against a plain Python loop, the C ABI's
refusals, the layer's parameter list, and the two conditions the GPU tests lean on: the integer layer cases are exact at every
rounding point, and every block of the GPU tests stays within the row length bounds.SPMM_K is derived for."""
import numpy as np
import pytest
import torch

import bounds
import spmm_self_ref as ref


def _hand_block():
    """5 sources, 3 destinations: destination 0 has no in-edge, destination 1 has parallel edges from source 3 (no destination) and
    one from source 0, destination 2 has one edge from source 1 and sends nothing itself; source 4 sends nothing."""
    indptr = torch.tensor([0, 0, 3, 4])
    src = torch.tensor([3, 0, 3, 1])
    dst = torch.tensor([1, 1, 1, 2])
    gen = torch.Generator().manual_seed(1)
    h = torch.randn(5, 3, generator=gen).bfloat16()
    w = (torch.rand(4, generator=gen) + 0.25).bfloat16()
    g = torch.randn(3, 3, generator=gen).bfloat16()
    return indptr, src, dst, h, w, g


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("pair", [False, True])
def test_restatement_equals_a_plain_loop(weighted, pair):
    indptr, src, dst, h, w, g = _hand_block()
    w = w if weighted else None
    S, K, D = 3, 5, 3
    hs = torch.randn(S, D, generator=torch.Generator().manual_seed(2)).bfloat16() if pair else None
    f32, f64 = np.float32, np.float64
    wv = [f32(1.0)] * 4 if w is None else [f32(float(x)) for x in w]
    out32, out64, mag64 = np.zeros((S, D), f32), np.zeros((S, D), f64), np.zeros((S, D), f64)
    selfrow = (h[:S] if hs is None else hs).float().numpy()
    for i in range(S):
        for c in range(D):
            a32, a64, m64 = f32(0), 0.0, 0.0
            for e in range(int(indptr[i]), int(indptr[i + 1])):
                x = f32(float(h[int(src[e]), c]))
                a32 = f32(a32 + f32(wv[e] * x))
                a64 += f64(wv[e]) * f64(x)
                m64 += abs(f64(wv[e]) * f64(x))
            d = int(indptr[i + 1] - indptr[i])
            out32[i, c] = f32(f32(a32 + selfrow[i, c]) * f32(f32(1.0) / f32(d + 1)))
            out64[i, c] = (a64 + f64(selfrow[i, c])) / (d + 1)
            mag64[i, c] = (m64 + abs(f64(selfrow[i, c]))) / (d + 1)
    got = ref.forward_f32(indptr, src, dst, h, w, hs)
    assert torch.equal(got, torch.from_numpy(out32).bfloat16())
    assert torch.equal(got[0], (h[:S] if hs is None else hs)[0])                  # the degree-0 row: its self row, bit for bit
    v, m = ref.terms(indptr, src, dst, h, w, hs)
    assert np.allclose(v.numpy(), out64, rtol=1e-14, atol=0) and np.allclose(m.numpy(), mag64, rtol=1e-14, atol=0)

    deg = (indptr[1:] - indptr[:-1]).tolist()
    gz32, gz64, gm64 = np.zeros((K, D), f32), np.zeros((K, D), f64), np.zeros((K, D), f64)
    for j in range(K):
        for c in range(D):
            a32, a64, m64 = f32(0), 0.0, 0.0
            for e in range(4):                                                   # ascending edge order = the by-source order
                if int(src[e]) == j:
                    i = int(dst[e])
                    x = f32(float(g[i, c]))
                    a32 = f32(a32 + f32(f32(wv[e] / f32(deg[i] + 1)) * x))
                    a64 += f64(wv[e]) / (deg[i] + 1) * f64(x)
                    m64 += abs(f64(wv[e]) / (deg[i] + 1) * f64(x))
            if j < S:
                x = f32(float(g[j, c]))
                a32 = f32(a32 + f32(f32(f32(1.0) / f32(deg[j] + 1)) * x))
                a64 += f64(x) / (deg[j] + 1)
                m64 += abs(f64(x)) / (deg[j] + 1)
            gz32[j, c], gz64[j, c], gm64[j, c] = a32, a64, m64
    assert torch.equal(ref.backward_f32(indptr, src, dst, g, K, w), torch.from_numpy(gz32).bfloat16())
    v, m = ref.terms_bwd(indptr, src, dst, g, K, w)
    assert np.allclose(v.numpy(), gz64, rtol=1e-14, atol=0) and np.allclose(m.numpy(), gm64, rtol=1e-14, atol=0)
    assert not bool(v[4].any()) and bool(v[2].any())             # a source that sends nothing; a destination's self term alone
    v0, _ = ref.terms_bwd(indptr, src, dst, g, K, w, fold_self=False)
    assert not bool(v0[2].any()) and torch.equal(v0[3], v[3])


def test_ordered_sum_follows_the_chunks():
    """A row cut by 16-edge chunks: the restatement adds chunk partials, not one running sum (values chosen so the two differ)."""
    B = 40
    indptr = torch.tensor([0, 3, B])
    dst = torch.tensor([0] * 3 + [1] * (B - 3))
    src = torch.arange(B) % 7 + 2
    h = torch.zeros(9, 1)
    h[2:, 0] = torch.tensor([2.0 ** 24, 1.0, 1.0, 1.0, -2.0 ** 24, 1.0, 3.0])
    h = h.bfloat16()
    got = ref._ordered_sum(dst, src, torch.ones(B), h, 2, 16)
    hv = h.float()[:, 0].numpy()
    want = []
    for r, (b, e) in enumerate([(0, 3), (3, B)]):
        parts, k = [], b
        while k < e:
            stop = min(e, (k // 16 + 1) * 16)
            a = np.float32(0)
            for q in range(k, stop):
                a = np.float32(a + hv[int(src[q])])
            parts.append(a)
            k = stop
        t = parts[0]
        for a in parts[1:]:
            t = np.float32(t + a)
        want.append(t)
    assert got[:, 0].tolist() == [float(x) for x in want]


def test_abi_refusals():
    from bliss_gnn_amd import _lib
    L, E = _lib.lib, _lib.EINVAL
    assert hasattr(L, "bliss_spmm_self_fwd") and hasattr(L, "bliss_spmm_self_bwd")
    assert len(_lib.SIGNATURES["bliss_spmm_self_fwd"]) == 17 and len(_lib.SIGNATURES["bliss_spmm_self_bwd"]) == 18
    P = 4096                                                                     # a non-NULL pointer no refused call reads
    fwd = dict(indptr=P, src=P, dst=P, w=0, h=P, h_stride=8, h_self=P, h_self_stride=8, n_dst=4, n_dst_dev=0, nnz_dev=0, nnz=8, dim=8,
               out=P, out_stride=8, partials=0, stream=0)
    bad_fwd = [dict(indptr=0), dict(h=0), dict(h_self=0), dict(out=0), dict(src=0), dict(dst=0), dict(n_dst=-1), dict(nnz=-1), dict(dim=0),
               dict(dim=-3), dict(h_stride=7), dict(h_self_stride=7), dict(out_stride=7), dict(nnz=17)]       # 17 edges: two chunks, no partials
    for change in bad_fwd:
        assert L.bliss_spmm_self_fwd(*{**fwd, **change}.values()) == E, change
    bwd = dict(t_indptr=P, t_edge=P, src=P, dst=P, indptr=P, w=0, gout=P, gout_stride=8, n_src=6, n_dst=4, n_dst_dev=0, nnz_dev=0, nnz=8,
               dim=8, gh=P, gh_stride=8, partials=0, stream=0)
    bad_bwd = [dict(t_indptr=0), dict(indptr=0), dict(gout=0), dict(gh=0), dict(t_edge=0), dict(src=0), dict(dst=0), dict(n_src=-1),
               dict(n_dst=-1), dict(nnz=-1), dict(dim=0), dict(gout_stride=7), dict(gh_stride=7), dict(nnz=17), dict(n_dst=7)]
    for change in bad_bwd:
        assert L.bliss_spmm_self_bwd(*{**bwd, **change}.values()) == E, change
    # no rows: nothing to launch, once the arguments are sound (the edge arrays do not count without edges)
    assert L.bliss_spmm_self_fwd(*{**fwd, "n_dst": 0, "nnz": 0, "src": 0, "dst": 0}.values()) == 0
    assert L.bliss_spmm_self_bwd(*{**bwd, "n_src": 0, "n_dst": 0, "nnz": 0, "t_edge": 0, "src": 0, "dst": 0}.values()) == 0
    names = [L.bliss_prof_kernel_name(i).decode() for i in range(L.bliss_prof_kernel_count())]
    assert all(n in names for n in ("k_spmm_self", "k_spmm_self_fixup", "k_spmm_self_bwd", "k_spmm_self_bwd_fixup"))


def test_sageconv_gcn_surface():
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.nn import SAGEConv, SAGEGCNConv
    layer = SAGEGCNConv(8, 4)
    assert isinstance(layer, SAGEConv) and layer._aggre_type == "gcn"
    with pytest.raises(NotImplementedError, match="SAGEGCNConv"):                # the constructor of SAGEConv itself keeps refusing
        SAGEConv(8, 4, "gcn")
    assert {n: tuple(q.shape) for n, q in layer.named_parameters()} == {"fc_neigh.weight": (4, 8), "bias": (4,)}
    assert not hasattr(layer, "fc_self") and not bool(layer.bias.any())
    assert [n for n, _ in SAGEGCNConv(8, 4, bias=False).named_parameters()] == ["fc_neigh.weight"]
    bound = torch.nn.init.calculate_gain("relu") * (6.0 / 12) ** 0.5               # xavier-uniform with the ReLU gain
    wmax = float(layer.fc_neigh.weight.detach().abs().max())
    assert 0.5 * bound < wmax <= bound
    with pytest.raises(NotImplementedError, match="'mean'.*'pool'.*'gcn'"):
        SAGEConv(8, 4, "lstm")
    m = SAGE(24, 16, 4, 3, torch.relu, 0.1, aggregator_type="gcn")
    assert sorted(n for n, _ in m.named_parameters()) == sorted("layers.%d.%s" % (l, n) for l in range(3) for n in ("bias", "fc_neigh.weight"))
    assert not m._mfma_ok(torch.zeros(1)) and not m._gcn_tile
    assert SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="tile", aggregator_type="gcn")._gcn_tile
    with pytest.raises(NotImplementedError, match="gcn"):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, transforms="wide", aggregator_type="gcn")
    with pytest.raises(NotImplementedError):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, aggregator_type="lstm")
    why = m.csc_refusal(None, torch.zeros(1))
    assert why is not None and '"gcn"' in why


def test_sharded_steps_refuse_gcn_by_name():
    from bliss_gnn_amd.model import SAGE
    from bliss_gnn_amd.shard import ShardedTrainStep
    from bliss_gnn_amd.shard_static import StaticShardedTrainStep
    m = SAGE(24, 16, 4, 2, torch.relu, 0.1, aggregator_type="gcn")
    with pytest.raises(NotImplementedError, match='"gcn".*sharded'):
        ShardedTrainStep(None, None, m)
    with pytest.raises(NotImplementedError, match='"gcn".*sharded'):
        StaticShardedTrainStep(None, None, m, 8)


@pytest.mark.parametrize("fin,fout", [(8, 4), (4, 8)])
def test_the_integer_layer_is_exact_at_every_rounding_point(fin, fout):
    """The GPU test on integers compares with == against fp64: that says something only if the restatement that rounds to bf16 at
    every store equals the fp64 one on these inputs."""
    c = ref.exact_case(fin, fout)
    kw = dict(bias=c["bias"], ew=c["ew"], g=c["g"], relu=True)
    a = ref.layer_terms(c["indptr"], c["src"], c["dst"], c["h"], c["w_neigh"], sim=True, **kw)
    b = ref.layer_terms(c["indptr"], c["src"], c["dst"], c["h"], c["w_neigh"], sim=False, **kw)
    for name in ("rst", "out", "d_w", "d_b", "d_h"):
        assert torch.equal(a[name], b[name]), name
        assert bool(b[name].any()), name
    assert (fin > fout) == (c["w_neigh"].shape[1] > c["w_neigh"].shape[0])
    deg = c["indptr"][1:] - c["indptr"][:-1]
    assert sorted(set(deg.tolist())) == [0, 1, 3, 7, 15, 31]
    assert bool((b["out"] > 0).any()) and bool((b["rst"] < 0).any())              # the ReLU's mask cuts something and passes something


def test_gpu_blocks_stay_within_the_row_limit():
    """bounds.SPMM_K is derived for an fp32 sum of at most 16 384 terms; a row here has deg + 1 terms and two more fp32 roundings
    (the reciprocal and the product), so it holds for rows of up to 16 381 edges, by destination and by source."""
    limit = bounds.SPMM_MAX_ROW - 3
    specs = [bounds.edge_shape_spec(), bounds.spmm_band_spec(60000, 21), bounds.spmm_band_spec(210000, 22)]
    for spec in specs:
        assert int(spec.in_degrees().max()) <= limit and int(spec.out_degrees().max()) <= limit
    assert ref.chunk_edges(specs[0].B) == 16 and ref.chunk_edges(specs[1].B) == 32 and ref.chunk_edges(specs[2].B) == 64
    assert 50000 <= specs[1].B < 200000 <= specs[2].B
    from bliss_gnn_amd import _lib
    assert all(_lib.lib.bliss_spmm_chunk_edges(n) == ref.chunk_edges(n) for n in (0, 1, 49999, 50000, 199999, 200000))
