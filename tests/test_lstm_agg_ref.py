"""CPU checks around the 'lstm' aggregator (csrc/lstm.hip): the float64 restatement of tests/lstm_agg_ref.py
against torch.nn.LSTM run per destination, the layer's and the model's parameter lists and init ranges, the refusals (the pinned
ones still raise, the new ones name their reason), the C entry points' argument checks, and the yardstick check: the model of the
kernel's rounding points (``model_f32``) meets the GPU test's acceptance inequality

    max |x - truth64| <= max |chain_bf16 - truth64|        per tensor, on the same bf16-valued inputs

on every case the GPU test asserts it on, so that a failure there speaks about the kernel alone."""
import ctypes as C

import pytest
import torch

import lstm_agg_ref as ref

T = 32                                  # bliss_lstm_tile_rows(), asserted below


def test_tile_rows_and_case_list():
    from bliss_gnn_amd import _lib
    assert _lib.lib.bliss_lstm_tile_rows() == T and T in (16, 32)
    cases = ref.degree_cases(T)
    assert sorted({len(d) for d in cases.values()}) == [1, T - 1, T, T + 1, 2 * T + 5]
    assert {d for degs in cases.values() for d in degs} == set(ref.DEGREES)
    assert cases["zero_tile"][:T] == [0] * T and sum(cases["no_edges"]) == 0
    last = cases["last_longest"]
    assert len(last) == T and last[-1] == max(last) and last[-1] > max(last[:-1])
    assert max(cases["deg_le_1"]) == 1
    assert [n for n, d in cases.items() if ref.asserted(d)] == ["mixed", "no_zero"]
    spec = ref.make_spec(cases["mixed"], 3)
    r = next(i for i in range(spec.S) if spec.in_degrees()[i] >= 2)
    assert spec.src[spec.indptr[r]] == spec.src[spec.indptr[r] + 1]              # the planted parallel edges
    assert spec.K > spec.S and int(spec.src.max()) >= spec.S                     # sources that are no destinations


@pytest.mark.parametrize("weighted", [False, True])
def test_truth64_is_nn_lstm_run_per_destination(weighted):
    spec, D = ref.hand_block(), 5
    assert spec.in_degrees().tolist() == [0, 3, 2, 1] and 2 not in spec.src.tolist() and 5 in spec.src.tolist()
    inp, gout = ref.make_inputs(spec, D, 7, weighted)
    got = ref.truth64(spec, inp, gout)
    lstm = torch.nn.LSTM(D, D, batch_first=True).double()
    leaves = {k: (None if v is None else v.double().requires_grad_(True)) for k, v in inp.items()}
    with torch.no_grad():
        for name, key in (("weight_ih_l0", "W_ih"), ("weight_hh_l0", "W_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(lstm, name).copy_(leaves[key])
    rows = []
    for d in range(spec.S):
        lo, hi = int(spec.indptr[d]), int(spec.indptr[d + 1])
        if hi == lo:
            rows.append(torch.zeros(D, dtype=torch.float64))
            continue
        x = leaves["h"][spec.src[lo:hi]]
        if weighted:
            x = x * leaves["w"][lo:hi].unsqueeze(1)
        rows.append(lstm(x.unsqueeze(0))[1][0].reshape(D))
    out = torch.stack(rows)
    out.backward(gout.double())
    assert torch.allclose(got["out"], out.detach(), rtol=0, atol=1e-13) and not got["out"][0].any()
    assert torch.allclose(got["dh"], leaves["h"].grad, rtol=0, atol=1e-12)
    for name, p in (("dW_ih", lstm.weight_ih_l0), ("dW_hh", lstm.weight_hh_l0), ("db_ih", lstm.bias_ih_l0), ("db_hh", lstm.bias_hh_l0)):
        assert torch.allclose(got[name], p.grad, rtol=0, atol=1e-12), name
    if weighted:
        assert torch.allclose(got["dw"], leaves["w"].grad, rtol=0, atol=1e-12)
    assert not got["dh"][2].any()                                                # the destination that sends nothing


CASES = [(n, d) for n, d in ref.degree_cases(T).items() if ref.asserted(d)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("D", ref.DIMS)
@pytest.mark.parametrize("name,degs", CASES, ids=[n for n, _ in CASES])
def test_the_rounding_model_meets_the_acceptance_inequality(name, degs, D, weighted):
    spec = ref.make_spec(degs, 3)
    inp, gout = ref.make_inputs(spec, D, ref.input_seed(name, D), weighted)
    truth, chain, model = ref.truth64(spec, inp, gout), ref.chain_bf16(spec, inp, gout), ref.model_f32(spec, inp, gout)
    for k in ref.TENSORS:
        if k in truth:
            assert ref.max_err(model[k], truth[k]) <= ref.max_err(chain[k], truth[k]), (k, ref.max_err(model[k], truth[k]))


def test_degree_at_most_one_leaves_no_recurrent_gradient():
    spec = ref.make_spec(ref.degree_cases(T)["deg_le_1"], 3)
    inp, gout = ref.make_inputs(spec, 8, 108, True)
    for fn in (ref.truth64, ref.chain_bf16, ref.model_f32):
        assert not fn(spec, inp, gout)["dW_hh"].any()


def test_layer_and_model_parameters():
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.model import SAGE, SAGELSTM
    from bliss_gnn_amd.nn import SAGEConv, SAGELSTMConv
    torch.manual_seed(0)
    layer = SAGELSTMConv(8, 4)
    assert isinstance(layer, SAGEConv) and layer._aggre_type == "lstm" and isinstance(layer.lstm, torch.nn.LSTM) and layer.lstm.batch_first
    assert [(n, tuple(q.shape)) for n, q in layer.named_parameters()] == [
        ("lstm.weight_ih_l0", (32, 8)), ("lstm.weight_hh_l0", (32, 8)), ("lstm.bias_ih_l0", (32,)), ("lstm.bias_hh_l0", (32,)),
        ("fc_neigh.weight", (4, 8)), ("fc_self.weight", (4, 8)), ("fc_self.bias", (4,))]
    assert [n for n, _ in SAGELSTMConv(8, 4, bias=False).named_parameters()][-2:] == ["fc_neigh.weight", "fc_self.weight"]
    big = SAGELSTMConv(64, 48)
    k = 1.0 / 64 ** 0.5
    for q in big.lstm.parameters():                                              # nn.LSTM.reset_parameters: uniform +-1/sqrt(D)
        assert 0.9 * k < float(q.detach().abs().max()) <= k
    bound = torch.nn.init.calculate_gain("relu") * (6.0 / (64 + 48)) ** 0.5      # xavier-uniform with the ReLU gain
    for q in (big.fc_neigh.weight, big.fc_self.weight):
        assert 0.9 * bound < float(q.detach().abs().max()) <= bound
    m = SAGELSTM(24, 16, 4, 3, torch.relu, 0.1)
    assert bg.SAGELSTM is SAGELSTM and isinstance(m, SAGE) and m.SAGE_AGGREGATORS == ("lstm",) and m.aggregator_type == "lstm"
    assert all(isinstance(l, SAGELSTMConv) for l in m.layers) and [l._in_src_feats for l in m.layers] == [24, 16, 16]
    names = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc_neigh.weight", "fc_self.weight", "fc_self.bias")
    assert [n for n, _ in m.named_parameters()] == ["layers.%d.%s" % (l, n) for l in range(3) for n in names]
    assert SAGE.SAGE_AGGREGATORS == ("mean", "pool", "gcn")


def test_refusals():
    from bliss_gnn_amd import explain
    from bliss_gnn_amd.model import SAGE, SAGELSTM
    from bliss_gnn_amd.nn import SAGEConv, SAGELSTMConv, lstm_aggregate, lstm_refusal
    from bliss_gnn_amd.shard import ShardedTrainStep
    from bliss_gnn_amd.shard_static import StaticShardedTrainStep
    for pattern in ("pool", "'mean'.*'pool'.*'gcn'", "'lstm'", "SAGEGCNConv", "SAGELSTMConv"):     # the pinned ones, and the new name
        with pytest.raises(NotImplementedError, match=pattern):
            SAGEConv(8, 4, "lstm")
    with pytest.raises(NotImplementedError, match="SAGELSTM"):
        SAGE(24, 16, 4, 3, torch.relu, 0.1, aggregator_type="lstm")
    with pytest.raises(NotImplementedError, match="256.*257"):
        SAGELSTMConv(257, 4)
    with pytest.raises(NotImplementedError, match="256"):
        SAGELSTM(300, 16, 4, 2, torch.relu, 0.0)
    SAGELSTMConv(256, 4)
    layer = SAGELSTMConv(8, 4)                                                   # fp32 on the CPU: refused by name, nothing launched
    assert "bf16" in lstm_refusal(layer.lstm) and "float32" in lstm_refusal(layer.lstm)
    with pytest.raises(NotImplementedError, match="bf16 features and LSTM parameters on the GPU"):
        lstm_aggregate(None, torch.zeros(3, 8), layer.lstm)
    with pytest.raises(NotImplementedError, match="nn.LSTM"):
        lstm_aggregate(None, torch.zeros(3, 8), torch.nn.LSTM(8, 4))
    m = SAGELSTM(24, 16, 4, 2, torch.relu, 0.1)
    why = m.csc_refusal(None, torch.zeros(1))
    assert why is not None and '"lstm"' in why
    with pytest.raises(NotImplementedError, match='"lstm".*sharded'):
        ShardedTrainStep(None, None, m)
    with pytest.raises(NotImplementedError, match='"lstm".*sharded'):
        StaticShardedTrainStep(None, None, m, 8)
    assert explain.refusal(m) is None


def test_abi_refusals():
    from bliss_gnn_amd import _lib
    L, E, P = _lib.lib, _lib.EINVAL, 4096
    fwd = dict(indptr=P, src=P, w=0, p=P, p_stride=32, w_hh=P, w_hh_stride=8, b_ih=0, b_hh=0, n_dst=4, n_dst_dev=0, nnz_dev=0, nnz=8, dim=8,
               out=P, out_stride=8, gates=0, cell=0, hprev=0, stream=0)
    bad = [dict(indptr=0), dict(src=0), dict(p=0), dict(w_hh=0), dict(out=0), dict(n_dst=-1), dict(nnz=-1), dict(dim=0), dict(dim=-2),
           dict(dim=257, p_stride=2048, w_hh_stride=512, out_stride=512), dict(p_stride=31), dict(w_hh_stride=7), dict(out_stride=7),
           dict(gates=P), dict(gates=P, cell=P), dict(hprev=P)]
    for change in bad:
        assert L.bliss_lstm_agg_fwd(*{**fwd, **change}.values()) == E, change
    assert L.bliss_lstm_agg_fwd(*{**fwd, "n_dst": 0, "nnz": 0, "src": 0, "p": 0}.values()) == 0          # no rows: nothing to launch
    bwd = dict(indptr=P, gout=P, gout_stride=8, w_hh_t=P, w_hh_t_stride=32, gates=P, cell=P, n_dst=4, n_dst_dev=0, nnz_dev=0, nnz=8, dim=8,
               dgate=P, stream=0)
    bad = [dict(indptr=0), dict(gout=0), dict(w_hh_t=0), dict(gates=0), dict(cell=0), dict(dgate=0), dict(n_dst=-1), dict(nnz=-1),
           dict(dim=0), dict(dim=257, gout_stride=512, w_hh_t_stride=2048), dict(gout_stride=7), dict(w_hh_t_stride=31)]
    for change in bad:
        assert L.bliss_lstm_agg_bwd(*{**bwd, **change}.values()) == E, change
    assert L.bliss_lstm_agg_bwd(*{**bwd, "nnz": 0, "gates": 0, "cell": 0, "dgate": 0}.values()) == 0     # no edge: nothing to write
    red = dict(t_indptr=P, t_edge=P, w=0, dgate=P, n_src=6, nnz_dev=0, nnz=8, dim=8, dp=P, dp_stride=32, stream=0)
    bad = [dict(t_indptr=0), dict(t_edge=0), dict(dgate=0), dict(dp=0), dict(n_src=-1), dict(nnz=-1), dict(dim=0), dict(dim=257, dp_stride=2048),
           dict(dp_stride=31)]
    for change in bad:
        assert L.bliss_lstm_edge_reduce(*{**red, **change}.values()) == E, change
    assert L.bliss_lstm_edge_reduce(*{**red, "n_src": 0, "nnz": 0}.values()) == 0
    names = [L.bliss_prof_kernel_name(i).decode() for i in range(L.bliss_prof_kernel_count())]
    assert all(names.count(n) == 1 for n in ("k_lstm_agg_fwd", "k_lstm_agg_bwd", "k_lstm_edge_reduce"))
    assert names[-3:] == ["k_sddmm_dot", "k_spmm_max_bwd_relu", "k_spmm_max_bwd_relu_fixup"] and names.index("k_spmm_max_bwd") == 26
    assert isinstance(C.c_int(_lib.LSTM_MAX_DIM).value, int) and _lib.LSTM_MAX_DIM == 256
