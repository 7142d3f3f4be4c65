"""GPU suite (-m gpu): ``sample_blocks_static(..., n_live_dev=word)``.  For every sampler family the engine
routes -- the layer-wise Poisson / LADIES chain, the multinomial device draw, neighbor, weighted neighbor, LABOR-0, LABOR-i and
weighted LABOR -- a seed buffer of 64 slots with n live seeds gives, over the live prefix, exactly the blocks of the same call
with a buffer of n seeds: same seeds, draw step and generator state; generator and draw step end up equal; the engine's scratch
is idle again.  Slots past the live count keep earlier batches' ids (or the initial zeros) and change nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, E, CAP, FAN, DRAW_SEED = 600, 7000, 64, [12, 8, 6], 31
FAMILIES = ["poisson-bandit", "poisson-ladies", "bandit-device", "ladies-device", "neighbor", "neighbor-prob", "neighbor-exp3",
            "labor", "labor-2", "labor-prob", "labor-exp3"]


def _graph(cuda):
    import bliss_gnn_amd as bg
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(V, E, seed=3)
    gen = torch.Generator().manual_seed(2)
    g = bg.Graph(ip.to(cuda), ix.to(cuda), ei.to(cuda), ndata={"features": torch.randn(V, 16, generator=gen).bfloat16().to(cuda)})
    g.edata["w"] = bg.normalized_edata(g)
    g.edata["prob"] = torch.exp2(torch.randint(-4, 3, (g.num_edges(),), generator=gen).float()).to(cuda)
    return g


def _sampler(name):
    from bliss_gnn_amd import fit
    if name == "neighbor-prob":
        s = fit.NeighborSampler(FAN, draw="device", prob="prob")
    elif name == "labor-prob":
        s = fit.WeightedLaborSampler(FAN, prob="prob")
    elif name.endswith("-device"):
        s = fit.make_sampler(name[:-len("-device")], FAN, draw="device")
    else:
        s = fit.make_sampler(name, FAN, draw="device")
    return s


def _device_draw(s):
    return getattr(s, "draw", "host") == "device"


def _static_call(s, g, seeds, step, **kw):
    """One enqueue + finish from a fixed state: draw step ``step`` / torch's generator seeded with 11."""
    if _device_draw(s):
        s.reset_draw(seed=DRAW_SEED, step=step)
    torch.manual_seed(11)
    s._engine.stage_rng_from_torch()
    _, _, blocks = s.sample_blocks_static(g, seeds, **kw)
    torch.cuda.synchronize()
    cnts = s.finish_static()
    return blocks, list(reversed(cnts)), torch.get_rng_state(), (s.draw_step() if _device_draw(s) else None)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _assert_scratch_idle(eng):
    """The checks of the samplers' own edge tests: tickets and node bitmap of whichever node-wise scratch exists, kept_map."""
    words = -(-(-(-eng.V // 32)) // 1024) * 1024
    for scr in (eng._nb_scr, eng._wn_scr, eng._lb_scr and eng._lb_scr[1], eng._li_scr and eng._li_scr[2], eng._wl_scr and eng._wl_scr[2]):
        if scr is not None:
            assert int(scr[:16 + words].abs().sum()) == 0
    for st in eng._sets.values():
        assert bool((st["kept_map"] == -1).all())
    assert int(eng.fs_ticket.item()) == 0


@pytest.mark.parametrize("name", FAMILIES)
def test_live_prefix_is_the_exact_size_call(cuda, name):
    import bliss_gnn_amd as bg
    g = _graph(cuda)
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(4)).to(torch.int32).to(cuda)
    A = _sampler(name)
    A.sample_blocks(g, perm[:CAP])                                              # binds the engine: capacities of CAP seeds
    assert A._engine.caps[0]["S"] == CAP
    buf = torch.zeros(CAP, dtype=torch.int32, device=cuda)                      # starts zeroed
    word = torch.zeros(1, dtype=torch.int32, device=cuda)
    off = 0
    for i, n in enumerate((37, 64, 1, 63)):
        batch = perm[off:off + n].clone()
        off += 70
        buf[:n] = batch                                                         # slots >= n: zeros, then the previous batches' ids
        word.fill_(n)
        got, c_got, rng_got, step_got = _static_call(A, g, buf, 5 + i, n_live_dev=word)
        B = _sampler(name)
        B.sample_blocks(g, batch)
        assert B._engine.caps[0]["S"] == n
        want, c_want, rng_want, step_want = _static_call(B, g, batch, 5 + i)
        assert torch.equal(rng_got, rng_want) and step_got == step_want, (name, n)
        for l, (bg_, bw, cg, cw) in enumerate(zip(got, want, c_got, c_want)):
            what = (name, n, l)
            assert (cg.S, cg.E, cg.C, cg.K, cg.B, cg.err) == (cw.S, cw.E, cw.C, cw.K, cw.B, 0), what
            S, K, B_ = cw.S, cw.K, cw.B
            assert torch.equal(bg_.indptr[:S + 1], bw.indptr[:S + 1]), what
            for f in ("src", "dst", "pos"):
                assert torch.equal(getattr(bg_, f)[:B_], getattr(bw, f)[:B_]), what + (f,)
            assert torch.equal(bg_.edata[bg.EID][:B_], bw.edata[bg.EID][:B_]), what
            assert torch.equal(bg_.srcdata[bg.NID][:K], bw.srcdata[bg.NID][:K]), what
            assert torch.equal(_bits(bg_._edge_weights[:B_]), _bits(bw._edge_weights[:B_])), what
            assert torch.equal(_bits(bg_._q[:B_]), _bits(bw._q[:B_])), what
            assert torch.equal(_bits(bg_._node_prob[:K]), _bits(bw._node_prob[:K])), what
            assert hasattr(bg_, "_p") == hasattr(bw, "_p")
            if hasattr(bw, "_p"):
                assert torch.equal(_bits(bg_._p[:B_]), _bits(bw._p[:B_])), what
            if getattr(bw, "_transposed", None) is not None and getattr(bg_, "_transposed", None) is not None:
                assert torch.equal(bg_._transposed[0][:K + 1], bw._transposed[0][:K + 1]), what
                assert torch.equal(bg_._transposed[1][:B_], bw._transposed[1][:B_]), what
        assert c_got[-1].S == n                                                 # the output block's counts record holds the live S
        assert int(got[-1]._counts_dev[0]) == n
        _assert_scratch_idle(A._engine)
        _assert_scratch_idle(B._engine)


@pytest.mark.parametrize("name", ["poisson-bandit", "labor", "neighbor"])
def test_bad_words_and_split_enqueues_are_refused_on_the_host(cuda, name):
    g = _graph(cuda)
    s = _sampler(name)
    seeds = torch.arange(CAP, dtype=torch.int32, device=cuda)
    s.sample_blocks(g, seeds)
    word = torch.full((1,), 5, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):                                             # a buffer that is not the static seed capacity
        s.sample_blocks_static(g, seeds[:40].contiguous(), n_live_dev=word)
    with pytest.raises(ValueError):
        s.sample_blocks_static(g, seeds, n_live_dev=word.long())
    with pytest.raises(ValueError):
        s.sample_blocks_static(g, seeds, n_live_dev=word.cpu())
    with pytest.raises(NotImplementedError):                                    # the pipelined loop's enqueues have no live count
        s.sample_blocks_static(g, seeds, chain_rng=True, n_live_dev=word)
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, seeds, part="main", external_rng=True, n_live_dev=word)
