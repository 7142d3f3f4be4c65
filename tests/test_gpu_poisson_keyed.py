"""GPU suite (-m gpu): the keyed Poisson draw of PoissonBanditLadiesSampler / PoissonLadiesSampler (``draw="device"``, DESIGN.md
section 21) against the oracle's keyed mode (tests/poisson_keyed_ref.py), bit for bit: node lists, indptr, src, dst, eid, the
bf16 bits of edge_weights / q_ij / node_prob, c, iters, all_one and the counts.  Also: the stream path with the keyed uniforms
planted, the static-shape path, the draw state, torch's generator, and the two other kernel routes (BLISS_FUSE_SCALE=0,
BLISS_BINS=0) in child processes."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, ETA, FAN = 20231, 0.1, [24, 16, 12]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _cpu_graph(V, E, gseed, n_seeds):
    from bliss_gnn_amd.synth import chung_lu_csc
    from oracle import bliss_oracle as bo
    ip, ix, ei = chung_lu_csc(V, E, seed=gseed)
    og = bo.CSC(ip, ix, ei)
    seeds = torch.randperm(V, generator=torch.Generator().manual_seed(4))[:n_seeds].to(torch.int32)
    return og, seeds, bo.normalized_edata(og)


def _toy():
    from oracle import bliss_oracle as bo
    og = bo.prepare_graph(torch.tensor([2, 3, 3, 4]), torch.tensor([0, 0, 1, 1]), 5)
    return og, torch.tensor([0, 1], dtype=torch.int32), bo.normalized_edata(og)


def _gpu_graph(og, cuda):
    import bliss_gnn_amd as bg
    g = bg.Graph(og.indptr.to(cuda), og.indices.to(cuda), og.eid.to(cuda))
    g.edata["w"] = bg.normalized_edata(g)
    return g


def _sampler(kind, fan, imp=True, dep=False, draw="device"):
    import bliss_gnn_amd as bg
    kw = dict(draw=draw, layer_dependency=dep) if draw == "device" else {}
    if kind == "bandit":
        return bg.PoissonBanditLadiesSampler(fan, importance_sampling=imp, node_embedding="features", num_steps=1000, eta=ETA,
                                             model="sage", **kw)
    return bg.PoissonLadiesSampler(fan, importance_sampling=imp, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_bandit(key, fan, step, imp, dep):
    """Steps 0 .. step of the oracle's keyed bandit sampler with its EXP3 update between them (embed norms from a fixed
    generator): per step (input nodes, blocks, embed norms, weights after the update).  Computed once per configuration."""
    import poisson_keyed_ref as ref
    from oracle import bliss_oracle as bo
    og, seeds, edge_w = _cpu_graph(*key) if key != "toy" else _toy()
    w = torch.ones(len(fan), og.num_edges, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(6)
    out = []
    for t in range(step + 1):
        inp, _, blocks = ref.sample_blocks_bandit(og, seeds, list(fan), w, ETA, SEED, t, imp, dep)
        en = [(torch.rand(b.n_src, generator=gen) * 20).bfloat16() for b in blocks]
        w, _ = bo.exp3(og, blocks, w, edge_w, en)
        out.append((inp, blocks, en, w))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_ladies(key, fan, step, imp, dep):
    import poisson_keyed_ref as ref
    og, seeds, edge_w = _cpu_graph(*key) if key != "toy" else _toy()
    inp, _, blocks = ref.sample_blocks_ladies(og, seeds, list(fan), edge_w, SEED, step, imp, dep)
    return inp, blocks


def _compare(inp, blocks, o_inp, o_blocks, fan, bandit):
    """Every field the issue lists, bit for bit; blocks input-most first on both sides."""
    import bliss_gnn_amd as bg
    assert torch.equal(inp.cpu().long(), o_inp)
    assert len(blocks) == len(o_blocks) == len(fan)
    for b, ob, num in zip(blocks, o_blocks, fan):
        c = b._counts
        C = ob.trace["cand_nid"].numel()
        assert (c.S, c.E, c.C, c.K, c.B, c.err) == (ob.n_dst, ob.trace["E"], C, ob.n_src, ob.src.numel(), 0)
        assert c.c == ob.trace["c"] and c.iters == ob.trace["iters"] and c.all_one == int(C <= num)
        assert torch.equal(b.srcdata[bg.NID].cpu().long(), ob.src_nid) and torch.equal(b.dstdata[bg.NID].cpu().long(), ob.dst_nid)
        assert torch.equal(b.indptr.cpu().long(), ob.indptr)
        assert torch.equal(b.src.cpu().long(), ob.src) and torch.equal(b.dst.cpu().long(), ob.dst)
        assert torch.equal(b.edata[bg.EID].cpu().long(), ob.eid)
        assert torch.equal(_bits(b.edata["edge_weights"]), _bits(ob.edge_weights))
        assert torch.equal(b._trace["cand_nid"].cpu().long(), ob.trace["cand_nid"])
        if bandit:
            assert torch.equal(_bits(b.edata["q_ij"]), _bits(ob.q_ij))
            assert torch.equal(_bits(b.srcdata["node_prob"]), _bits(ob.node_prob))


def _same_blocks(a, b):
    import bliss_gnn_amd as bg
    for x, y in zip(a, b):
        cx, cy = x._counts, y._counts
        assert (cx.S, cx.E, cx.C, cx.K, cx.B, cx.c, cx.iters, cx.all_one) == (cy.S, cy.E, cy.C, cy.K, cy.B, cy.c, cy.iters, cy.all_one)
        for f in ("indptr", "src", "dst", "pos"):
            assert torch.equal(getattr(x, f), getattr(y, f)), f
        assert torch.equal(x.srcdata[bg.NID], y.srcdata[bg.NID]) and torch.equal(x.edata[bg.EID], y.edata[bg.EID])
        assert torch.equal(_bits(x._edge_weights), _bits(y._edge_weights))
        assert torch.equal(_bits(x._q), _bits(y._q)) and torch.equal(_bits(x._node_prob), _bits(y._node_prob))


KEY600 = (600, 7000, 21, 64)


def test_toy_graph(cuda):
    og, seeds, _ = _toy()
    g = _gpu_graph(og, cuda)
    s = _sampler("bandit", [2])
    s.reset_draw(seed=SEED)
    inp, _, blocks = s.sample_blocks(g, seeds.to(cuda))
    o_inp, o_blocks, _, _ = _oracle_bandit("toy", (2,), 0, True, False)[0]
    _compare(inp, blocks, o_inp, o_blocks, [2], True)
    s = _sampler("ladies", [2])
    s.reset_draw(seed=SEED)
    inp, _, blocks = s.sample_blocks(g, seeds.to(cuda))
    _compare(inp, blocks, *_oracle_ladies("toy", (2,), 0, True, False), [2], False)


@pytest.mark.parametrize("dep", [False, True])
@pytest.mark.parametrize("imp", [True, False])
def test_bandit_two_steps_with_the_exp3_update_between(cuda, imp, dep):
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    s = _sampler("bandit", FAN, imp, dep)
    s.reset_draw(seed=SEED)
    before = torch.get_rng_state()
    for t, (o_inp, o_blocks, en, o_w) in enumerate(_oracle_bandit(KEY600, tuple(FAN), 1, imp, dep)):
        assert s.draw_step() == t
        inp, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        _compare(inp, blocks, o_inp, o_blocks, FAN, True)
        for b, e_ in zip(blocks, en):
            b.srcdata["embed_norm"] = e_.to(cuda)
        s.exp3(blocks, g)
        s.check_errors()
        assert torch.equal(_bits(s.exp3_weights), _bits(o_w))
    assert s.draw_step() == 2 and torch.equal(before, torch.get_rng_state())


@pytest.mark.parametrize("dep", [False, True])
@pytest.mark.parametrize("imp", [True, False])
def test_ladies_two_steps(cuda, imp, dep):
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    s = _sampler("ladies", FAN, imp, dep)
    s.reset_draw(seed=SEED)
    before = torch.get_rng_state()
    for t in range(2):
        inp, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        _compare(inp, blocks, *_oracle_ladies(KEY600, tuple(FAN), t, imp, dep), FAN, False)
    assert s.draw_step() == 2 and torch.equal(before, torch.get_rng_state())


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_all_one_early_out(cuda, kind):
    fan = [4096] * 3
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    s = _sampler(kind, fan)
    s.reset_draw(seed=SEED)
    inp, _, blocks = s.sample_blocks(g, seeds.to(cuda))
    if kind == "bandit":
        o_inp, o_blocks, _, _ = _oracle_bandit(KEY600, tuple(fan), 0, True, False)[0]
    else:
        o_inp, o_blocks = _oracle_ladies(KEY600, tuple(fan), 0, True, False)
    _compare(inp, blocks, o_inp, o_blocks, fan, kind == "bandit")
    assert all(b._counts.all_one == 1 and b._counts.K == b._counts.C for b in blocks) and s.draw_step() == 1


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_look_back_crosses_chunks(cuda, kind):
    """More than 1024 candidates in the first-sampled layers: several workgroups of the select, whose ranks come from the
    look-back over their predecessors, and the last ticket of a multi-workgroup launch bumps the step."""
    key, fan = (6000, 60000, 33, 256), [512, 256, 128]
    og, seeds, _ = _cpu_graph(*key)
    g = _gpu_graph(og, cuda)
    s = _sampler(kind, fan)
    s.reset_draw(seed=SEED)
    inp, _, blocks = s.sample_blocks(g, seeds.to(cuda))
    if kind == "bandit":
        o_inp, o_blocks, _, _ = _oracle_bandit(key, tuple(fan), 0, True, False)[0]
    else:
        o_inp, o_blocks = _oracle_ladies(key, tuple(fan), 0, True, False)
    sizes = [b._counts.C for b in reversed(blocks)]                       # sampling order
    print(kind, "C per layer (sampling order):", sizes, "K:", [b._counts.K for b in reversed(blocks)])
    assert sizes[0] > 1024 and sizes[1] > 1024
    _compare(inp, blocks, o_inp, o_blocks, fan, kind == "bandit")
    assert s.draw_step() == 1


@pytest.mark.parametrize("dep", [False, True])
@pytest.mark.parametrize("imp", [True, False])
@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_stream_path_with_planted_keyed_uniforms_gives_the_same_blocks(cuda, kind, imp, dep):
    """Equality (a): the existing select, handed uniforms=[keyed_uniform(seed, t, n', cand_nid_n) per layer]."""
    from oracle import bliss_oracle as bo
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    keyed, stream = _sampler(kind, FAN, imp, dep), _sampler(kind, FAN, imp, draw="host")
    keyed.reset_draw(seed=SEED, step=5)
    _, _, kb = keyed.sample_blocks(g, seeds.to(cuda))
    planted = [bo.keyed_uniform(SEED, 5, 0 if dep else n, b._trace["cand_nid"].cpu().long()) for n, b in enumerate(reversed(kb))]
    before = torch.get_rng_state()
    _, _, sb = stream.sample_blocks(g, seeds.to(cuda), uniforms=planted)
    assert torch.equal(before, torch.get_rng_state())
    _same_blocks(kb, sb)
    with pytest.raises(ValueError):
        keyed.sample_blocks(g, seeds.to(cuda), uniforms=planted)
    assert keyed.draw_step() == 6


@pytest.mark.parametrize("kind", ["bandit", "ladies"])
def test_static_path_draw_state_and_replay(cuda, kind):
    """sample_blocks_static = sample_blocks for the same draw state; the step rises by one per call, eager, static and replayed
    from a captured graph; reset_draw reproduces a step; torch's generator is never touched."""
    import bliss_gnn_amd as bg
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    seeds = seeds.to(cuda)
    s = _sampler(kind, FAN)
    torch.manual_seed(SEED)                                                # seed=None: torch.initial_seed() at first use
    before = torch.get_rng_state()
    exact = []
    for t in range(4):
        assert s.draw_step() == t
        exact.append(s.sample_blocks(g, seeds)[2])
        if kind == "bandit" and t == 1:                                    # (now: the blocks' _trace are views of the workspace)
            _compare(exact[1][0].srcdata[bg.NID], exact[1], *_oracle_bandit_step1_plain(), FAN, True)
    assert not torch.equal(exact[0][0].srcdata[bg.NID], exact[1][0].srcdata[bg.NID])

    def trimmed(padded, cnts):
        out = []
        for bp, c in zip(padded, reversed(cnts)):
            out.append(dict(indptr=bp.indptr[:c.S + 1].clone(), src=bp.src[:c.B].clone(), dst=bp.dst[:c.B].clone(),
                            nid=bp.srcdata[bg.NID][:c.K].clone(), eid=bp.edata[bg.EID][:c.B].clone(),
                            w=_bits(bp.edata["edge_weights"][:c.B]), size=(c.S, c.E, c.C, c.K, c.B, c.c, c.iters, c.all_one)))
        return out

    def check(got, want):
        for a, b in zip(got, want):
            c = b._counts
            assert a["size"] == (c.S, c.E, c.C, c.K, c.B, c.c, c.iters, c.all_one)
            assert torch.equal(a["indptr"], b.indptr) and torch.equal(a["src"], b.src) and torch.equal(a["dst"], b.dst)
            assert torch.equal(a["nid"], b.srcdata[bg.NID]) and torch.equal(a["eid"], b.edata[bg.EID])
            assert torch.equal(a["w"], _bits(b.edata["edge_weights"]))

    s.reset_draw(seed=SEED, step=0)                                        # the same steps again, through the static path
    assert s.draw_step() == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, _, padded = s.sample_blocks_static(g, seeds)
        side.synchronize()
        check(trimmed(padded, s.finish_static()), exact[0])
        assert s.draw_step() == 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, _, padded = s.sample_blocks_static(g, seeds)
    assert s.draw_step() == 1                                              # the capture executed nothing
    for t in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        check(trimmed(padded, s.finish_static()), exact[t])
        assert s.draw_step() == t + 1
    s.reset_draw(seed=SEED, step=2)                                        # a fresh state object: eager call on step 2
    check(trimmed(*_static_once(s, g, seeds)), exact[2])
    assert torch.equal(before, torch.get_rng_state())
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, seeds, external_rng=True)
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, seeds, chain_rng=True)
    with pytest.raises(NotImplementedError):
        s.sample_blocks_static(g, seeds, part="main", external_rng=True)
    assert s.draw_step() == 3
    del graph


def _static_once(s, g, seeds):
    _, _, padded = s.sample_blocks_static(g, seeds)
    torch.cuda.synchronize()
    return padded, s.finish_static()


def _oracle_bandit_step1_plain():
    """Step 1 of the keyed bandit oracle WITHOUT an update between the steps (uniform weights): what a second plain
    sample_blocks call draws."""
    import poisson_keyed_ref as ref
    og, seeds, _ = _cpu_graph(*KEY600)
    w = torch.ones(len(FAN), og.num_edges, dtype=torch.bfloat16)
    inp, _, blocks = ref.sample_blocks_bandit(og, seeds, FAN, w, ETA, SEED, 1)
    return inp, blocks


def _dump(path):
    """Child process: the default configuration's two families on the 600-node graph, saved as CPU tensors."""
    import bliss_gnn_amd as bg
    cuda = torch.device("cuda:0")
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    out = {}
    for kind in ("bandit", "ladies"):
        s = _sampler(kind, FAN)
        s.reset_draw(seed=SEED, step=1)
        _, _, blocks = s.sample_blocks(g, seeds.to(cuda))
        out[kind] = [dict(indptr=b.indptr.cpu(), src=b.src.cpu(), dst=b.dst.cpu(), nid=b.srcdata[bg.NID].cpu(),
                          eid=b.edata[bg.EID].cpu(), w=_bits(b._edge_weights), q=_bits(b._q), node_prob=_bits(b._node_prob),
                          size=(b._counts.S, b._counts.E, b._counts.C, b._counts.K, b._counts.B, b._counts.c, b._counts.iters,
                                b._counts.all_one)) for b in blocks]
        out[kind + "_route"] = (s._engine.n_bins > 0, s._engine.fuse_scale, s.draw_step())
    torch.save(out, path)


def test_other_kernel_routes_give_the_defaults_blocks(cuda, tmp_path):
    """BLISS_FUSE_SCALE=0 (the scale as a launch of its own, NULL rng_ctl) and BLISS_BINS=0 (the atomic candidate passes): one
    fresh child process each, one after the other, against this process's default route."""
    import bliss_gnn_amd as bg
    og, seeds, _ = _cpu_graph(*KEY600)
    g = _gpu_graph(og, cuda)
    want = {}
    for kind in ("bandit", "ladies"):
        s = _sampler(kind, FAN)
        s.reset_draw(seed=SEED, step=1)
        want[kind] = s.sample_blocks(g, seeds.to(cuda))[2]
        assert s._engine.n_bins > 0 and s._engine.fuse_scale
    for var, route in (("BLISS_FUSE_SCALE", (True, False, 2)), ("BLISS_BINS", (False, True, 2))):
        path = str(tmp_path / (var + ".pt"))
        env = dict(os.environ, **{var: "0"})
        env.pop("BLISS_NBINS", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = torch.load(path)
        for kind in ("bandit", "ladies"):
            assert got[kind + "_route"] == route, (var, got[kind + "_route"])
            for a, b in zip(got[kind], want[kind]):
                c = b._counts
                assert a["size"] == (c.S, c.E, c.C, c.K, c.B, c.c, c.iters, c.all_one)
                assert torch.equal(a["indptr"], b.indptr.cpu()) and torch.equal(a["src"], b.src.cpu())
                assert torch.equal(a["dst"], b.dst.cpu()) and torch.equal(a["nid"], b.srcdata[bg.NID].cpu())
                assert torch.equal(a["eid"], b.edata[bg.EID].cpu()) and torch.equal(a["w"], _bits(b._edge_weights))
                assert torch.equal(a["q"], _bits(b._q)) and torch.equal(a["node_prob"], _bits(b._node_prob))


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    _dump(sys.argv[1])
