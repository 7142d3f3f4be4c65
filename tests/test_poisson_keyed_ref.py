"""CPU suite: the oracle in keyed mode as tests/poisson_keyed_ref.py drives it -- what the GPU suite compares the keyed Poisson
draw against."""
import math

import torch

import poisson_keyed_ref as ref
from oracle import bliss_oracle as bo

FAN = [24, 16, 12]


def _graph():
    from bliss_gnn_amd.synth import chung_lu_csc
    ip, ix, ei = chung_lu_csc(600, 7000, seed=21)
    g = bo.CSC(ip, ix, ei)
    seeds = torch.randperm(600, generator=torch.Generator().manual_seed(4))[:64].to(torch.int32)
    return g, seeds, bo.normalized_edata(g)


def _same(a, b):
    if not torch.equal(a[0], b[0]):
        return False
    return all(torch.equal(x.src, y.src) and torch.equal(x.eid, y.eid) and torch.equal(x.src_nid, y.src_nid)
               and torch.equal(x.edge_weights.view(torch.int16), y.edge_weights.view(torch.int16)) for x, y in zip(a[2], b[2]))


def _both(g, seeds, w, seed, step, **kw):
    ones = torch.ones(3, g.num_edges, dtype=torch.bfloat16)
    return (ref.sample_blocks_bandit(g, seeds, FAN, ones, 0.1, seed, step, **kw),
            ref.sample_blocks_ladies(g, seeds, FAN, w, seed, step, **kw))


def test_deterministic_in_seed_and_step_and_different_between_steps():
    g, seeds, w = _graph()
    torch.manual_seed(1)
    state = torch.get_rng_state()
    a, b, c, d = _both(g, seeds, w, 77, 3), _both(g, seeds, w, 77, 3), _both(g, seeds, w, 77, 4), _both(g, seeds, w, 78, 3)
    assert torch.equal(state, torch.get_rng_state())                     # no generator takes part
    for fam in range(2):
        assert _same(a[fam], b[fam])
        assert not _same(a[fam], c[fam]) and not _same(a[fam], d[fam])
        for blk in a[fam][2]:                                            # seeds are always kept, in place
            assert torch.equal(blk.src_nid[:blk.n_dst], blk.dst_nid)


def test_layer_dependency_uses_layer_zero_throughout():
    g, seeds, w = _graph()
    seen = []
    for fam, (dep, ind) in enumerate(zip(_both(g, seeds, w, 5, 9, layer_dependency=True), _both(g, seeds, w, 5, 9))):
        assert not _same(dep, ind)
        for n, blk in enumerate(reversed(dep[2])):                       # sampling order
            nid, P = blk.trace["cand_nid"], blk.trace["P"]
            u0 = bo.keyed_uniform(5, 9, 0, nid)
            assert torch.equal(blk.trace["chosen"], torch.arange(nid.numel())[u0 < P.float()])
            if n:
                assert not torch.equal(u0, bo.keyed_uniform(5, 9, n, nid))
            seen.append(dict(zip(nid.tolist(), u0.tolist())))
    for a in seen:                                                       # one variate per node for all layers (and both families)
        for b in seen:
            assert all(b[k] == v for k, v in a.items() if k in b)
    assert ref.layer_key(2, True) == 0 and ref.layer_key(2, False) == 2


def test_planted_uniforms_reproduce_the_keyed_blocks():
    """Equality (a) on the oracle's side: its stream mode with the keyed uniforms planted = its keyed mode."""
    g, seeds, w = _graph()
    ones = torch.ones(3, g.num_edges, dtype=torch.bfloat16)
    keyed = ref.sample_blocks_bandit(g, seeds, FAN, ones, 0.1, 11, 2)
    planted = bo.sample_blocks_bandit(g, seeds, FAN, ones, 0.1, uniforms=ref.layer_uniforms(keyed[2], 11, 2))
    assert _same(keyed, planted)
    keyed = ref.sample_blocks_ladies(g, seeds, FAN, w, 11, 2)
    planted = bo.sample_blocks_ladies(g, seeds, FAN, w, uniforms=ref.layer_uniforms(keyed[2], 11, 2))
    assert _same(keyed, planted)


def test_inclusion_statistic():
    """DESIGN.md section 12's bound: over steps 0 .. 2047 the number of inclusions of every node lies within 5 sigma of
    2048 * P_j, for every layer key (largest deviations of the oracle: 3.58, 3.33 and 2.90 sigma for layers 0, 1, 2)."""
    j = torch.arange(256)
    nid = 7 * j + 3
    P = ((j % 16 + 1).float() / 17).bfloat16()
    Pf = P.float()
    for layer in range(3):
        cnt = torch.zeros(256, dtype=torch.int64)
        for t in range(2048):
            cnt += (bo.keyed_uniform(1234, t, layer, nid) < Pf).long()
        sigma = torch.sqrt(2048 * Pf.double() * (1 - Pf.double()))
        dev = ((cnt.double() - 2048 * Pf.double()).abs() / sigma).max().item()
        print(layer, dev)
        assert math.isfinite(dev) and dev <= 5.0
