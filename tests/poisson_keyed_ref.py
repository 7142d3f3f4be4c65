"""The keyed Poisson draw of the two LADIES samplers, driven through the oracle: candidate ``nid`` of
sampling layer n (0 = sampled first) of draw step t is kept iff ``keyed_uniform(seed, t, n', nid) < float(P)``, n' = n, or 0 for
every layer with ``layer_dependency``.  Everything else is the oracle's stream-mode sampler: the bandit family through
``sample_blocks_bandit(uniform_fn=)``, the LADIES family through the same loop as ``sample_blocks_ladies`` built from the oracle's
primitives (that function has no ``uniform_fn``)."""
from oracle import bliss_oracle as bo


def layer_key(n, layer_dependency):
    return 0 if layer_dependency else n


def uniform_fn(seed, step, layer_dependency=False):
    """``uniform_fn(n, cand_nid)`` of the oracle's keyed mode for draw step ``step``."""
    return lambda n, nid: bo.keyed_uniform(seed, step, layer_key(n, layer_dependency), nid)


def sample_blocks_bandit(g, seeds, fanouts, exp3_weights, eta, seed, step, importance_sampling=True, layer_dependency=False):
    """PoissonBanditLadiesSampler(draw="device").sample_blocks: (input nodes, output nodes, blocks input-most first)."""
    return bo.sample_blocks_bandit(g, seeds, fanouts, exp3_weights, eta, poisson=True, importance_sampling=importance_sampling,
                                   uniform_fn=uniform_fn(seed, step, layer_dependency))


def sample_blocks_ladies(g, seeds, fanouts, edge_w, seed, step, importance_sampling=True, layer_dependency=False):
    """PoissonLadiesSampler(draw="device").sample_blocks, ladies_sampler.py:109-123 with the keyed uniforms."""
    import torch
    fn = uniform_fn(seed, step, layer_dependency)
    blocks = []
    seed_nodes = seeds.to(torch.int64)
    for n, block_id in enumerate(reversed(range(len(fanouts)))):
        fr = bo.expand_frontier(g, seed_nodes)
        w_e = edge_w[fr.eid]
        p, tr = bo.ladies_node_importance(fr, w_e, importance_sampling)
        # The rule takes P_j "exactly as the stream path computes it".  The package holds the LADIES importances in bf16 in BOTH
        # branches (ladies_sampler.LadiesSampler._mode: the 0 / 1 of the non-importance branch are bf16 on the device), the
        # reference builds fp32 ones there (ladies_sampler.py:50) and so does this primitive; the Poisson scale then runs in the
        # importances' dtype.  That difference is the stream path's own, older than the keyed draw, and is not the draw's to
        # change: the non-importance branch is cast here so that the scale and the weights run in the stream path's arithmetic.
        if not importance_sampling:
            p = p.bfloat16()
        P, c, iters = bo.poisson_scale(p, fr.n_seeds, fanouts[block_id])
        chosen = bo.poisson_draw(P, fn(n, fr.nid))
        blk = bo.generate_block(g, fr, chosen, P, w_e, hajek=False)
        blk.trace.update(tr)
        blk.trace.update(p=p, P=P, c=c, iters=iters, cand_nid=fr.nid, E=fr.pos.numel(), chosen=chosen)
        seed_nodes = blk.src_nid
        blocks.insert(0, blk)
    return seed_nodes, seeds, blocks


def layer_uniforms(blocks, seed, step, layer_dependency=False):
    """The planted ``uniforms=`` list (sampling order) that makes the stream path draw what the keyed path draws: per layer the
    keyed uniforms of that layer's candidates, in candidate order."""
    fn = uniform_fn(seed, step, layer_dependency)
    return [fn(n, blk.trace["cand_nid"]) for n, blk in enumerate(reversed(blocks))]
