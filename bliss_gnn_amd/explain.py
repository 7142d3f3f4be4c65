"""Edge-weight gradients of a whole model: which sampled edges did this prediction lean on.

``edge_gradients(model, blocks, x, objective)`` differentiates ``objective(model(blocks, x))`` w.r.t. every block's
``edata["edge_weights"]`` through the model's own forward: the aggregation ops hand their edge weights a gradient
(``torch.ops.bliss.sddmm``, csrc/sddmm.hip).  Models whose layers detach the edge weights or ignore them are refused, by name,
before any launch."""
import torch

from .model import GATv2, GCN, SAGE
from .nn import TILE_KINDS


def refusal(model):
    """Why ``edge_gradients`` cannot differentiate ``model`` w.r.t. its blocks' edge weights, or None."""
    if isinstance(model, GATv2):
        return ("GATv2 ignores the blocks' edge weights (its messages are weighted by the attention alone), so the gradient is "
                "identically zero")
    if isinstance(model, GCN):
        if model.transforms in TILE_KINDS:
            return ('GCN(transforms="%s") runs the tile nodes, which detach the edge weights (DESIGN.md section 36, "Not built"); '
                    'transforms="library" differentiates' % model.transforms)
        return None
    if isinstance(model, SAGE):
        if model.transforms == "tile" and model.aggregator_type in ("pool", "gcn"):
            return ('SAGE(transforms="tile", aggregator_type="%s") runs the tile nodes, which detach the edge weights (DESIGN.md '
                    'section 36, "Not built"); transforms="auto" differentiates' % model.aggregator_type)
        return None
    return "edge_gradients covers the package's SAGE and GCN models, not %s" % type(model).__name__


def edge_gradients(model, blocks, x, objective):
    """[g_0, ..., g_{L-1}], g_l bf16 [len(blocks[l].src)] = d objective(model(blocks, x)) / d blocks[l].edata["edge_weights"].

    ``objective`` maps the model's output to a scalar tensor.  Every block's edge weights are swapped for a detached leaf copy
    (bf16 ones where a block has none) for the duration of the call and restored afterwards; the gradients come from
    ``torch.autograd.grad``, so no parameter's ``.grad`` is touched.  Entries past a capacity-padded block's live edge count are
    +0.  Raises NotImplementedError, naming the reason, before any launch for a model that does not differentiate w.r.t. the
    edge weights (``refusal``)."""
    why = refusal(model)
    if why is not None:
        raise NotImplementedError("edge_gradients: " + why)
    key = "edge_weights"
    saved, leaves = [], []
    try:
        for b in blocks:
            had = key in b.edata
            old = b.edata[key] if had else None
            saved.append((b, had, old))
            leaf = (old.detach().to(torch.bfloat16).clone() if had
                    else torch.ones(b.num_edges(), dtype=torch.bfloat16, device=b.device))
            leaf.requires_grad_(True)
            b.edata[key] = leaf
            leaves.append(leaf)
        with torch.enable_grad():
            value = objective(model(blocks, x))
            grads = torch.autograd.grad(value, leaves, allow_unused=True)
    finally:
        for b, had, old in saved:
            if had:
                b.edata[key] = old
            else:
                dict.pop(b.edata, key, None)
    missing = [l for l, g in enumerate(grads) if g is None]
    if missing:
        raise RuntimeError("edge_gradients: the model's forward did not use the edge weights of block(s) %r" % (missing,))
    return [g.detach() for g in grads]
