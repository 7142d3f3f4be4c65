"""CPU restatement of the device-side multinomial draw (csrc/mn_draw.hip), on top of the oracle's
``keyed_uniform``.  The rule is normative; the kernels and this file both implement it:

    u_j   = keyed_uniform(seed, step, layer, nid_j) + 2^-24          in (0, 1], exact in fp32
    key_j = float32(-log(float64(u_j)) / float64(p_j))               +inf unless p_j > 0; the sign of a zero key is dropped
    drawn = the k smallest pairs (bit pattern of key_j, j)           keys are >= 0: their bits order as unsigned integers
"""
import numpy as np
import torch

from oracle.bliss_oracle import keyed_uniform


def keyed_uniforms(nid, seed, step, layer):
    """The keyed uniforms of candidates ``nid`` (any integer array / tensor), fp32 in (0, 1]."""
    nid = torch.as_tensor(np.asarray(nid)).to(torch.int64)
    return keyed_uniform(seed, step, layer, nid).numpy() + np.float32(2.0 ** -24)


def keys(p_bf16, nid, seed, step, layer, uniforms=None):
    """fp32 race keys.  ``p_bf16``: torch.bfloat16 importances; ``uniforms``: optional fp32 values replacing the keyed ones."""
    p = p_bf16.detach().cpu().to(torch.bfloat16).to(torch.float64).numpy()
    u = keyed_uniforms(nid, seed, step, layer) if uniforms is None else np.asarray(uniforms, dtype=np.float32)[: p.shape[0]]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        k = np.abs((-np.log(u.astype(np.float64)) / p).astype(np.float32))
    k[~(p > 0)] = np.float32(np.inf)
    return k


def select(keys, k):
    """Positions of the ``min(k, C)`` smallest (key bits, position) pairs, in that order."""
    bits = np.ascontiguousarray(keys, dtype=np.float32).view(np.uint32)
    order = np.lexsort((np.arange(bits.shape[0]), bits))
    return order[: max(0, min(int(k), bits.shape[0]))].astype(np.int64)


def drawn_mask(keys, k):
    m = np.zeros(np.asarray(keys).shape[0], dtype=np.int32)
    m[select(keys, k)] = 1
    return m


def inclusion_probabilities(p, k):
    """Exact inclusion probabilities of successive sampling without replacement, by enumeration of the ordered k-tuples."""
    import itertools
    p = np.asarray(p, dtype=np.float64)
    pi = np.zeros(p.shape[0])
    for t in itertools.permutations(range(p.shape[0]), k):
        rest, pr = p.sum(), 1.0
        for j in t:
            pr *= p[j] / rest
            rest -= p[j]
        pi[list(t)] += pr
    return pi
