// The counter-based uniform of the keyed draws (oracle: bliss_oracle.keyed_uniform): the draw of node `nid` in sampling layer
// `layer` of draw step `step` is a pure function of (seed, step, layer, nid).  Used by the keyed Poisson select of the layer-wise
// samplers (csrc/sampler.hip); csrc/shard.hip, csrc/shard_dense.hip, csrc/mn_draw.hip and
// csrc/neighbor_tail.cuh keep their own copies of the same two functions.
#pragma once
#include "common.cuh"

namespace {

// (seed, step, layer) -> key.  The (seed, step) pair is FINALISED before the layer and the node id are mixed in: with the step in
// the low bits beside the id, an aligned block of 2^k ids would see the same 2^k uniforms, permuted, on consecutive steps.
__device__ __forceinline__ unsigned long long keyed_mix(unsigned long long seed, unsigned long long step, int layer) {
  unsigned long long key = seed * 0x9E3779B97F4A7C15ull + step;
  key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
  key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
  key ^= key >> 31;
  return key ^ ((unsigned long long)((unsigned)layer & 0xffu) << 56);
}

// SplitMix64 finaliser of key ^ node id; top 24 bits -> u = r * 2^-24 in [0, 1), exact in fp32 (the resolution of torch's CPU stream)
__device__ __forceinline__ float keyed_u24(unsigned long long key, int nid) {
  unsigned long long z = key ^ (unsigned long long)(unsigned)nid;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)(unsigned)(z >> 40) * (1.0f / 16777216.0f);
}

}  // namespace
