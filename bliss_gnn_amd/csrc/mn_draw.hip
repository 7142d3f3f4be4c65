// The multinomial samplers' draw on the device (BanditLadiesSampler / LadiesSampler with draw="device").
//
// torch.multinomial(p, k, replacement=False) on the CPU is the exponential race topk(p / Exp(1)); its exponentials come from a serial
// host stream that cannot be restated (tests/test_oracle.py).  The same algorithm with COUNTER-BASED uniforms is a correct draw
// without replacement that needs neither a serial stream nor the host -- the defined-mode arrangement of the sharded sampler
// (csrc/shard.hip): the rule below is normative, tests/mn_draw_ref.py restates it on the CPU and drives the oracle with it.
//
//   u_j   = keyed_uniform(seed, step, layer, nid_j) + 2^-24          in (0, 1], exact in fp32  (csrc/shard.hip:keyed_u24)
//   key_j = (float)(-log((double)u_j) / (double)p_j)                  one fp64 quotient, rounded once;  +inf unless p_j > 0
//   drawn = the k = min(fanout, C) smallest pairs (bits of key_j, j)  keys are >= 0: their bit patterns order as unsigned integers
//
// bliss_multinomial_draw = five launches on one stream, no host round trip, C read on the device:
//   k_md_pass<0>   keys + histogram of key bits 31..21     | every workgroup counts in LDS-private bins and flushes the non-empty
//   k_md_pass<1>   histogram of bits 20..10 under the digit | ones to the global bins; the LAST workgroup (a ticket) scans the bins,
//   k_md_pass<2>   histogram of bits  9..0  under both      | fixes the digit and what is left of k, and leaves bins and ticket ZERO
//   k_md_tie_count per 1024-candidate chunk: how many keys equal the threshold T
//   k_md_mark      drawn_j = key_j < T, or key_j == T and fewer than r equal keys at lower positions (r = what is left of k)
// Every word a replay relies on (bins, ticket) is left zero by the kernel that used it; threshold, remainder and the chunk
// counts are rewritten by every call before they are read.
#include "common.cuh"
#include "bliss_gnn.h"

namespace {

#define MD_TPB 1024
#define MD_BINS 2048
#define MD_CHUNK 1024
#define MD_HDR 8            // scratch words: [0] ticket, [1] threshold (prefix while the passes run), [2] what is left of k
#define MD_INF 0x7f800000u

// SplitMix64 finaliser of (seed, step, layer, node id)   (= csrc/shard.hip, csrc/shard_dense.hip, oracle keyed_uniform)
__device__ __forceinline__ unsigned long long md_key(unsigned long long seed, unsigned long long step, int layer) {
  unsigned long long key = seed * 0x9E3779B97F4A7C15ull + step;
  key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
  key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
  key ^= key >> 31;
  return key ^ ((unsigned long long)((unsigned)layer & 0xffu) << 56);
}
// top 24 bits r -> (r + 1) * 2^-24 = keyed_uniform + 2^-24, exact
__device__ __forceinline__ float md_uniform(unsigned long long key, int nid) {
  unsigned long long z = key ^ (unsigned long long)(unsigned)nid;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (float)((unsigned)(z >> 40) + 1u) * (1.0f / 16777216.0f);
}
// the race key's bit pattern, sign cleared (u = 1 gives -0 / p = -0: the key is 0)
__device__ __forceinline__ unsigned md_race_key(float u, bf16_t pb) {
  const float p = bf2f(pb);
  if (!(p > 0.0f)) return MD_INF;                       // zero importance: taken only when fewer than k positive ones exist
  const float k = (float)(-log((double)u) / (double)p);
  return __float_as_uint(k) & 0x7fffffffu;
}

template <int PASS>
__global__ void __launch_bounds__(MD_TPB) k_md_pass(const int* __restrict__ cand_nid, const bf16_t* __restrict__ p,
                                                    const LayerCounts* __restrict__ cnt, int cap_c, int fanout,
                                                    const float* __restrict__ uniforms, unsigned long long seed, long long* step_dev,
                                                    int layer, int bump_step, unsigned* keys, unsigned* scr) {
  constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  constexpr int ABOVE = PASS == 0 ? 32 : (PASS == 1 ? 21 : 10);       // the bits the earlier passes have fixed start here
  constexpr int NB = PASS == 2 ? 1024 : 2048;
  __shared__ int lb[MD_BINS];
  __shared__ int sh[17];
  __shared__ int sh_last;
  const int C = min(cnt->C, cap_c);
  const unsigned prefix = PASS == 0 ? 0u : scr[1];
  const int k = PASS == 0 ? min(fanout, C) : (int)scr[2];
  unsigned long long key = 0;
  if (PASS == 0 && !uniforms) key = md_key(seed, (unsigned long long)*step_dev, layer);
  for (int b = threadIdx.x; b < NB; b += MD_TPB) lb[b] = 0;
  __syncthreads();
  for (int j = blockIdx.x * MD_TPB + threadIdx.x; j < C; j += gridDim.x * MD_TPB) {
    unsigned kb;
    if (PASS == 0) {
      kb = md_race_key(uniforms ? uniforms[j] : md_uniform(key, cand_nid[j]), p[j]);
      keys[j] = kb;
      atomicAdd(&lb[kb >> SHIFT], 1);                   // (sign bit clear: < 2048)
    } else {
      kb = keys[j];
      if ((kb >> ABOVE) == (prefix >> ABOVE)) atomicAdd(&lb[(kb >> SHIFT) & (NB - 1)], 1);
    }
  }
  __syncthreads();
  int* bins = (int*)scr + MD_HDR;
  for (int b = threadIdx.x; b < NB; b += MD_TPB) {
    const int v = lb[b];
    if (v) atomicAdd(bins + b, v);
  }
  // the bins are complete when every workgroup has passed here: atomics drained, then a ticket (k_cand_number's hand-over)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    sh_last = atomicAdd(scr, 1u) == gridDim.x - 1;
    if (sh_last) __hip_atomic_store(scr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!sh_last) return;
  // the last workgroup: two bins per thread, read past this XCD's L2 and left zero
  int n0 = 0, n1 = 0;
  const int b0 = 2 * threadIdx.x;
  if (b0 < NB) {
    n0 = __hip_atomic_load(bins + b0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n1 = __hip_atomic_load(bins + b0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n0) __hip_atomic_store(bins + b0, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n1) __hip_atomic_store(bins + b0 + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  int tot;
  const int ex = block_excl_scan(n0 + n1, sh, &tot);
  if (k > 0 && ex < k && k <= ex + n0 + n1) {           // exactly one thread: the k-th smallest key has its digit here
    const bool first = k <= ex + n0;
    scr[1] = prefix | ((unsigned)(first ? b0 : b0 + 1) << SHIFT);
    scr[2] = (unsigned)(k - (first ? ex : ex + n0));
  }
  if (PASS == 0 && threadIdx.x == 0) {
    if (k <= 0) { scr[1] = 0u; scr[2] = 0u; }           // nothing to draw: no key is below 0, no tie is taken
    if (bump_step) *step_dev += 1;                      // (every workgroup has read the step: it did so before its ticket)
  }
}

__global__ void __launch_bounds__(MD_TPB) k_md_tie_count(const unsigned* __restrict__ keys, const LayerCounts* __restrict__ cnt, int cap_c,
                                                         unsigned* scr) {
  const int C = min(cnt->C, cap_c);
  const unsigned T = scr[1];
  int* tie = (int*)scr + MD_HDR + MD_BINS;
  const int nchunks = (C + MD_CHUNK - 1) / MD_CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int j = chunk * MD_CHUNK + threadIdx.x;
    const int n = __syncthreads_count(j < C && keys[j] == T);
    if (threadIdx.x == 0) tie[chunk] = n;
  }
}

__global__ void __launch_bounds__(MD_TPB) k_md_mark(const unsigned* __restrict__ keys, const LayerCounts* __restrict__ cnt, int cap_c,
                                                    const unsigned* __restrict__ scr, int* __restrict__ drawn) {
  __shared__ int sh[17];
  const int C = min(cnt->C, cap_c);
  const unsigned T = scr[1];
  const int r = (int)scr[2];
  const int* tie = (const int*)scr + MD_HDR + MD_BINS;
  const int nchunks = (C + MD_CHUNK - 1) / MD_CHUNK;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    int part = 0;                                       // equal keys in the chunks before this one (a few hundred words at most)
    for (int i = threadIdx.x; i < chunk; i += MD_TPB) part += tie[i];
    int before;
    block_excl_scan(part, sh, &before);
    const int j = chunk * MD_CHUNK + threadIdx.x;
    const unsigned kb = j < C ? keys[j] : 0xffffffffu;
    const int is_tie = (j < C && kb == T) ? 1 : 0;
    int tot;
    const int ex = block_excl_scan(is_tie, sh, &tot);
    if (j < C) drawn[j] = (kb < T || (is_tie && before + ex < r)) ? 1 : 0;
  }
}

static inline int md_grid(int n, int per, int cap) {
  int g = (n + per - 1) / per;
  return g < 1 ? 1 : (g > cap ? cap : g);
}

}  // namespace

extern "C" {

int64_t bliss_multinomial_draw_scratch_bytes(int32_t cap_c) {
  if (cap_c <= 0) return BLISS_EINVAL;
  const int64_t words = MD_HDR + MD_BINS + ((int64_t)cap_c + MD_CHUNK - 1) / MD_CHUNK;
  return (words * 4 + 15) & ~(int64_t)15;
}

int bliss_multinomial_draw(const int32_t* cand_nid, const void* p_bf16, const void* counts, int32_t cap_c, int32_t fanout,
                           const float* uniforms, uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step, void* scratch,
                           float* keys, int32_t* drawn, void* stream) {
  if (!cand_nid || !p_bf16 || !counts || !scratch || !keys || !drawn || cap_c <= 0 || fanout < 0) return BLISS_EINVAL;
  if (((uintptr_t)scratch & 15) || ((uintptr_t)keys & 3) || ((!uniforms || bump_step) && !step_dev)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const LayerCounts* cnt = (const LayerCounts*)counts;
  const bf16_t* p = (const bf16_t*)p_bf16;
  unsigned* kb = (unsigned*)keys;
  unsigned* scr = (unsigned*)scratch;
  const int gp = md_grid(cap_c, MD_TPB * 4, 256), gc = md_grid(cap_c, MD_CHUNK, 1024);
  k_md_pass<0><<<gp, MD_TPB, 0, st>>>(cand_nid, p, cnt, cap_c, fanout, uniforms, seed, (long long*)step_dev, layer, bump_step, kb, scr);
  k_md_pass<1><<<gp, MD_TPB, 0, st>>>(cand_nid, p, cnt, cap_c, fanout, uniforms, seed, (long long*)step_dev, layer, 0, kb, scr);
  k_md_pass<2><<<gp, MD_TPB, 0, st>>>(cand_nid, p, cnt, cap_c, fanout, uniforms, seed, (long long*)step_dev, layer, 0, kb, scr);
  k_md_tie_count<<<gc, MD_TPB, 0, st>>>(kb, cnt, cap_c, scr);
  k_md_mark<<<gc, MD_TPB, 0, st>>>(kb, cnt, cap_c, scr, drawn);
  return (int)hipGetLastError();
}

}  // extern "C"
