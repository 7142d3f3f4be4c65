// The EXP3 edge probability q_ij with the reference's bf16 roundings, shared by the layer-wise samplers (csrc/sampler.hip), the
// node-wise bandit sampler (csrc/neighbor_w.hip) and the weighted LABOR sampler (csrc/labor_w.hip).  The column sum `wsum` is the
// exact block-floating sum of common.cuh (rel_frac / bf_to_fixed_wide / fixed_wide_to_bf), rounded once to bf16.  The two node-wise
// samplers also share the per-seed (bf16 sum, eta / n) record of a column, found by one workgroup, and q of a CSC position.
#pragma once
#include "common.cuh"

namespace {

// q_ij = eta/n_i + (1-eta) * w_ij / sum_j w_ij        bandit_sampler.py:131-137
__device__ __forceinline__ bf16_t edge_q(bf16_t w, bf16_t wsum, int n, float eta_f, float ome_f) {
  float wd = rbf(bf2f(w) / bf2f(wsum));     // :131 e_div_v
  // :137 (self.eta / n_i).bfloat16(): Python `scalar / tensor` is Tensor.__rtruediv__ = reciprocal() * scalar,
  // i.e. TWO fp32 roundings on the int32 -> fp32 degree, then one to bf16
  float a = rbf((1.0f / (float)n) * eta_f);
  float b = rbf(ome_f * wd);                // :137 (1 - self.eta) * exp_weights_divided
  return f2bf(a + b);                       // :137 v_add_e
}

// the same with the per-seed part a = rbf((1/n) * eta) taken from k_col_sums' per-seed record
__device__ __forceinline__ bf16_t edge_q_pre(bf16_t w, bf16_t wsum, float a, float ome_f) {
  float wd = rbf(bf2f(w) / bf2f(wsum));
  float b = rbf(ome_f * wd);
  return f2bf(a + b);
}

// q of the edge at CSC position pos; cf = the column's (bf16 sum, fp32 bits of the eta / n term) in EXP3 mode
__device__ __forceinline__ bf16_t wn_q(int mode, const bf16_t* __restrict__ prob, int pos, uint2 cf, float ome_f) {
  const bf16_t x = prob[pos];
  return mode == BLISS_WN_EXP3 ? edge_q_pre(x, (bf16_t)(cf.x & 0xffffu), __uint_as_float(cf.y), ome_f) : x;
}

// workgroup-wide reductions for a workgroup of TPB threads; `sh` needs TPB / 64 words
template <int TPB>
__device__ __forceinline__ long long wn_block_sum_i64(long long v, long long* sh) {
  v = wave_total_i64(v);
  __syncthreads();                                                  // sh free again
  if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
#pragma unroll
  for (int w = 0; w < TPB / BLISS_WAVE; ++w) t += sh[w];
  return t;
}

template <int TPB>
__device__ __forceinline__ int wn_block_max_u31(int v, long long* sh) {
  v = wave_max_u31(v);
  __syncthreads();                                                  // sh free again
  if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < TPB / BLISS_WAVE; ++w) t = max(t, (int)sh[w]);
  return t;
}

// the EXP3-mode record of the column at CSC positions [a, a + d), d > 0, by the whole workgroup: sum_j w_ij exactly
// (csrc/sampler.hip:k_col_sums' block-floating form: integer adds, any order gives the same bits), rounded once to bf16, and the
// fp32 bits of rbf((1 / d) * eta)
template <int TPB>
__device__ __forceinline__ uint2 wn_col_record(const bf16_t* __restrict__ prob, int a, int d, float eta_f, long long* sh, int* bad) {
  const int tid = threadIdx.x;
  int emax = 1;
  for (int i = tid; i < d; i += TPB) emax = max(emax, bf_exp_field(prob[a + i]));
  emax = wn_block_max_u31<TPB>(emax, sh);
  const int wfrac = rel_frac(FRAC_DST, emax);
  long long part = 0, part_lo = 0;
  int sticky = 0;
  for (int i = tid; i < d; i += TPB) part += bf_to_fixed_wide(prob[a + i], wfrac, &part_lo, &sticky, bad);
  const long long hi = wn_block_sum_i64<TPB>(part, sh);
  const long long lo = wn_block_sum_i64<TPB>(part_lo, sh);
  const long long st = wn_block_sum_i64<TPB>(sticky, sh);
  const bf16_t wsum = fixed_wide_to_bf(hi, lo, st != 0, wfrac, bad);
  return make_uint2((unsigned)wsum, __float_as_uint(rbf((1.0f / (float)d) * eta_f)));
}

}  // namespace
