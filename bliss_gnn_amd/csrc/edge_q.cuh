// The EXP3 edge probability q_ij with the reference's bf16 roundings, shared by the layer-wise samplers (csrc/sampler.hip) and the
// node-wise bandit sampler (csrc/neighbor_w.hip).  The column sum `wsum` is the exact block-floating sum of common.cuh
// (rel_frac / bf_to_fixed_wide / fixed_wide_to_bf), rounded once to bf16.
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

}  // namespace
