// What the two LABOR samplers share (csrc/labor.hip, csrc/labor_is.hip) in front of the source-numbering tail: the per-source key,
// the clamped seed count, and the one-workgroup scan behind their counting kernels.
//   k_lb_scan    one workgroup: seg_ptr (degrees), indptr (c_s), S / E / B, clamps and error bits, the rest of the counts record
#pragma once
#include "neighbor_tail.cuh"

namespace {

// the source's key, top 32 bits; ov (planted keys) is indexed by node id
__device__ __forceinline__ unsigned lb_key(unsigned long long mk, const unsigned* __restrict__ ov, int u) {
  if (ov) return ov[u];
  unsigned long long z = mk ^ (unsigned long long)(unsigned)u;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (unsigned)(z >> 32);
}
__device__ __forceinline__ int lb_seed_count(int S_host, const int* __restrict__ S_dev, int cap_s) {
  const int S = S_host >= 0 ? S_host : *S_dev;
  return S > cap_s ? cap_s : (S < 0 ? 0 : S);
}

__global__ void __launch_bounds__(NB_SCAN_TPB) k_lb_scan(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
                                                         int S_host, const int* __restrict__ S_dev, int cap_s,
                                                         const int* __restrict__ col_cnt, LayerCounts* cnt, int* __restrict__ seg_ptr,
                                                         int* __restrict__ b_indptr, int cap_b, int cap_k) {
  __shared__ long long sh[17];
  __shared__ int sh_bad;
  int S = S_host >= 0 ? S_host : *S_dev;
  int bad = 0;
  if (S > cap_s) { S = cap_s; bad |= BLISS_ERR_CAP_SEEDS; }         // clamp: results invalid but in bounds
  if (S < 0) S = 0;
  if (S > cap_k) bad |= BLISS_ERR_CAP_KEPT;                         // (the seeds are the first S block sources)
  if (threadIdx.x == 0) sh_bad = 0;
  __syncthreads();
  long long run_d = 0, run_k = 0;
  for (int base = 0; base < S; base += NB_SCAN_TPB) {
    const int i = base + threadIdx.x;
    long long d = 0, k = 0;
    if (i < S) {
      const int nid = seeds[i];
      if ((unsigned)nid < (unsigned)V) {
        d = g_indptr[nid + 1] - g_indptr[nid];
        k = col_cnt[i];
      } else {
        bad |= BLISS_ERR_CAP_CAND;                                  // seed id out of range: an empty column
      }
    }
    long long td, tk;
    const long long exd = nb_scan64(d, sh, &td);
    const long long exk = nb_scan64(k, sh, &tk);
    if (i < S) {
      seg_ptr[i] = (int)min(run_d + exd, (long long)INT32_MAX);
      b_indptr[i] = (int)min(run_k + exk, (long long)cap_b);
    }
    run_d += td;
    run_k += tk;
  }
  // rows S .. cap_s are empty: capacity-padded consumers (static shapes, HIP-graph replay) may walk them
  for (int k = S + 1 + threadIdx.x; k <= cap_s; k += NB_SCAN_TPB) b_indptr[k] = (int)min(run_k, (long long)cap_b);
  if (bad) atomicOr(&sh_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    bad |= sh_bad;
    if (run_d > (long long)INT32_MAX) { bad |= BLISS_ERR_CAP_FRONTIER; run_d = INT32_MAX; }
    if (run_k > (long long)cap_b) { bad |= BLISS_ERR_CAP_EDGES; run_k = cap_b; }
    seg_ptr[S] = (int)run_d;
    b_indptr[S] = (int)run_k;
    cnt->S = S; cnt->E = (int)run_d; cnt->B = (int)run_k;
    cnt->C = cnt->K = min(S, cap_k);                                // (k_nb_count adds the new sources)
    cnt->err = bad; cnt->iters = 0; cnt->all_one = 0; cnt->c = 0.0;
  }
}

}  // namespace
