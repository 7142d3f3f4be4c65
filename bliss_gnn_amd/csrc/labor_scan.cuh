// What the LABOR samplers share (csrc/labor.hip, csrc/labor_is.hip, csrc/labor_w.hip) in front of the source-numbering tail: the
// per-source key, the clamped seed count, the one-workgroup scan behind their counting kernels; for the two with per-edge
// probabilities also a seed's column, the column-size paths of their scale solves and the one-rounding fp64 -> bf16 of the weights.
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

#define LI_ONE (1ull << 32)
#define LI_WAVE_D 256         // a wave solves a column up to this degree from registers: four positions per lane
#define LI_STAGE 2048         // the workgroup stages a column's importances in LDS up to this degree
#define LI_COLS 4             // columns per workgroup and trip in the wave-per-column kernels (= waves per workgroup)

// column s: first CSC position and degree; an empty column for a seed id outside [0, V)
__device__ __forceinline__ void li_column(const long long* __restrict__ g_indptr, const int* __restrict__ seeds, int V, int s, int* a,
                                          int* d) {
  const int nid = seeds[s];
  *a = 0; *d = 0;
  if ((unsigned)nid < (unsigned)V) {
    const long long a64 = g_indptr[nid];
    *a = (int)a64; *d = (int)(g_indptr[nid + 1] - a64);
  }
}
__device__ __forceinline__ bool li_whole(int fanout, int d) { return fanout < 0 || d <= fanout; }
// fp64 -> bf16, ONE rounding to nearest even (positive normal values in bf16's range: the weights)
__device__ __forceinline__ bf16_t li_d2bf(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  int e = (int)((b >> 52) & 0x7ffull) - 1023 + 127;
  const unsigned long long m = b & ((1ull << 52) - 1ull), rem = m & ((1ull << 45) - 1ull), half = 1ull << 44;
  unsigned q = (unsigned)(m >> 45);
  if (rem > half || (rem == half && (q & 1u))) q += 1u;
  if (q >= 128u) { q = 0u; e += 1; }
  return (bf16_t)(((unsigned)e << 7) | q);
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
