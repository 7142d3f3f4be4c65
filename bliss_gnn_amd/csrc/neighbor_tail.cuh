// The source-numbering tail shared by the node-wise samplers (csrc/neighbor.hip, csrc/labor.hip): the kernels behind the one that
// wrote pos / dst / eid and marked the kept edges' sources in the |V|-bit bitmap.
//   k_nb_count   popcount per bitmap tile; the last workgroup (a ticket, k_md_pass's hand-over) scans the tile counts and writes K
//   k_nb_number  ordered numbering: new sources get kept_nid[S + rank] and kept_map; every bitmap word read here is left ZERO
//   k_nb_tail    src = kept_map[indices[pos]], unit weights
//   k_nb_clean   kept_map back to -1 at kept_nid[0 .. K); kept_nid[K .. cap_k) = 0 (capacity padding), node_prob = 1
// Scratch layout of both samplers: [0, NB_HDR) tickets ([0] step ticket, [1] tile ticket), the bitmap (whole tiles), one count per tile.
#pragma once
#include "common.cuh"
#include "bliss_gnn.h"

namespace {

#define NB_TPB 256
#define NB_SCAN_TPB 1024
#define NB_TILE 1024          // bitmap words per tile: four per thread
#define NB_HDR 16             // scratch words in front of the bitmap: [0] step ticket, [1] tile ticket
#define NB_ONE_BF16 0x3f80

// (seed, step, layer) mixing   (= csrc/mn_draw.hip:md_key, oracle keyed_uniform)
__device__ __forceinline__ unsigned long long nb_mdkey(unsigned long long seed, unsigned long long step, int layer) {
  unsigned long long key = seed * 0x9E3779B97F4A7C15ull + step;
  key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
  key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
  key ^= key >> 31;
  return key ^ ((unsigned long long)((unsigned)layer & 0xffu) << 56);
}

// block-wide exclusive scan of one 64-bit value per thread (1024 threads); `sh` needs 17 words
__device__ __forceinline__ long long nb_scan64(long long v, long long* sh, long long* total) {
  const int lane = lane_id(), wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < BLISS_WAVE; d <<= 1) {
    const long long t = shfl_up_i64(inc, d);
    if (lane >= d) inc += t;
  }
  __syncthreads();
  if (lane == BLISS_WAVE - 1) sh[wid] = inc;
  __syncthreads();
  if (wid == 0) {
    const long long w = lane < nw ? sh[lane] : 0;
    long long winc = w;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const long long t = shfl_up_i64(winc, d);
      if (lane >= d) winc += t;
    }
    if (lane < nw) sh[lane] = winc - w;
    if (lane == nw - 1) sh[16] = winc;
  }
  __syncthreads();
  *total = sh[16];
  return sh[wid] + inc - v;
}

__device__ __forceinline__ int nb_popc4(uint4 w) { return __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w); }

__global__ void __launch_bounds__(NB_TPB) k_nb_count(const unsigned* __restrict__ bitmap, int n_tiles, LayerCounts* cnt, int cap_k,
                                                     int* tile_cnt, unsigned* ticket) {
  __shared__ int sh[17];
  __shared__ int sh_last;
  const int tid = threadIdx.x;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int c = nb_popc4(((const uint4*)bitmap)[(size_t)tile * NB_TPB + tid]);
    int tot;
    block_excl_scan(c, sh, &tot);
    if (tid == 0) __hip_atomic_store(tile_cnt + tile, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the tile counts are complete when every workgroup has passed here: stores drained, then a ticket (k_md_pass's hand-over)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    sh_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    if (sh_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!sh_last) return;
  // the last workgroup: counts read past this XCD's L2, replaced by their exclusive prefix (k_nb_number's tile offsets)
  long long run = 0;
  for (int base = 0; base < n_tiles; base += NB_TPB) {
    const int t = base + tid;
    const int v = t < n_tiles ? __hip_atomic_load(tile_cnt + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    int tot;
    const int ex = block_excl_scan(v, sh, &tot);
    if (t < n_tiles) tile_cnt[t] = (int)min(run + ex, (long long)INT32_MAX);
    run += tot;
  }
  if (tid == 0) {
    long long K = (long long)cnt->S + run;
    if (K > (long long)cap_k) { atomicOr(&cnt->err, BLISS_ERR_CAP_KEPT); K = cap_k; }   // clamp: results invalid but in bounds
    cnt->K = (int)K;
    cnt->C = (int)K;
  }
}

__global__ void __launch_bounds__(NB_TPB) k_nb_number(unsigned* bitmap, int n_tiles, const LayerCounts* __restrict__ cnt,
                                                      const int* __restrict__ tile_off, int cap_k, int* __restrict__ kept_nid,
                                                      int* __restrict__ kept_map) {
  __shared__ int sh[17];
  const int tid = threadIdx.x;
  const int S = cnt->S;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint4* wp = (uint4*)bitmap + (size_t)tile * NB_TPB + tid;
    const uint4 w = *wp;
    const int c = nb_popc4(w);
    int tot;
    const int ex = block_excl_scan(c, sh, &tot);
    if (!c) continue;
    long long id = (long long)S + tile_off[tile] + ex;
    const unsigned ws[4] = {w.x, w.y, w.z, w.w};
    const int nid0 = (tile * NB_TILE + tid * 4) * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned x = ws[q];
      while (x) {
        const int nid = nid0 + 32 * q + __ffs((int)x) - 1;
        x &= x - 1;
        if (id < (long long)cap_k) { kept_nid[id] = nid; kept_map[nid] = (int)id; }
        ++id;
      }
    }
    *wp = make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ void __launch_bounds__(NB_TPB) k_nb_tail(const int* __restrict__ indices, int V, const LayerCounts* __restrict__ cnt,
                                                    const int* __restrict__ b_pos, const int* __restrict__ kept_map,
                                                    int* __restrict__ b_src, bf16_t* __restrict__ b_w, bf16_t* __restrict__ b_q, int cap_b) {
  const int B = min(cnt->B, cap_b);
  for (int j = blockIdx.x * NB_TPB + threadIdx.x; j < B; j += gridDim.x * NB_TPB) {
    const int u = indices[b_pos[j]];
    b_src[j] = (unsigned)u < (unsigned)V ? kept_map[u] : -1;
    b_w[j] = NB_ONE_BF16;
    b_q[j] = NB_ONE_BF16;
  }
}

__global__ void __launch_bounds__(NB_TPB) k_nb_clean(const LayerCounts* __restrict__ cnt, int* __restrict__ kept_nid, int cap_k, int V,
                                                     int* __restrict__ kept_map, bf16_t* __restrict__ node_prob) {
  const int K = min(cnt->K, cap_k);
  for (int i = blockIdx.x * NB_TPB + threadIdx.x; i < cap_k; i += gridDim.x * NB_TPB) {
    if (i < K) {
      const int nid = kept_nid[i];
      if ((unsigned)nid < (unsigned)V) kept_map[nid] = -1;
    } else {
      kept_nid[i] = 0;                                  // capacity padding: a valid node id, so that padded feature gathers are harmless
    }
    if (node_prob) node_prob[i] = NB_ONE_BF16;
  }
}

static inline int nb_grid(long long n, int per, int cap) {
  long long g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
static inline long long nb_bitmap_words(int num_nodes) {
  const long long w = ((long long)num_nodes + 31) / 32;
  return (w + NB_TILE - 1) / NB_TILE * NB_TILE;
}

}  // namespace
