// The source-numbering tail shared by the node-wise samplers (csrc/neighbor.hip, csrc/neighbor_w.hip, csrc/labor.hip,
// csrc/labor_is.hip): the kernels behind the one that wrote pos / dst / eid and marked the kept edges' sources in the |V|-bit bitmap.
//   k_nb_count   popcount per bitmap tile; the last workgroup (a ticket, k_md_pass's hand-over) scans the tile counts and writes K
//   k_nb_number  ordered numbering: new sources get kept_nid[S + rank] and kept_map; every bitmap word read here is left ZERO
//   k_nb_tail    src = kept_map[indices[pos]] (0 where a clamped K left the source without a number), unit weights
//   k_nb_clean   kept_map back to -1 at kept_nid[0 .. K); kept_nid[K .. cap_k) = 0 (capacity padding), node_prob = 1
//   k_nb_scan / k_nb_select: the head of the per-column draws (csrc/neighbor.hip; csrc/neighbor_w.hip selects over its own keys)
// Scratch layout of these samplers: [0, NB_HDR) tickets ([0] step ticket, [1] tile ticket), the bitmap (whole tiles), one count per tile.
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
    // a source that k_nb_number could not number (K clamped at cap_k) has no kept_map entry: its edges stand at source 0, a seed,
    // which exists wherever an edge does -- invalid like the rest of the flagged step, but inside [0, K) for whoever walks the block
    const int k = (unsigned)u < (unsigned)V ? kept_map[u] : -1;
    b_src[j] = k < 0 ? 0 : k;
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

// ---- the head of the per-column draws (csrc/neighbor.hip, and csrc/neighbor_w.hip with its staged race keys as `ov`) ----
// the edge's key: the CSC position in the node id's place, top 32 bits
__device__ __forceinline__ unsigned nb_key(unsigned long long mk, const unsigned* __restrict__ ov, int pos) {
  if (ov) return ov[pos];
  unsigned long long z = mk ^ (unsigned long long)(unsigned)pos;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (unsigned)(z >> 32);
}

__global__ void __launch_bounds__(NB_SCAN_TPB) k_nb_scan(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
                                                         int S_host, const int* __restrict__ S_dev, int cap_s, int fanout,
                                                         LayerCounts* cnt, int* __restrict__ seg_ptr, int* __restrict__ b_indptr,
                                                         int cap_b, int* __restrict__ kept_nid, int* __restrict__ kept_map, int cap_k) {
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
      if (i < cap_k) kept_nid[i] = nid;
      if ((unsigned)nid < (unsigned)V) {
        d = g_indptr[nid + 1] - g_indptr[nid];
        k = (fanout < 0 || d <= fanout) ? d : fanout;
        if (i < cap_k) kept_map[nid] = i;
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

__global__ void __launch_bounds__(NB_TPB) k_nb_select(const long long* __restrict__ g_indptr, const int* __restrict__ indices,
                                                      const int* __restrict__ g_eid, int V, const int* __restrict__ seeds,
                                                      const LayerCounts* __restrict__ cnt, int fanout,
                                                      const unsigned* __restrict__ ov, unsigned long long seed, long long* step_dev,
                                                      int layer, int bump_step, const int* __restrict__ kept_map,
                                                      const int* __restrict__ b_indptr, int* __restrict__ b_pos, int* __restrict__ b_dst,
                                                      int* __restrict__ b_eid, int cap_b, unsigned* bitmap, unsigned* ticket) {
  __shared__ int lb[256];
  __shared__ int sh[17];
  __shared__ unsigned sh_prefix;
  __shared__ int sh_need;
  const int tid = threadIdx.x;
  const int S = cnt->S;
  unsigned long long mk = 0;
  if (!ov) mk = nb_mdkey(seed, (unsigned long long)*step_dev, layer);
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int nid = seeds[s];
    if ((unsigned)nid >= (unsigned)V) continue;
    const long long a64 = g_indptr[nid];
    const int a = (int)a64, d = (int)(g_indptr[nid + 1] - a64);
    const int o = b_indptr[s];
    const bool all = fanout < 0 || d <= fanout;
    unsigned T = 0;                                                 // the k-th smallest key ...
    int r = 0;                                                      // ... and how many edges with that key are kept
    if (!all) {
      unsigned prefix = 0;
      int need = fanout;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        lb[tid] = 0;
        __syncthreads();
        for (int i = tid; i < d; i += NB_TPB) {
          const unsigned key = nb_key(mk, ov, a + i);
          if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&lb[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        const int n = lb[tid];
        int tot;
        const int ex = block_excl_scan(n, sh, &tot);
        if (ex < need && need <= ex + n) {                          // exactly one thread: the k-th smallest key has its digit here
          sh_prefix = prefix | ((unsigned)tid << shift);
          sh_need = need - ex;
        }
        __syncthreads();
        prefix = sh_prefix;
        need = sh_need;
      }
      T = prefix;
      r = need;
    }
    int run_below = 0, run_tie = 0;
    for (int base = 0; base < d; base += NB_TPB) {
      const int i = base + tid;
      bool take = all && i < d;
      int rank = i;
      if (!all) {
        int below = 0, tie = 0;
        if (i < d) {
          const unsigned key = nb_key(mk, ov, a + i);
          below = key < T ? 1 : 0;
          tie = key == T ? 1 : 0;
        }
        int tot;                                                    // both counts in one scan: at most 256 each per chunk
        const int ex = block_excl_scan(below | (tie << 16), sh, &tot);
        const int tb = run_tie + (ex >> 16);                        // equal keys at lower positions
        take = below || (tie && tb < r);
        rank = run_below + (ex & 0xffff) + min(tb, r);
        run_below += tot & 0xffff;
        run_tie += tot >> 16;
      }
      if (take && (long long)o + rank < (long long)cap_b) {
        const int j = o + rank, p = a + i;
        b_pos[j] = p;
        b_dst[j] = s;
        b_eid[j] = g_eid ? g_eid[p] : p;
        const int u = indices[p];
        if ((unsigned)u < (unsigned)V && kept_map[u] < 0) atomicOr(bitmap + (u >> 5), 1u << (u & 31));
      }
    }
  }
  if (!bump_step) return;
  // every workgroup has read the step when it takes its ticket; the last one bumps it and leaves the ticket zero
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *step_dev += 1;
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
