// The LABOR-i sampler on the device (fit.ImportanceLaborSampler): csrc/labor.hip's keyed per-source draw with
// a per-EDGE inclusion probability p = (c_s * pi_u) >> 32 in the place of the per-column threshold -- pi_u the importance of the
// source, found by I fixed-point iterations, c_s the column's scale, found by bisection.  Unsigned integers up to the weights; the
// rule is normative, tests/labor_is_ref.py restates it on the CPU (ONE = 2^32):
//
//   column s, CSC positions [a, b), d = b - a: WHOLE if fanout < 0 or d <= fanout (every edge kept, no key computed)
//   pi^(0)_u = ONE;  c_s(pi) = the largest c in [0, ONE - 1] with sum_pos (c * pi_{indices[pos]}) >> 32 <= fanout * ONE
//   pi^(i+1)_u = max(1, max over the frontier edges u -> s of P),  P = ONE if s is whole, else (c_s(pi^(i)) * pi^(i)_u) >> 32
//   the edge at pos is kept iff (uint64)key(u) < p_pos = (c_s(pi^(I)) * pi^(I)_u) >> 32      (key, block, sources: csrc/labor.hip's)
//   q_ij = bf16(fp32(p) * 2^-32);  edge_weights = bf16((ONE / p_e) * k_s / sum_{kept e'} ONE / p_e') in fp64;  both 1 in whole columns
//
// An importance is stored as pi - 1 in a uint32 (ONE fits; the idle value 0 is atomicMax's identity and the rule's floor pi = 1) in
// two |V|-word buffers; pi^(0) is implicit (the first scale is the closed form (fanout << 32) / d and the first push writes it).
// bliss_labor_is_layer = 8 launches for I = 0 and 2 I + 9 for I >= 1, on one stream, no host round trip:
//   k_li_push    (I times) a wave per column: atomicMax(next[u], P - 1) per frontier edge; no output depends on the landing order
//   k_li_solve   (I times) c_s of the new importances: a wave per column of degree <= 256 (the values in registers), the workgroup
//                per larger column (the values staged in LDS up to LI_STAGE positions, streamed above); 32 bisection steps, each a
//                reduction of uint64 partial sums.  It also stores the idle value over the frontier into the buffer no longer needed
//   k_li_count, k_lb_scan, k_li_write    labor.hip's three with p_pos in thr's place; the write pass leaves p_e per kept edge
//   k_nb_count, k_nb_number, k_nb_tail, k_nb_clean   the neighbor sampler's tail (csrc/neighbor_tail.cuh), as it stands
//   k_li_weights a workgroup per column: the fp64 sum of ONE / p_e in a fixed order, then edge_weights and q_ij
//   k_li_clear   (I >= 1) the live importance buffer back to idle over the frontier
// Every word a replay relies on (tickets, bitmap, kept_map, both importance buffers) is back at its idle value when the call ends,
// also after a flagged capacity overflow and for a seed id out of range (an empty column); everything else is rewritten by every
// call before it is read.
#include "labor_scan.cuh"

namespace {

__device__ __forceinline__ unsigned long long li_closed(int fanout, int d) {
  return ((unsigned long long)(unsigned)fanout << 32) / (unsigned long long)d;
}
// the scale of a non-whole column and the inclusion probability of one of its edges (pi == NULL: pi^(0), the closed form)
__device__ __forceinline__ unsigned long long li_scale(const unsigned* __restrict__ pi, const unsigned* __restrict__ c_arr, int s,
                                                       int fanout, int d) {
  return pi ? (unsigned long long)c_arr[s] : li_closed(fanout, d);
}
__device__ __forceinline__ unsigned long long li_p(const unsigned* __restrict__ pi, unsigned long long c, int u) {
  return pi ? (c * ((unsigned long long)pi[u] + 1ull)) >> 32 : c;
}

__global__ void __launch_bounds__(NB_TPB) k_li_push(const long long* __restrict__ g_indptr, const int* __restrict__ indices, int V,
                                                    const int* __restrict__ seeds, int S_host, const int* __restrict__ S_dev,
                                                    int cap_s, int fanout, const unsigned* __restrict__ cur,
                                                    const unsigned* __restrict__ c_arr, unsigned* next) {
  const int lane = lane_id(), wid = threadIdx.x >> 6;
  const int S = lb_seed_count(S_host, S_dev, cap_s);
  for (int s = blockIdx.x * LI_COLS + wid; s < S; s += gridDim.x * LI_COLS) {      // (uniform over the wave)
    int a, d;
    li_column(g_indptr, seeds, V, s, &a, &d);
    const bool whole = li_whole(fanout, d);
    const unsigned long long c = whole ? 0ull : li_scale(cur, c_arr, s, fanout, d);
    for (int i = lane; i < d; i += BLISS_WAVE) {
      const int u = indices[a + i];
      if ((unsigned)u >= (unsigned)V) continue;
      const unsigned long long P = whole ? LI_ONE : li_p(cur, c, u);
      atomicMax(next + u, (unsigned)((P ? P : 1ull) - 1ull));
    }
  }
}

__global__ void __launch_bounds__(NB_TPB) k_li_solve(const long long* __restrict__ g_indptr, const int* __restrict__ indices, int V,
                                                     const int* __restrict__ seeds, int S_host, const int* __restrict__ S_dev,
                                                     int cap_s, int fanout, const unsigned* __restrict__ pi, unsigned* old,
                                                     unsigned* __restrict__ c_arr) {
  __shared__ unsigned long long sh_pv[LI_STAGE];                      // pi per staged position; 0 = no term
  __shared__ unsigned long long sh_red[NB_TPB / BLISS_WAVE];
  const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
  const int S = lb_seed_count(S_host, S_dev, cap_s);
  const unsigned long long lim = (unsigned long long)(unsigned)(fanout < 0 ? 0 : fanout) << 32;
  for (int s0 = blockIdx.x * LI_COLS; s0 < S; s0 += gridDim.x * LI_COLS) {
    // a wave per column: the buffer no longer needed back to idle, and the columns of degree <= LI_WAVE_D solved from registers
    const int s = s0 + wid;
    if (s < S) {                                                       // (uniform over the wave)
      int a, d;
      li_column(g_indptr, seeds, V, s, &a, &d);
      if (old) {
        for (int i = lane; i < d; i += BLISS_WAVE) {
          const int u = indices[a + i];
          if ((unsigned)u < (unsigned)V) old[u] = 0u;
        }
      }
      if (!li_whole(fanout, d) && d <= LI_WAVE_D) {
        unsigned long long pv[LI_WAVE_D / BLISS_WAVE];
#pragma unroll
        for (int q = 0; q < LI_WAVE_D / BLISS_WAVE; ++q) {
          const int i = lane + BLISS_WAVE * q;
          pv[q] = 0ull;                                                // (a source id outside [0, V) is no term)
          if (i < d) {
            const int u = indices[a + i];
            if ((unsigned)u < (unsigned)V) pv[q] = (unsigned long long)pi[u] + 1ull;
          }
        }
        unsigned long long c = 0ull;
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned long long t = c | (1ull << bit);
          unsigned long long sum = 0ull;
#pragma unroll
          for (int q = 0; q < LI_WAVE_D / BLISS_WAVE; ++q) sum += (t * pv[q]) >> 32;
          if ((unsigned long long)wave_total_i64((long long)sum) <= lim) c = t;
        }
        if (lane == 0) c_arr[s] = (unsigned)c;
      }
    }
    // the workgroup per larger column (every thread takes the same path)
    for (int w = 0; w < LI_COLS && s0 + w < S; ++w) {
      int a, d;
      li_column(g_indptr, seeds, V, s0 + w, &a, &d);
      if (li_whole(fanout, d) || d <= LI_WAVE_D) continue;
      const bool staged = d <= LI_STAGE;
      __syncthreads();                                                 // (sh_pv and sh_red of the previous column are done with)
      if (staged) {
        for (int i = tid; i < d; i += NB_TPB) {
          const int u = indices[a + i];
          sh_pv[i] = (unsigned)u < (unsigned)V ? (unsigned long long)pi[u] + 1ull : 0ull;
        }
        __syncthreads();
      }
      unsigned long long c = 0ull;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned long long t = c | (1ull << bit);
        unsigned long long sum = 0ull;
        if (staged) {
          for (int i = tid; i < d; i += NB_TPB) sum += (t * sh_pv[i]) >> 32;
        } else {
          for (int i = tid; i < d; i += NB_TPB) {
            const int u = indices[a + i];
            if ((unsigned)u < (unsigned)V) sum += (t * ((unsigned long long)pi[u] + 1ull)) >> 32;
          }
        }
        const unsigned long long wt = (unsigned long long)wave_total_i64((long long)sum);
        if (lane == 0) sh_red[wid] = wt;
        __syncthreads();
        unsigned long long tot = 0ull;
#pragma unroll
        for (int k = 0; k < NB_TPB / BLISS_WAVE; ++k) tot += sh_red[k];
        __syncthreads();
        if (tot <= lim) c = t;
      }
      if (tid == 0) c_arr[s0 + w] = (unsigned)c;
    }
  }
}

// is the edge at CSC position pos kept, and with which probability?  (a source id outside [0, V) is dropped unread)
__device__ __forceinline__ bool li_take(unsigned long long mk, const unsigned* __restrict__ ov, const int* __restrict__ indices, int V,
                                        int pos, const unsigned* __restrict__ pi, unsigned long long c, unsigned long long* p) {
  const int u = indices[pos];
  if ((unsigned)u >= (unsigned)V) return false;
  *p = li_p(pi, c, u);
  return (unsigned long long)lb_key(mk, ov, u) < *p;
}

__global__ void __launch_bounds__(NB_TPB) k_li_count(const long long* __restrict__ g_indptr, const int* __restrict__ indices, int V,
                                                     const int* __restrict__ seeds, int S_host, const int* __restrict__ S_dev,
                                                     int cap_s, int fanout, const unsigned* __restrict__ ov, unsigned long long seed,
                                                     const long long* __restrict__ step_dev, int layer,
                                                     const unsigned* __restrict__ pi, const unsigned* __restrict__ c_arr,
                                                     int* __restrict__ kept_nid, int* __restrict__ kept_map, int cap_k,
                                                     int* __restrict__ col_cnt) {
  __shared__ int sh[17];
  const int tid = threadIdx.x;
  const int S = lb_seed_count(S_host, S_dev, cap_s);
  unsigned long long mk = 0;
  if (!ov) mk = nb_mdkey(seed, (unsigned long long)*step_dev, layer);
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int nid = seeds[s];
    const bool valid = (unsigned)nid < (unsigned)V;                 // (k_lb_scan flags a seed id out of range: an empty column)
    if (tid == 0 && s < cap_k) {
      kept_nid[s] = nid;
      if (valid) kept_map[nid] = s;
    }
    int a, d, tot = 0;
    li_column(g_indptr, seeds, V, s, &a, &d);
    if (li_whole(fanout, d)) {
      tot = d;
    } else {
      const unsigned long long c = li_scale(pi, c_arr, s, fanout, d);
      int k = 0;
      unsigned long long p;
      for (int i = tid; i < d; i += NB_TPB) k += li_take(mk, ov, indices, V, a + i, pi, c, &p) ? 1 : 0;
      block_excl_scan(k, sh, &tot);
    }
    if (tid == 0) col_cnt[s] = tot;
  }
}

__global__ void __launch_bounds__(NB_TPB) k_li_write(const long long* __restrict__ g_indptr, const int* __restrict__ indices,
                                                     const int* __restrict__ g_eid, int V, const int* __restrict__ seeds,
                                                     const LayerCounts* __restrict__ cnt, int fanout,
                                                     const unsigned* __restrict__ ov, unsigned long long seed, long long* step_dev,
                                                     int layer, int bump_step, const unsigned* __restrict__ pi,
                                                     const unsigned* __restrict__ c_arr, const int* __restrict__ kept_map,
                                                     const int* __restrict__ b_indptr, int* __restrict__ b_pos, int* __restrict__ b_dst,
                                                     int* __restrict__ b_eid, unsigned* __restrict__ b_pe, int cap_b, unsigned* bitmap,
                                                     unsigned* ticket) {
  __shared__ int sh[17];
  const int tid = threadIdx.x;
  const int S = cnt->S;
  unsigned long long mk = 0;
  if (!ov) mk = nb_mdkey(seed, (unsigned long long)*step_dev, layer);
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    int a, d;
    li_column(g_indptr, seeds, V, s, &a, &d);
    if (d == 0) continue;
    const int o = b_indptr[s];
    const bool all = li_whole(fanout, d);
    const unsigned long long c = all ? 0ull : li_scale(pi, c_arr, s, fanout, d);
    int run = 0;
    for (int base = 0; base < d; base += NB_TPB) {
      const int i = base + tid;
      bool take = all && i < d;
      int rank = i;
      unsigned long long p = 0ull;                                  // (p_e = 0 marks an edge of a whole column: a kept edge has p >= 1)
      if (!all) {
        take = i < d && li_take(mk, ov, indices, V, a + i, pi, c, &p);
        int tot;
        rank = run + block_excl_scan(take ? 1 : 0, sh, &tot);
        run += tot;
      }
      if (take && (long long)o + rank < (long long)cap_b) {
        const int j = o + rank, pos = a + i;
        b_pos[j] = pos;
        b_dst[j] = s;
        b_eid[j] = g_eid ? g_eid[pos] : pos;
        b_pe[j] = (unsigned)p;
        const int u = indices[pos];
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

__global__ void __launch_bounds__(NB_TPB) k_li_weights(const LayerCounts* __restrict__ cnt, const int* __restrict__ b_indptr,
                                                       const unsigned* __restrict__ b_pe, bf16_t* __restrict__ b_w,
                                                       bf16_t* __restrict__ b_q, int cap_b) {
  __shared__ double sh[NB_TPB / BLISS_WAVE];
  const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
  const int S = cnt->S;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int o = min(b_indptr[s], cap_b), e = min(b_indptr[s + 1], cap_b);
    if (e <= o) continue;
    if (b_pe[o] == 0u) continue;                                    // a whole column: k_nb_tail's unit weights stand
    // the sum in a fixed order: a strided partial per thread, a shuffle tree per wave, the waves in order
    double acc = 0.0;
    for (int j = o + tid; j < e; j += NB_TPB) acc += 4294967296.0 / (double)b_pe[j];
#pragma unroll
    for (int dd = BLISS_WAVE / 2; dd >= 1; dd >>= 1) acc += __shfl_down(acc, dd);
    __syncthreads();                                                // (sh of the previous column is done with)
    if (lane == 0) sh[wid] = acc;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < NB_TPB / BLISS_WAVE; ++k) tot += sh[k];
    const double ks = (double)(e - o);
    for (int j = o + tid; j < e; j += NB_TPB) {
      const unsigned p = b_pe[j];
      b_w[j] = li_d2bf((4294967296.0 / (double)p) * ks / tot);
      b_q[j] = f2bf((float)p * 2.3283064365386963e-10f);            // uint32 -> fp32 to nearest even, * 2^-32 exact
    }
  }
}

__global__ void __launch_bounds__(NB_TPB) k_li_clear(const long long* __restrict__ g_indptr, const int* __restrict__ indices, int V,
                                                     const int* __restrict__ seeds, int S_host, const int* __restrict__ S_dev,
                                                     int cap_s, unsigned* pi) {
  const int lane = lane_id(), wid = threadIdx.x >> 6;
  const int S = lb_seed_count(S_host, S_dev, cap_s);
  for (int s = blockIdx.x * LI_COLS + wid; s < S; s += gridDim.x * LI_COLS) {
    int a, d;
    li_column(g_indptr, seeds, V, s, &a, &d);
    for (int i = lane; i < d; i += BLISS_WAVE) {
      const int u = indices[a + i];
      if ((unsigned)u < (unsigned)V) pi[u] = 0u;
    }
  }
}

}  // namespace

extern "C" {

int64_t bliss_labor_is_scratch_bytes(int32_t num_nodes, int32_t cap_s, int32_t cap_b) {
  if (num_nodes <= 0 || cap_s <= 0 || cap_b < 0) return BLISS_EINVAL;
  const long long words = nb_bitmap_words(num_nodes);
  return (int64_t)(((NB_HDR + words + words / NB_TILE + 2ll * num_nodes + 2ll * cap_s + (long long)cap_b) * 4 + 15) & ~15ll);
}

int bliss_labor_is_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                         int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer,
                         int bump_step, int layer_dependency, int32_t iterations, const bliss_layer_ws_t* ws,
                         const bliss_block_out_t* out, void* scratch, void* stream) {
  if (!g || !seeds || !ws || !out || !scratch || cap_s <= 0 || fanout == 0 || iterations < 0 || iterations > 8) return BLISS_EINVAL;
  if (!g->indptr || !g->indices || g->num_nodes <= 0 || g->num_edges < 0 || g->num_edges > (int64_t)INT32_MAX) return BLISS_EINVAL;
  if (n_seeds < 0 && !n_seeds_dev) return BLISS_EINVAL;
  if (!ws->counts || !ws->seg_ptr || !ws->kept_nid || !ws->kept_map || ws->cap_k <= 0) return BLISS_EINVAL;
  if (!out->indptr || !out->src || !out->dst || !out->pos || !out->eid || !out->edge_weights || !out->q_ij || out->cap_b < 0)
    return BLISS_EINVAL;
  if (((uintptr_t)scratch & 15) || ((!keys_override || bump_step) && !step_dev)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  LayerCounts* cnt = (LayerCounts*)ws->counts;
  const long long* indptr = (const long long*)g->indptr;
  const int V = g->num_nodes, cap_k = ws->cap_k, cap_b = out->cap_b;
  const int key_layer = layer_dependency ? 0 : layer;               // the same variate per vertex in all layers of a step
  // scratch: tickets, bitmap, tile counts, the two importance buffers (all that must be idle first: their place depends on
  // num_nodes alone), then c_s counts, c_s scales and p_e
  unsigned* scr = (unsigned*)scratch;
  unsigned* bitmap = scr + NB_HDR;
  const long long words = nb_bitmap_words(V);
  const int n_tiles = (int)(words / NB_TILE);
  int* tile_cnt = (int*)(bitmap + words);
  unsigned* pi_a = (unsigned*)(tile_cnt + n_tiles);
  unsigned* pi_b = pi_a + V;
  int* col_cnt = (int*)(pi_b + V);
  unsigned* c_arr = (unsigned*)(col_cnt + cap_s);
  unsigned* b_pe = c_arr + cap_s;
  const int gt = nb_grid(n_tiles, 1, 1024), gs = nb_grid(cap_s, 1, 2048), gw = nb_grid(cap_s, LI_COLS, 1024);
  const unsigned* pi = nullptr;                                     // pi^(0) is implicit
  for (int i = 0; i < iterations && fanout > 0; ++i) {              // (fanout < 0: every column is whole, nothing reads pi)
    unsigned* next = pi == pi_a ? pi_b : pi_a;
    k_li_push<<<gw, NB_TPB, 0, st>>>(indptr, g->indices, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, pi, c_arr, next);
    k_li_solve<<<gw, NB_TPB, 0, st>>>(indptr, g->indices, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, next, (unsigned*)pi, c_arr);
    pi = next;
  }
  k_li_count<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, keys_override, seed,
                                    (const long long*)step_dev, key_layer, pi, c_arr, ws->kept_nid, ws->kept_map, cap_k, col_cnt);
  k_lb_scan<<<1, NB_SCAN_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, col_cnt, cnt, ws->seg_ptr, out->indptr, cap_b,
                                       cap_k);
  k_li_write<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, g->eid, V, seeds, cnt, fanout, keys_override, seed, (long long*)step_dev,
                                    key_layer, bump_step, pi, c_arr, ws->kept_map, out->indptr, out->pos, out->dst, out->eid, b_pe,
                                    cap_b, bitmap, scr);
  k_nb_count<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, cap_k, tile_cnt, scr + 1);
  k_nb_number<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, tile_cnt, cap_k, ws->kept_nid, ws->kept_map);
  k_nb_tail<<<nb_grid(cap_b, NB_TPB, 2048), NB_TPB, 0, st>>>(g->indices, V, cnt, out->pos, ws->kept_map, out->src,
                                                             (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  k_nb_clean<<<nb_grid(cap_k, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, ws->kept_nid, cap_k, V, ws->kept_map,
                                                              (bf16_t*)ws->node_prob);
  k_li_weights<<<gs, NB_TPB, 0, st>>>(cnt, out->indptr, b_pe, (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  if (pi) k_li_clear<<<gw, NB_TPB, 0, st>>>(indptr, g->indices, V, seeds, n_seeds, n_seeds_dev, cap_s, (unsigned*)pi);
  return (int)hipGetLastError();
}

}  // extern "C"
