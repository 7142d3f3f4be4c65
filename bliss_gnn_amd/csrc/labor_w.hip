// The WEIGHTED LABOR sampler on the device (fit.WeightedLaborSampler and fit.BanditLaborSampler): csrc/labor.hip's
// keyed per-source draw with a per-EDGE inclusion probability p_pos = min(ONE - 1, (c_s * a_pos) >> 24) in the place of the per-column
// threshold -- a_pos the edge probability q_pos as an integer relative to the column's largest one, c_s the column's scale, found by
// bisection.  Unsigned integers from the bf16 bits of q up to the weights; the rule is normative, tests/wlabor_ref.py restates it
// on the CPU (ONE = 2^32):
//
//   q_pos   = prob_pos[pos] (raw mode, bf16, unnormalised), or eta / n_i + (1 - eta) * w_pos / sum_col(w) with edge_q's roundings
//             (EXP3 mode: the column sum exact in block-floating fixed point, rounded once to bf16; csrc/neighbor_w.hip's q)
//   column s, CSC positions [a, b), d = b - a: WHOLE if fanout < 0 or d <= fanout (every edge kept, no key computed, unit weights)
//   an edge is VALID iff q_pos is positive and finite; from its bf16 bits (exponent field E, mantissa M): m = E ? 128 + M : M,
//             e = max(E, 1); e_max = the largest e over the column's valid edges
//   a_pos   = (m << 24) >> (e_max - e), 0 when the shift is >= 32 and for an invalid edge (so a_pos < ONE; no division, no rounding)
//   p_pos(c) = min(ONE - 1, (c * a_pos) >> 24) in 64 bits;  c_s = the largest c in [0, ONE - 1] with sum_pos p_pos(c) <= fanout * ONE
//             (32 bisection steps from bit 31 down).  A column with fewer than `fanout` edges of comparable weight ends at
//             c_s = ONE - 1 and keeps fewer than `fanout` edges in expectation
//   the edge at pos is kept iff (uint64)key(u) < p_pos(c_s), u = indices[pos]  (key, block, sources: csrc/labor.hip's); an edge with
//             a_pos = 0 is never kept in a non-whole column (no filler rule, unlike csrc/neighbor_w.hip)
//   q_ij = q_pos for every kept edge (whole columns too);  p_ij = bf16(fp32(p_pos) * 2^-32), 1 in whole columns;  node_prob = 1
//   edge_weights = bf16((ONE / p_e) * k_s / sum_{kept e'} ONE / p_e') in fp64 (csrc/labor_is.hip's order of summation), 1 in whole columns
//
// bliss_wlabor_layer = 9 launches in raw mode and 10 in EXP3 mode, on one stream, no host round trip:
//   k_wl_coef    (EXP3 mode) a workgroup per column: the per-seed (bf16 sum, eta / n) record, as csrc/neighbor_w.hip:k_wn_keys writes it
//   k_wl_solve   e_max and c_s per non-whole column, csrc/labor_is.hip:k_li_solve's three paths: a wave per column of degree <= 256
//                (the a_pos in registers), the workgroup per larger column (the a_pos staged in LDS up to LI_STAGE positions,
//                recomputed from q above); 32 bisection steps, each a reduction of uint64 partial sums.  A hub column is not split
//   k_wl_count, k_lb_scan, k_wl_write    labor.hip's three with p_pos in thr's place; the write pass leaves p_e per kept edge
//                (0 marks an edge of a whole column: a kept edge of another column has p >= 1)
//   k_nb_count, k_nb_number, k_nb_tail, k_nb_clean   the neighbor sampler's tail (csrc/neighbor_tail.cuh), as it stands
//   k_wl_weights a workgroup per column: q_ij and p_ij, the fp64 sum of ONE / p_e in a fixed order, then edge_weights
// Every word a replay relies on (tickets, the pending-error word, bitmap, kept_map) is back at its idle value when the call ends,
// also after a flagged capacity overflow and for a seed id out of range (an empty column); everything else is rewritten by every
// call before it is read.
#include "labor_scan.cuh"
#include "edge_q.cuh"

namespace {

#define WL_ERR_WORD 2         // scratch header word: error bits of k_wl_coef, handed to the counts record behind k_lb_scan

// e of a valid edge probability, 0 (the maximum's identity) of any other
__device__ __forceinline__ int wl_e(bf16_t q) {
  const int E = (q >> 7) & 0xff;
  if ((q & 0x8000u) || E == 0xff || (q & 0x7fffu) == 0u) return 0;
  return E ? E : 1;
}
// a_pos: q's significand at the scale of the column's largest exponent
__device__ __forceinline__ unsigned wl_a(bf16_t q, int emax) {
  const int e = wl_e(q);
  if (e == 0) return 0u;
  const unsigned E = (q >> 7) & 0xffu, M = q & 0x7fu;
  const unsigned m = E ? 128u + M : M;
  const int sh = emax - e;
  return sh >= 32 ? 0u : (m << 24) >> sh;
}
__device__ __forceinline__ unsigned long long wl_p(unsigned long long c, unsigned a) {
  const unsigned long long p = (c * (unsigned long long)a) >> 24;
  return p < LI_ONE - 1ull ? p : LI_ONE - 1ull;
}

__global__ void __launch_bounds__(NB_TPB) k_wl_coef(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
                                                    int S_host, const int* __restrict__ S_dev, int cap_s,
                                                    const bf16_t* __restrict__ prob, float eta_f, uint2* __restrict__ coef,
                                                    unsigned* err_word) {
  __shared__ long long sh[NB_TPB / BLISS_WAVE];
  const int S = lb_seed_count(S_host, S_dev, cap_s);
  int bad = 0;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    int a, d;
    li_column(g_indptr, seeds, V, s, &a, &d);
    if (d == 0) continue;
    const uint2 cf = wn_col_record<NB_TPB>(prob, a, d, eta_f, sh, &bad);
    if (threadIdx.x == 0) coef[s] = cf;
  }
  if (bad) atomicOr(err_word, (unsigned)bad);
}

__global__ void __launch_bounds__(NB_TPB) k_wl_solve(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
                                                     int S_host, const int* __restrict__ S_dev, int cap_s, int fanout, int mode,
                                                     const bf16_t* __restrict__ prob, float ome_f, const uint2* __restrict__ coef,
                                                     uint2* __restrict__ sc) {
  __shared__ unsigned sh_a[LI_STAGE];                                 // q's bits, then a_pos, per staged position
  __shared__ unsigned long long sh_red[NB_TPB / BLISS_WAVE];
  const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
  const int S = lb_seed_count(S_host, S_dev, cap_s);
  const unsigned long long lim = (unsigned long long)(unsigned)(fanout < 0 ? 0 : fanout) << 32;
  for (int s0 = blockIdx.x * LI_COLS; s0 < S; s0 += gridDim.x * LI_COLS) {
    // a wave per column: the columns of degree <= LI_WAVE_D solved from registers
    const int s = s0 + wid;
    if (s < S) {                                                       // (uniform over the wave)
      int a, d;
      li_column(g_indptr, seeds, V, s, &a, &d);
      if (!li_whole(fanout, d) && d <= LI_WAVE_D) {
        const uint2 cf = mode == BLISS_WN_EXP3 ? coef[s] : make_uint2(0u, 0u);
        bf16_t qv[LI_WAVE_D / BLISS_WAVE];
        int em = 0;
#pragma unroll
        for (int q = 0; q < LI_WAVE_D / BLISS_WAVE; ++q) {
          const int i = lane + BLISS_WAVE * q;
          qv[q] = i < d ? wn_q(mode, prob, a + i, cf, ome_f) : (bf16_t)0;      // (0: not valid, no term)
          em = max(em, wl_e(qv[q]));
        }
        em = wave_max_u31(em);
        unsigned av[LI_WAVE_D / BLISS_WAVE];
#pragma unroll
        for (int q = 0; q < LI_WAVE_D / BLISS_WAVE; ++q) av[q] = wl_a(qv[q], em);
        unsigned long long c = 0ull;
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned long long t = c | (1ull << bit);
          unsigned long long sum = 0ull;
#pragma unroll
          for (int q = 0; q < LI_WAVE_D / BLISS_WAVE; ++q) sum += wl_p(t, av[q]);
          if ((unsigned long long)wave_total_i64((long long)sum) <= lim) c = t;
        }
        if (lane == 0) sc[s] = make_uint2((unsigned)c, (unsigned)em);
      }
    }
    // the workgroup per larger column (every thread takes the same path)
    for (int w = 0; w < LI_COLS && s0 + w < S; ++w) {
      int a, d;
      li_column(g_indptr, seeds, V, s0 + w, &a, &d);
      if (li_whole(fanout, d) || d <= LI_WAVE_D) continue;
      const uint2 cf = mode == BLISS_WN_EXP3 ? coef[s0 + w] : make_uint2(0u, 0u);
      const bool staged = d <= LI_STAGE;
      int em = 0;
      for (int i = tid; i < d; i += NB_TPB) {
        const bf16_t q = wn_q(mode, prob, a + i, cf, ome_f);
        if (staged) sh_a[i] = q;                                       // (a thread reads back only what it stored itself)
        em = max(em, wl_e(q));
      }
      em = wn_block_max_u31<NB_TPB>(em, (long long*)sh_red);
      if (staged) {
        for (int i = tid; i < d; i += NB_TPB) sh_a[i] = wl_a((bf16_t)sh_a[i], em);
      }
      __syncthreads();                                                 // (sh_red is free again)
      unsigned long long c = 0ull;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned long long t = c | (1ull << bit);
        unsigned long long sum = 0ull;
        if (staged) {
          for (int i = tid; i < d; i += NB_TPB) sum += wl_p(t, sh_a[i]);
        } else {
          for (int i = tid; i < d; i += NB_TPB) sum += wl_p(t, wl_a(wn_q(mode, prob, a + i, cf, ome_f), em));
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
      if (tid == 0) sc[s0 + w] = make_uint2((unsigned)c, (unsigned)em);
    }
  }
}

// is the edge at CSC position pos kept, and with which probability?  (a source id outside [0, V) is dropped unread)
__device__ __forceinline__ bool wl_take(unsigned long long mk, const unsigned* __restrict__ ov, const int* __restrict__ indices, int V,
                                        int pos, int mode, const bf16_t* __restrict__ prob, uint2 cf, float ome_f, uint2 ce,
                                        unsigned long long* p) {
  const int u = indices[pos];
  if ((unsigned)u >= (unsigned)V) return false;
  *p = wl_p((unsigned long long)ce.x, wl_a(wn_q(mode, prob, pos, cf, ome_f), (int)ce.y));
  return (unsigned long long)lb_key(mk, ov, u) < *p;
}

__global__ void __launch_bounds__(NB_TPB) k_wl_count(const long long* __restrict__ g_indptr, const int* __restrict__ indices, int V,
                                                     const int* __restrict__ seeds, int S_host, const int* __restrict__ S_dev,
                                                     int cap_s, int fanout, const unsigned* __restrict__ ov, unsigned long long seed,
                                                     const long long* __restrict__ step_dev, int layer, int mode,
                                                     const bf16_t* __restrict__ prob, float ome_f, const uint2* __restrict__ coef,
                                                     const uint2* __restrict__ sc, int* __restrict__ kept_nid,
                                                     int* __restrict__ kept_map, int cap_k, int* __restrict__ col_cnt) {
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
      const uint2 cf = mode == BLISS_WN_EXP3 ? coef[s] : make_uint2(0u, 0u);
      const uint2 ce = sc[s];
      int k = 0;
      unsigned long long p;
      for (int i = tid; i < d; i += NB_TPB) k += wl_take(mk, ov, indices, V, a + i, mode, prob, cf, ome_f, ce, &p) ? 1 : 0;
      block_excl_scan(k, sh, &tot);
    }
    if (tid == 0) col_cnt[s] = tot;
  }
}

__global__ void __launch_bounds__(NB_TPB) k_wl_write(const long long* __restrict__ g_indptr, const int* __restrict__ indices,
                                                     const int* __restrict__ g_eid, int V, const int* __restrict__ seeds,
                                                     const LayerCounts* __restrict__ cnt, int fanout,
                                                     const unsigned* __restrict__ ov, unsigned long long seed, long long* step_dev,
                                                     int layer, int bump_step, int mode, const bf16_t* __restrict__ prob, float ome_f,
                                                     const uint2* __restrict__ coef, const uint2* __restrict__ sc,
                                                     const int* __restrict__ kept_map, const int* __restrict__ b_indptr,
                                                     int* __restrict__ b_pos, int* __restrict__ b_dst, int* __restrict__ b_eid,
                                                     unsigned* __restrict__ b_pe, int cap_b, unsigned* bitmap, unsigned* ticket) {
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
    const uint2 cf = !all && mode == BLISS_WN_EXP3 ? coef[s] : make_uint2(0u, 0u);
    const uint2 ce = all ? make_uint2(0u, 0u) : sc[s];
    int run = 0;
    for (int base = 0; base < d; base += NB_TPB) {
      const int i = base + tid;
      bool take = all && i < d;
      int rank = i;
      unsigned long long p = 0ull;                                  // (p_e = 0 marks an edge of a whole column: a kept edge has p >= 1)
      if (!all) {
        take = i < d && wl_take(mk, ov, indices, V, a + i, mode, prob, cf, ome_f, ce, &p);
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

__global__ void __launch_bounds__(NB_TPB) k_wl_weights(LayerCounts* cnt, int mode, const bf16_t* __restrict__ prob, float ome_f,
                                                       const uint2* __restrict__ coef, const int* __restrict__ b_indptr,
                                                       const int* __restrict__ b_pos, const unsigned* __restrict__ b_pe,
                                                       bf16_t* __restrict__ b_w, bf16_t* __restrict__ b_q, bf16_t* __restrict__ b_p,
                                                       int cap_b, unsigned* err_word) {
  __shared__ double sh[NB_TPB / BLISS_WAVE];
  const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
  const int S = cnt->S;
  if (blockIdx.x == 0 && tid == 0) {                                // k_wl_coef's error bits: into the record, the word back to idle
    const unsigned bad = *err_word;
    if (bad) {
      atomicOr(&cnt->err, (int)bad);
      *err_word = 0u;
    }
  }
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int o = min(b_indptr[s], cap_b), e = min(b_indptr[s + 1], cap_b);
    if (e <= o) continue;
    const uint2 cf = mode == BLISS_WN_EXP3 ? coef[s] : make_uint2(0u, 0u);
    if (b_pe[o] == 0u) {                                            // a whole column: k_nb_tail's unit weights stand
      for (int j = o + tid; j < e; j += NB_TPB) {
        b_q[j] = wn_q(mode, prob, b_pos[j], cf, ome_f);
        b_p[j] = NB_ONE_BF16;
      }
      continue;
    }
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
      b_q[j] = wn_q(mode, prob, b_pos[j], cf, ome_f);
      b_p[j] = f2bf((float)p * 2.3283064365386963e-10f);            // uint32 -> fp32 to nearest even, * 2^-32 exact
    }
  }
}

static inline long long wl_rec_word(int num_nodes) {                // the per-seed records behind the tile counts, 8-byte aligned
  const long long words = nb_bitmap_words(num_nodes);
  return (NB_HDR + words + words / NB_TILE + 1) & ~1ll;
}

}  // namespace

extern "C" {

int64_t bliss_wlabor_scratch_bytes(int32_t num_nodes, int32_t cap_s, int32_t cap_b) {
  if (num_nodes <= 0 || cap_s <= 0 || cap_b < 0) return BLISS_EINVAL;
  return (int64_t)(((wl_rec_word(num_nodes) + 5ll * cap_s + (long long)cap_b) * 4 + 15) & ~15ll);
}

int bliss_wlabor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                       int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step,
                       int layer_dependency, int32_t mode, const void* prob_pos, float eta, float one_minus_eta,
                       const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* p_ij, void* scratch, void* stream) {
  if (!g || !seeds || !ws || !out || !scratch || cap_s <= 0 || fanout == 0) return BLISS_EINVAL;
  if (!g->indptr || !g->indices || g->num_nodes <= 0 || g->num_edges < 0 || g->num_edges > (int64_t)INT32_MAX) return BLISS_EINVAL;
  if (n_seeds < 0 && !n_seeds_dev) return BLISS_EINVAL;
  if (!ws->counts || !ws->seg_ptr || !ws->kept_nid || !ws->kept_map || ws->cap_k <= 0) return BLISS_EINVAL;
  if (!out->indptr || !out->src || !out->dst || !out->pos || !out->eid || !out->edge_weights || !out->q_ij || out->cap_b < 0)
    return BLISS_EINVAL;
  if (((uintptr_t)scratch & 15) || ((!keys_override || bump_step) && !step_dev)) return BLISS_EINVAL;
  if ((mode != BLISS_WN_RAW && mode != BLISS_WN_EXP3) || !prob_pos || ((uintptr_t)prob_pos & 1)) return BLISS_EINVAL;
  if (!p_ij || ((uintptr_t)p_ij & 1) || ((uintptr_t)keys_override & 3)) return BLISS_EINVAL;
  if (mode == BLISS_WN_EXP3 && !(eta >= 0.0f && one_minus_eta >= 0.0f)) return BLISS_EINVAL;   // (negative or NaN)
  hipStream_t st = (hipStream_t)stream;
  LayerCounts* cnt = (LayerCounts*)ws->counts;
  const long long* indptr = (const long long*)g->indptr;
  const bf16_t* prob = (const bf16_t*)prob_pos;
  const int V = g->num_nodes, cap_k = ws->cap_k, cap_b = out->cap_b;
  const int key_layer = layer_dependency ? 0 : layer;               // the same variate per vertex in all layers of a step
  // scratch: tickets and the pending-error word, bitmap (all that must be idle first: their place depends on num_nodes alone),
  // tile counts, then the per-seed (sum, eta / n) records, the (c_s, e_max) records, c_s counts and p_e
  unsigned* scr = (unsigned*)scratch;
  unsigned* bitmap = scr + NB_HDR;
  const long long words = nb_bitmap_words(V);
  const int n_tiles = (int)(words / NB_TILE);
  int* tile_cnt = (int*)(bitmap + words);
  uint2* coef = (uint2*)(scr + wl_rec_word(V));
  uint2* sc = coef + cap_s;
  int* col_cnt = (int*)(sc + cap_s);
  unsigned* b_pe = (unsigned*)(col_cnt + cap_s);
  const int gt = nb_grid(n_tiles, 1, 1024), gs = nb_grid(cap_s, 1, 2048), gw = nb_grid(cap_s, LI_COLS, 1024);
  if (mode == BLISS_WN_EXP3)
    k_wl_coef<<<gs, NB_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, prob, eta, coef, scr + WL_ERR_WORD);
  if (fanout > 0)                                                   // (fanout < 0: every column is whole, nothing reads a scale)
    k_wl_solve<<<gw, NB_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, mode, prob, one_minus_eta, coef, sc);
  k_wl_count<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, keys_override, seed,
                                    (const long long*)step_dev, key_layer, mode, prob, one_minus_eta, coef, sc, ws->kept_nid,
                                    ws->kept_map, cap_k, col_cnt);
  k_lb_scan<<<1, NB_SCAN_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, col_cnt, cnt, ws->seg_ptr, out->indptr, cap_b,
                                       cap_k);
  k_wl_write<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, g->eid, V, seeds, cnt, fanout, keys_override, seed, (long long*)step_dev,
                                    key_layer, bump_step, mode, prob, one_minus_eta, coef, sc, ws->kept_map, out->indptr, out->pos,
                                    out->dst, out->eid, b_pe, cap_b, bitmap, scr);
  k_nb_count<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, cap_k, tile_cnt, scr + 1);
  k_nb_number<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, tile_cnt, cap_k, ws->kept_nid, ws->kept_map);
  k_nb_tail<<<nb_grid(cap_b, NB_TPB, 2048), NB_TPB, 0, st>>>(g->indices, V, cnt, out->pos, ws->kept_map, out->src,
                                                             (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  k_nb_clean<<<nb_grid(cap_k, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, ws->kept_nid, cap_k, V, ws->kept_map,
                                                              (bf16_t*)ws->node_prob);
  k_wl_weights<<<gs, NB_TPB, 0, st>>>(cnt, mode, prob, one_minus_eta, coef, out->indptr, out->pos, b_pe, (bf16_t*)out->edge_weights,
                                      (bf16_t*)out->q_ij, (bf16_t*)p_ij, cap_b, scr + WL_ERR_WORD);
  return (int)hipGetLastError();
}

}  // extern "C"
