// The WEIGHTED neighbor draw on the device (fit.NeighborSampler(draw="device", prob=...) and fit.BanditNeighborSampler; DESIGN.md
// section 17): up to `fanout` in-edges per seed column, without replacement, drawn by a keyed exponential race over the column's
// edge probabilities -- csrc/neighbor.hip's per-column select over the race keys of csrc/mn_draw.hip, keyed by the EDGE.  The rule
// is normative, tests/wneighbor_ref.py restates it on the CPU:
//
//   q_pos   = prob_pos[pos] (raw mode, bf16, unnormalised), or eta / n_i + (1 - eta) * w_pos / sum_col(w) with edge_q's roundings
//             (EXP3 mode: the column sum exact in block-floating fixed point, rounded once to bf16)
//   u_pos   = ((key32(pos) >> 8) + 1) * 2^-24, key32 = csrc/neighbor.hip's edge key (seed, step, layer, CSC position); in (0, 1]
//   key_pos = fp32(-log(fp64(u_pos)) / fp64(q_pos)), the sign of zero dropped; +inf unless q_pos > 0 (a NaN q: +inf)
//   column s with CSC positions [a, b), d = b - a:  k = d if fanout < 0 or d <= fanout (WHOLE: no key is computed), else fanout;
//   kept = the k smallest pairs (key bits, pos) -- an edge with q <= 0 is a filler, taken only when the positive ones run out
//   q_ij = q_pos for every kept edge (whole columns too); edge_weights = the Hajek weight under the mean aggregation,
//   (1 / q_e) * k_s / sum over the column's kept e' of (1 / q_e'), fp64, rounded once to bf16; 1 in a whole column and in a column
//   that keeps an edge whose q is not a positive finite number; node_prob = 1.  Block, sources, counts, clamps: csrc/neighbor.hip's.
//
// bliss_wneighbor_layer = eight launches on one stream, no host round trip; S, E, B, K are read and written on the device:
//   k_nb_scan     unchanged (k = min(fanout, d) is known before the draw)
//   k_wn_keys     one workgroup per column: in EXP3 mode the exact column sum and the per-seed eta / n term (left in scratch for
//                 k_wn_weights); the race key of every position of a non-whole column, STAGED once by CSC position (an fp64 log and
//                 a divide per key: the select reads a key five times); the last workgroup (a ticket) bumps the step
//   k_nb_select   csrc/neighbor.hip's radix select and ordered write, over the staged keys
//   k_nb_count / k_nb_number / k_nb_tail / k_nb_clean   the shared tail (unit weights, q_ij = 1)
//   k_wn_weights  one workgroup per column: q_ij of every kept edge, the fp64 sum of 1 / q in a fixed order, the Hajek weights
// Every word a replay relies on (the two tickets, the bitmap, kept_map) is left zero / -1 by the kernel that used it; everything
// else (the per-seed record, the staged keys) is rewritten by every call before it is read.
#include "neighbor_tail.cuh"
#include "edge_q.cuh"

namespace {

#define WN_INF_BITS 0x7f800000u

// the race key's fp32 bits: non-negative, so they order as unsigned integers
__device__ __forceinline__ unsigned wn_key_bits(unsigned long long mk, int pos, bf16_t qb) {
  const float q = bf2f(qb);
  if (!(q > 0.0f)) return WN_INF_BITS;                              // zero, negative, NaN: a filler
  const unsigned k32 = nb_key(mk, nullptr, pos);
  const float u = (float)((k32 >> 8) + 1u) * 5.9604644775390625e-8f;      // (0, 1], exact in fp32
  const float key = (float)(-log((double)u) / (double)q);           // one fp64 quotient, rounded once
  return __float_as_uint(key) & 0x7fffffffu;                        // (u = 1: -0.0)
}

__global__ void __launch_bounds__(NB_TPB) k_wn_keys(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
                                                    LayerCounts* cnt, int fanout, int mode, const bf16_t* __restrict__ prob,
                                                    float eta_f, float ome_f, const unsigned* __restrict__ ov,
                                                    unsigned long long seed, long long* step_dev, int layer, int bump_step,
                                                    uint2* __restrict__ coef, unsigned* __restrict__ keyst,
                                                    unsigned* __restrict__ keys_out, unsigned* ticket) {
  __shared__ long long sh[NB_TPB / BLISS_WAVE];
  const int tid = threadIdx.x;
  const int S = cnt->S;
  unsigned long long mk = 0;
  if (!ov) mk = nb_mdkey(seed, (unsigned long long)*step_dev, layer);
  int bad = 0;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int nid = seeds[s];
    if ((unsigned)nid >= (unsigned)V) continue;
    const long long a64 = g_indptr[nid];
    const int a = (int)a64, d = (int)(g_indptr[nid + 1] - a64);
    if (d == 0) continue;
    uint2 cf = make_uint2(0u, 0u);
    if (mode == BLISS_WN_EXP3) {
      cf = wn_col_record<NB_TPB>(prob, a, d, eta_f, sh, &bad);         // the exact column sum and the eta / n term (edge_q.cuh)
      if (tid == 0) coef[s] = cf;
    }
    if (fanout < 0 || d <= fanout) continue;                        // a whole column: no key
    for (int i = tid; i < d; i += NB_TPB) {
      const int pos = a + i;
      const unsigned kb = ov ? ov[pos] : wn_key_bits(mk, pos, wn_q(mode, prob, pos, cf, ome_f));
      keyst[pos] = kb;
      if (keys_out) keys_out[pos] = kb;
    }
  }
  if (bad) atomicOr(&cnt->err, bad);
  if (!bump_step) return;
  // every workgroup has read the step when it takes its ticket; the last one bumps it and leaves the ticket zero
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *step_dev += 1;
  }
}

// fp64 -> bf16, ONE rounding to nearest even (positive finite values below bf16's largest: the weights, at most k_s)
__device__ __forceinline__ bf16_t wn_d2bf(double x) {
  if (x < 0x1p-126) return (bf16_t)(unsigned)rint(x * 0x1p133);     // bf16's subnormal spacing; 128 = the smallest normal number
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  int e = (int)((b >> 52) & 0x7ffull) - 1023 + 127;
  const unsigned long long m = b & ((1ull << 52) - 1ull), rem = m & ((1ull << 45) - 1ull), half = 1ull << 44;
  unsigned q = (unsigned)(m >> 45);
  if (rem > half || (rem == half && (q & 1u))) q += 1u;
  if (q >= 128u) { q = 0u; e += 1; }
  return (bf16_t)(((unsigned)e << 7) | q);
}

__global__ void __launch_bounds__(NB_TPB) k_wn_weights(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
                                                       const LayerCounts* __restrict__ cnt, int fanout, int mode,
                                                       const bf16_t* __restrict__ prob, float ome_f, const uint2* __restrict__ coef,
                                                       const int* __restrict__ b_indptr, const int* __restrict__ b_pos,
                                                       bf16_t* __restrict__ b_w, bf16_t* __restrict__ b_q, int cap_b) {
  __shared__ double sh[NB_TPB / BLISS_WAVE];
  __shared__ int sh_bad;
  const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
  const int S = cnt->S;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int nid = seeds[s];
    if ((unsigned)nid >= (unsigned)V) continue;
    const int d = (int)(g_indptr[nid + 1] - g_indptr[nid]);
    const int o = min(b_indptr[s], cap_b), e = min(b_indptr[s + 1], cap_b);
    if (e <= o) continue;
    const bool all = fanout < 0 || d <= fanout;
    const uint2 cf = mode == BLISS_WN_EXP3 ? coef[s] : make_uint2(0u, 0u);
    // q_ij of every kept edge; the sum of 1 / q in a fixed order: a strided partial per thread, a shuffle tree per wave, the
    // waves in order
    double acc = 0.0;
    int degenerate = 0;
    for (int j = o + tid; j < e; j += NB_TPB) {
      const bf16_t qb = wn_q(mode, prob, b_pos[j], cf, ome_f);
      b_q[j] = qb;
      const float q = bf2f(qb);
      if (q > 0.0f && q < __uint_as_float(WN_INF_BITS)) acc += 1.0 / (double)q;
      else degenerate = 1;
    }
    if (all) continue;                                              // a whole column: k_nb_tail's unit weights stand
#pragma unroll
    for (int dd = BLISS_WAVE / 2; dd >= 1; dd >>= 1) acc += __shfl_down(acc, dd);
    __syncthreads();                                                // (sh of the previous column is done with)
    if (tid == 0) sh_bad = 0;
    if (lane == 0) sh[wid] = acc;
    __syncthreads();
    if (degenerate) sh_bad = 1;
    __syncthreads();
    if (sh_bad) continue;                                           // a kept edge without a positive finite q: unit weights
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < NB_TPB / BLISS_WAVE; ++k) tot += sh[k];
    const double ks = (double)(e - o);
    for (int j = o + tid; j < e; j += NB_TPB) b_w[j] = wn_d2bf((1.0 / (double)bf2f(b_q[j])) * ks / tot);
  }
}

static inline long long wn_coef_word(int num_nodes) {               // the per-seed record behind the tile counts, 8-byte aligned
  const long long words = nb_bitmap_words(num_nodes);
  return (NB_HDR + words + words / NB_TILE + 1) & ~1ll;
}

}  // namespace

extern "C" {

int64_t bliss_wneighbor_scratch_bytes(int32_t num_nodes, int32_t cap_s, int64_t num_edges) {
  if (num_nodes <= 0 || cap_s <= 0 || num_edges < 0 || num_edges > (int64_t)INT32_MAX) return BLISS_EINVAL;
  return (int64_t)(((wn_coef_word(num_nodes) + 2ll * cap_s + num_edges) * 4 + 15) & ~15ll);
}

int bliss_wneighbor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                          int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer,
                          int bump_step, int32_t mode, const void* prob_pos, float eta, float one_minus_eta, uint32_t* keys_out,
                          const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* scratch, void* stream) {
  if (!g || !seeds || !ws || !out || !scratch || cap_s <= 0 || fanout == 0) return BLISS_EINVAL;
  if (!g->indptr || !g->indices || g->num_nodes <= 0 || g->num_edges < 0 || g->num_edges > (int64_t)INT32_MAX) return BLISS_EINVAL;
  if (n_seeds < 0 && !n_seeds_dev) return BLISS_EINVAL;
  if (!ws->counts || !ws->seg_ptr || !ws->kept_nid || !ws->kept_map || ws->cap_k <= 0) return BLISS_EINVAL;
  if (!out->indptr || !out->src || !out->dst || !out->pos || !out->eid || !out->edge_weights || !out->q_ij || out->cap_b < 0)
    return BLISS_EINVAL;
  if (((uintptr_t)scratch & 15) || ((!keys_override || bump_step) && !step_dev)) return BLISS_EINVAL;
  if ((mode != BLISS_WN_RAW && mode != BLISS_WN_EXP3) || !prob_pos || ((uintptr_t)prob_pos & 1)) return BLISS_EINVAL;
  if (((uintptr_t)keys_override & 3) || ((uintptr_t)keys_out & 3)) return BLISS_EINVAL;
  if (mode == BLISS_WN_EXP3 && !(eta >= 0.0f && one_minus_eta >= 0.0f)) return BLISS_EINVAL;   // (negative or NaN)
  hipStream_t st = (hipStream_t)stream;
  LayerCounts* cnt = (LayerCounts*)ws->counts;
  const long long* indptr = (const long long*)g->indptr;
  const bf16_t* prob = (const bf16_t*)prob_pos;
  const int V = g->num_nodes, cap_k = ws->cap_k, cap_b = out->cap_b;
  // scratch: tickets, bitmap (all that must be idle first: their place depends on num_nodes alone), tile counts, the per-seed
  // record, the staged keys by CSC position
  unsigned* scr = (unsigned*)scratch;
  unsigned* bitmap = scr + NB_HDR;
  const long long words = nb_bitmap_words(V);
  const int n_tiles = (int)(words / NB_TILE);
  int* tile_cnt = (int*)(bitmap + words);
  uint2* coef = (uint2*)(scr + wn_coef_word(V));
  unsigned* keyst = (unsigned*)(coef + cap_s);
  const int gt = nb_grid(n_tiles, 1, 1024), gs = nb_grid(cap_s, 1, 2048);
  k_nb_scan<<<1, NB_SCAN_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, cnt, ws->seg_ptr, out->indptr, cap_b,
                                       ws->kept_nid, ws->kept_map, cap_k);
  k_wn_keys<<<gs, NB_TPB, 0, st>>>(indptr, V, seeds, cnt, fanout, mode, prob, eta, one_minus_eta, keys_override, seed,
                                   (long long*)step_dev, layer, bump_step, coef, keyst, keys_out, scr);
  k_nb_select<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, g->eid, V, seeds, cnt, fanout, keyst, seed, (long long*)step_dev, layer, 0,
                                     ws->kept_map, out->indptr, out->pos, out->dst, out->eid, cap_b, bitmap, scr);
  k_nb_count<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, cap_k, tile_cnt, scr + 1);
  k_nb_number<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, tile_cnt, cap_k, ws->kept_nid, ws->kept_map);
  k_nb_tail<<<nb_grid(cap_b, NB_TPB, 2048), NB_TPB, 0, st>>>(g->indices, V, cnt, out->pos, ws->kept_map, out->src,
                                                             (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  k_nb_clean<<<nb_grid(cap_k, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, ws->kept_nid, cap_k, V, ws->kept_map,
                                                              (bf16_t*)ws->node_prob);
  k_wn_weights<<<gs, NB_TPB, 0, st>>>(indptr, V, seeds, cnt, fanout, mode, prob, one_minus_eta, coef, out->indptr, out->pos,
                                      (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  return (int)hipGetLastError();
}

}  // extern "C"
