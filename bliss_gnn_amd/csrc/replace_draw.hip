// Draws WITH REPLACEMENT on the device: a keyed categorical draw in integers only, for the node-wise
// sampler (fit.NeighborSampler(draw="device", replace=True), uniform or with edge probabilities) and for the layer-wise multinomial
// samplers (LadiesSampler / BanditLadiesSampler with draw="device-replace").  The rule is normative, tests/replace_ref.py restates
// it on the CPU with Python integers, and every comparison is exact:
//
//   fin(z)  = the SplitMix64 finaliser of nb_key;  mk = nb_mdkey(seed, step, layer)
//   h       = fin(mk ^ (uint64)(uint32)ident), ident = the node id of the seed column (node-wise) or 0xFFFFFFFF (layer-wise)
//   r_j     = fin(h ^ ((uint64)(j + 1) * 0x9E3779B97F4A7C15)), the variate of draw j = 0, 1, ...
//   weights: over one group of bf16 probabilities (a seed column, or a layer's candidates), E = floor(log2(largest positive finite
//           value)), w_i = floor(x_i * 2^(23 - E)) for a positive finite x_i, else 0 (<= 0, NaN, inf); the largest lands in
//           [2^23, 2^24), a value below 2^(E - 23) becomes 0 and is never drawn (the mode's resolution); W = sum w_i (uint64)
//   one draw over a group of m entries: W > 0: t = mulhi64(r_j, W), the pick is the smallest i whose inclusive prefix sum exceeds t;
//           W == 0, or the uniform mode: the pick is mulhi64(r_j, m)
//
// bliss_neighbor_replace_layer: column s with node id v, CSC positions [a, a + d), fanout f:  k_s = d if f < 0 (a whole column, no
// draw), 0 if d == 0, else f -- ALSO when d <= f.  Block edges column by column, inside a column in ascending (position, j); repeats
// are separate, adjacent edges.  Everything else is csrc/neighbor.hip's.  Launches on one stream, no host round trip:
//   k_nr_scan     k_nb_scan with k_s as above (B is known before the draw)
//   k_nr_draw     one workgroup per column (one wave per column in the uniform mode with f <= 64, where a column costs O(f) and none
//                 of it is read).  Weighted: the block maximum of the positive finite bit patterns (they order as integers), totals of
//                 <= 1024 chunks (the chunk widens by powers of two for columns longer than 1024) scanned into inclusive prefixes in
//                 LDS; per draw a binary search over the chunk prefixes and a rescan of one chunk; the f picks ranked by counting in
//                 LDS; pos / dst / eid written at indptr[s] + rank, the sources marked in the bitmap; the last workgroup (a ticket)
//                 bumps the step
//   k_nb_count / k_nb_number / k_nb_tail / k_nb_clean   the shared tail (unit weights, q_ij = 1)
//   k_nr_weights  (with probabilities) q_ij = prob_pos[pos]; W_e = (1 / q_e) * k_s / sum over the column's edges, repeats counted, of
//                 1 / q_e', fp64 in a fixed order, rounded once to bf16; unit weights in a whole column and in a column that fell back
//                 to the uniform pick
//
// bliss_multinomial_draw_replace: n = min(fanout, C) draws over the layer's C candidates, drawn[i] = 1 iff some draw picked i.
//   k_mr_max      per-workgroup maxima of the positive finite bit patterns (plain stores, one slot per workgroup)
//   k_mr_sums     per 1024-candidate chunk: fixed-point weights, their inclusive prefix inside the chunk (scratch), the chunk total;
//                 drawn[0, C) = 0; the LAST workgroup (a ticket, k_nb_count's hand-over) scans the chunk totals into inclusive chunk
//                 prefixes and W, reads the step ONCE, leaves h in the scratch and bumps the step; the ticket is left zero
//   k_mr_draw     one thread per draw: a binary search over the chunk prefixes, then one inside the chunk; drawn[pick] = 1
// Only the ticket relies on its earlier value; every other scratch word is rewritten by each call before it is read.
#include "neighbor_tail.cuh"

namespace {

#define NR_MAX_FANOUT BLISS_NR_MAX_FANOUT
#define NR_CHUNKS 1024                                                // chunk prefixes of one column held in LDS
#define NR_GOLD 0x9E3779B97F4A7C15ull
#define MR_TPB 1024
#define MR_CHUNK 1024
#define MR_SLOTS 256                                                  // k_mr_max's grid bound
#define MR_HDR 4                                                      // scratch, 64-bit words: [0] ticket, [1] h, [2] W, [3] unused

__device__ __forceinline__ unsigned long long rd_fin(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long rd_variate(unsigned long long h, int j) {
  return rd_fin(h ^ ((unsigned long long)(j + 1) * NR_GOLD));
}
// a positive finite bf16: sign clear, not zero, below +inf; such bit patterns order like their values
__device__ __forceinline__ unsigned rd_posfin(bf16_t b) { return ((unsigned)b - 1u) < 0x7f7fu ? (unsigned)b : 0u; }
// value = M * 2^ex with M < 256: the mantissa with its hidden bit, subnormals at the smallest normal exponent
__device__ __forceinline__ void rd_split(unsigned b, unsigned* M, int* ex) {
  const unsigned e = b >> 7;
  *M = (b & 0x7fu) | (e ? 0x80u : 0u);
  *ex = (int)(e ? e : 1u) - 134;
}
// floor(log2) of a positive finite bit pattern
__device__ __forceinline__ int rd_log2(unsigned b) {
  unsigned M; int ex;
  rd_split(b, &M, &ex);
  return ex + 31 - __clz((int)M);
}
// w = floor(x * 2^(23 - E)); 0 for anything but a positive finite x (E = rd_log2 of the group's largest, so w < 2^24)
__device__ __forceinline__ unsigned rd_weight(bf16_t b, int E) {
  if (!rd_posfin(b)) return 0u;
  unsigned M; int ex;
  rd_split(b, &M, &ex);
  const int sh = ex + 23 - E;
  return sh >= 0 ? M << sh : (sh > -8 ? M >> (-sh) : 0u);
}

// block maximum of one non-negative int per thread; `sh` needs 16 ints
__device__ __forceinline__ int rd_block_max(int v, int* sh) {
  const int wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_max_u31(v);
  __syncthreads();                                                  // (sh of an earlier use is done with)
  if (lane_id() == 0) sh[wid] = v;
  __syncthreads();
  int m = 0;
  for (int k = 0; k < nw; ++k) m = max(m, sh[k]);
  return m;
}

// ---------------------------------------------------------------------------------------------------------------- node-wise
// k_nb_scan (neighbor_tail.cuh) with the replacement rule's k: a non-empty column holds `fanout` edges whatever its degree
__global__ void __launch_bounds__(NB_SCAN_TPB) k_nr_scan(const long long* __restrict__ g_indptr, int V, const int* __restrict__ seeds,
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
        k = (fanout < 0 || d == 0) ? d : fanout;
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

template <int TPB, bool WEIGHTED>
__global__ void __launch_bounds__(TPB) k_nr_draw(const long long* __restrict__ g_indptr, const int* __restrict__ indices,
                                                 const int* __restrict__ g_eid, int V, const int* __restrict__ seeds,
                                                 const LayerCounts* __restrict__ cnt, int fanout,
                                                 const bf16_t* __restrict__ prob, const unsigned long long* __restrict__ r_ov,
                                                 unsigned long long seed, long long* step_dev, int layer, int bump_step,
                                                 const int* __restrict__ kept_map, const int* __restrict__ b_indptr,
                                                 int* __restrict__ b_pos, int* __restrict__ b_dst, int* __restrict__ b_eid,
                                                 int* __restrict__ picks_out, int cap_b, unsigned* bitmap, unsigned* ticket) {
  constexpr int PER = NR_CHUNKS / TPB;                              // chunk prefixes per thread
  __shared__ unsigned long long pre[WEIGHTED ? NR_CHUNKS : 1];
  __shared__ int pk[NR_MAX_FANOUT];
  __shared__ long long sh[17];
  const int tid = threadIdx.x;
  const int S = cnt->S;
  unsigned long long mk = 0;
  if (!r_ov) mk = nb_mdkey(seed, (unsigned long long)*step_dev, layer);
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int nid = seeds[s];
    if ((unsigned)nid >= (unsigned)V) continue;
    const long long a64 = g_indptr[nid];
    const int a = (int)a64, d = (int)(g_indptr[nid + 1] - a64);
    if (d == 0) continue;
    const int o = b_indptr[s];
    if (fanout < 0) {                                               // a whole column: no draw
      for (int i = tid; i < d; i += TPB) {
        if ((long long)o + i >= (long long)cap_b) break;
        const int j = o + i, p = a + i;
        b_pos[j] = p;
        b_dst[j] = s;
        b_eid[j] = g_eid ? g_eid[p] : p;
        if (picks_out) picks_out[j] = i;
        const int u = indices[p];
        if ((unsigned)u < (unsigned)V && kept_map[u] < 0) atomicOr(bitmap + (u >> 5), 1u << (u & 31));
      }
      continue;
    }
    __syncthreads();                                                // (pk, pre, sh of the previous column are done with)
    unsigned long long W = 0;
    int lg = 0, E = 0;
    if constexpr (WEIGHTED) {
      int mx = 0;
      for (int i = tid; i < d; i += TPB) mx = max(mx, (int)rd_posfin(prob[a + i]));
      mx = rd_block_max(mx, (int*)sh);
      if (mx) {                                                     // (else W stays 0: the uniform pick)
        E = rd_log2((unsigned)mx);
        while (((long long)NR_CHUNKS << lg) < (long long)d) ++lg;   // chunk width 2^lg: at most NR_CHUNKS chunks
        unsigned long long part[PER], mine = 0;
#pragma unroll
        for (int c = 0; c < PER; ++c) {
          const long long lo = (long long)(tid * PER + c) << lg;
          const long long hi = min(lo + (1ll << lg), (long long)d);
          unsigned long long t = 0;
          for (long long i = lo; i < hi; ++i) t += rd_weight(prob[a + i], E);
          part[c] = t;
          mine += t;
        }
        long long tot;
        unsigned long long run = (unsigned long long)nb_scan64((long long)mine, sh, &tot);
#pragma unroll
        for (int c = 0; c < PER; ++c) { run += part[c]; pre[tid * PER + c] = run; }
        W = (unsigned long long)tot;
        __syncthreads();
      }
    }
    const unsigned long long h = rd_fin(mk ^ (unsigned long long)(unsigned)nid);
    for (int j = tid; j < fanout; j += TPB) {
      const unsigned long long r = r_ov ? r_ov[(long long)s * fanout + j] : rd_variate(h, j);
      int pick;
      if (WEIGHTED && W) {
        const unsigned long long t = __umul64hi(r, W);              // < W
        int lo = 0, hi = NR_CHUNKS - 1;                             // the smallest chunk whose inclusive prefix exceeds t
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (pre[mid] > t) hi = mid; else lo = mid + 1;
        }
        unsigned long long acc = lo ? pre[lo - 1] : 0ull;
        int i = (int)((long long)lo << lg);
        for (; i < d - 1; ++i) {                                    // ends inside the chunk: its prefix exceeds t
          acc += rd_weight(prob[a + i], E);
          if (acc > t) break;
        }
        pick = i;
      } else {
        pick = (int)__umul64hi(r, (unsigned long long)d);
      }
      pk[j] = pick;
    }
    __syncthreads();
    for (int j = tid; j < fanout; j += TPB) {
      const int pick = pk[j];
      int rank = 0;                                                 // picks ordered by (pick, j)
      for (int i = 0; i < fanout; ++i) {
        const int q = pk[i];
        rank += (q < pick || (q == pick && i < j)) ? 1 : 0;
      }
      if ((long long)o + rank < (long long)cap_b) {
        const int e = o + rank, p = a + pick;
        b_pos[e] = p;
        b_dst[e] = s;
        b_eid[e] = g_eid ? g_eid[p] : p;
        if (picks_out) picks_out[e] = pick;
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

// fp64 -> bf16, ONE rounding to nearest even (positive finite values below bf16's largest)   (= csrc/neighbor_w.hip:wn_d2bf)
__device__ __forceinline__ bf16_t nr_d2bf(double x) {
  if (x < 0x1p-126) return (bf16_t)(unsigned)rint(x * 0x1p133);
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  int e = (int)((b >> 52) & 0x7ffull) - 1023 + 127;
  const unsigned long long m = b & ((1ull << 52) - 1ull), rem = m & ((1ull << 45) - 1ull), half = 1ull << 44;
  unsigned q = (unsigned)(m >> 45);
  if (rem > half || (rem == half && (q & 1u))) q += 1u;
  if (q >= 128u) { q = 0u; e += 1; }
  return (bf16_t)(((unsigned)e << 7) | q);
}

__global__ void __launch_bounds__(NB_TPB) k_nr_weights(const LayerCounts* __restrict__ cnt, int fanout, const bf16_t* __restrict__ prob,
                                                       const int* __restrict__ b_indptr, const int* __restrict__ b_pos,
                                                       bf16_t* __restrict__ b_w, bf16_t* __restrict__ b_q, int cap_b) {
  __shared__ double sh[NB_TPB / BLISS_WAVE];
  __shared__ int sh_bad;
  const int tid = threadIdx.x, lane = lane_id(), wid = tid >> 6;
  const int S = cnt->S;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {                 // (everything below is uniform over the workgroup)
    const int o = min(b_indptr[s], cap_b), e = min(b_indptr[s + 1], cap_b);
    if (e <= o) continue;
    double acc = 0.0;
    int degenerate = 0;
    for (int j = o + tid; j < e; j += NB_TPB) {
      const bf16_t qb = prob[b_pos[j]];
      b_q[j] = qb;
      if (rd_posfin(qb)) acc += 1.0 / (double)bf2f(qb);
      else degenerate = 1;
    }
    if (fanout < 0) continue;                                       // a whole column: k_nb_tail's unit weights stand
#pragma unroll
    for (int dd = BLISS_WAVE / 2; dd >= 1; dd >>= 1) acc += __shfl_down(acc, dd);
    __syncthreads();                                                // (sh of the previous column is done with)
    if (tid == 0) sh_bad = 0;
    if (lane == 0) sh[wid] = acc;
    __syncthreads();
    if (degenerate) sh_bad = 1;
    __syncthreads();
    if (sh_bad) continue;                                           // the column fell back to the uniform pick: unit weights
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < NB_TPB / BLISS_WAVE; ++k) tot += sh[k];
    const double ks = (double)(e - o);
    for (int j = o + tid; j < e; j += NB_TPB) b_w[j] = nr_d2bf((1.0 / (double)bf2f(b_q[j])) * ks / tot);
  }
}

// --------------------------------------------------------------------------------------------------------------- layer-wise
__global__ void __launch_bounds__(MR_TPB) k_mr_max(const bf16_t* __restrict__ p, const LayerCounts* __restrict__ cnt, int cap_c,
                                                   unsigned* __restrict__ slots) {
  __shared__ int sh[16];
  const int C = max(min(cnt->C, cap_c), 0);
  int mx = 0;
  for (int i = blockIdx.x * MR_TPB + threadIdx.x; i < C; i += gridDim.x * MR_TPB) mx = max(mx, (int)rd_posfin(p[i]));
  mx = rd_block_max(mx, sh);
  if (threadIdx.x == 0) slots[blockIdx.x] = (unsigned)mx;
}

__global__ void __launch_bounds__(MR_TPB) k_mr_sums(const bf16_t* __restrict__ p, const LayerCounts* __restrict__ cnt, int cap_c,
                                                    int n_slots, const unsigned* __restrict__ slots, int r_given,
                                                    unsigned long long seed, long long* step_dev, int layer, int bump_step,
                                                    unsigned long long* scr, unsigned long long* chunk_inc,
                                                    unsigned long long* __restrict__ pre, int* __restrict__ drawn) {
  __shared__ long long sh[17];
  __shared__ int sh_last;
  const int tid = threadIdx.x;
  const int C = max(min(cnt->C, cap_c), 0);
  const int nchunks = (C + MR_CHUNK - 1) / MR_CHUNK;
  const int mx = rd_block_max(tid < n_slots ? (int)slots[tid] : 0, (int*)sh);
  const int E = mx ? rd_log2((unsigned)mx) : 0;
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int i = chunk * MR_CHUNK + tid;
    const long long w = (mx && i < C) ? (long long)rd_weight(p[i], E) : 0;
    long long tot;
    const long long ex = nb_scan64(w, sh, &tot);
    if (i < C) { pre[i] = (unsigned long long)(ex + w); drawn[i] = 0; }
    if (tid == 0) __hip_atomic_store(chunk_inc + chunk, (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the chunk totals are complete when every workgroup has passed here: stores drained, then a ticket (k_nb_count's hand-over)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    unsigned* ticket = (unsigned*)scr;
    sh_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    if (sh_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!sh_last) return;
  // the last workgroup: totals read past this XCD's L2, replaced by their inclusive prefix
  long long run = 0;
  for (int base = 0; base < nchunks; base += MR_TPB) {
    const int c = base + tid;
    const long long v = c < nchunks ? (long long)__hip_atomic_load(chunk_inc + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    long long tot;
    const long long ex = nb_scan64(v, sh, &tot);
    if (c < nchunks) chunk_inc[c] = (unsigned long long)(run + ex + v);
    run += tot;
  }
  if (tid == 0) {
    scr[2] = (unsigned long long)run;                               // W
    if (!r_given) scr[1] = rd_fin(nb_mdkey(seed, (unsigned long long)*step_dev, layer) ^ 0xFFFFFFFFull);
    if (bump_step) *step_dev += 1;                                  // (nobody else reads the step: h travels in the scratch)
  }
}

__global__ void __launch_bounds__(NB_TPB) k_mr_draw(const LayerCounts* __restrict__ cnt, int cap_c, int fanout,
                                                    const unsigned long long* __restrict__ r_ov,
                                                    const unsigned long long* __restrict__ scr,
                                                    const unsigned long long* __restrict__ chunk_inc,
                                                    const unsigned long long* __restrict__ pre, int* __restrict__ drawn,
                                                    int* __restrict__ picks_out) {
  const int C = max(min(cnt->C, cap_c), 0);
  const int n = min(fanout, C);
  const int nchunks = (C + MR_CHUNK - 1) / MR_CHUNK;
  const unsigned long long h = scr[1], W = scr[2];
  for (int j = blockIdx.x * NB_TPB + threadIdx.x; j < n; j += gridDim.x * NB_TPB) {
    const unsigned long long r = r_ov ? r_ov[j] : rd_variate(h, j);
    int pick;
    if (W) {
      const unsigned long long t = __umul64hi(r, W);                // < W = chunk_inc[nchunks - 1]
      int lo = 0, hi = nchunks - 1;                                 // the smallest chunk whose inclusive prefix exceeds t
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (chunk_inc[mid] > t) hi = mid; else lo = mid + 1;
      }
      const unsigned long long rest = t - (lo ? chunk_inc[lo - 1] : 0ull);
      const int base = lo * MR_CHUNK;
      int l2 = 0, h2 = min(MR_CHUNK, C - base) - 1;                 // the smallest entry whose prefix inside the chunk exceeds rest
      while (l2 < h2) {
        const int mid = (l2 + h2) >> 1;
        if (pre[base + mid] > rest) h2 = mid; else l2 = mid + 1;
      }
      pick = base + l2;
    } else {
      pick = (int)__umul64hi(r, (unsigned long long)C);
    }
    drawn[pick] = 1;
    if (picks_out) picks_out[j] = pick;
  }
}

static inline long long mr_chunks(int cap_c) { return ((long long)cap_c + MR_CHUNK - 1) / MR_CHUNK; }

}  // namespace

extern "C" {

int64_t bliss_neighbor_replace_scratch_bytes(int32_t num_nodes, int32_t cap_s) {
  if (num_nodes <= 0 || cap_s <= 0) return BLISS_EINVAL;
  const long long words = nb_bitmap_words(num_nodes);
  return (int64_t)(((NB_HDR + words + words / NB_TILE) * 4 + 15) & ~15ll);
}

int bliss_neighbor_replace_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev,
                                 int32_t cap_s, int32_t fanout, const uint64_t* r_override, uint64_t seed, int64_t* step_dev,
                                 int32_t layer, int bump_step, const void* prob_pos, int32_t* picks_out, const bliss_layer_ws_t* ws,
                                 const bliss_block_out_t* out, void* scratch, void* stream) {
  if (!g || !seeds || !ws || !out || !scratch || cap_s <= 0 || fanout == 0 || fanout > NR_MAX_FANOUT) return BLISS_EINVAL;
  if (!g->indptr || !g->indices || g->num_nodes <= 0 || g->num_edges < 0 || g->num_edges > (int64_t)INT32_MAX) return BLISS_EINVAL;
  if (n_seeds < 0 && !n_seeds_dev) return BLISS_EINVAL;
  if (!ws->counts || !ws->seg_ptr || !ws->kept_nid || !ws->kept_map || ws->cap_k <= 0) return BLISS_EINVAL;
  if (!out->indptr || !out->src || !out->dst || !out->pos || !out->eid || !out->edge_weights || !out->q_ij || out->cap_b < 0)
    return BLISS_EINVAL;
  if (((uintptr_t)scratch & 15) || ((!r_override || bump_step) && !step_dev)) return BLISS_EINVAL;
  if (((uintptr_t)prob_pos & 1) || ((uintptr_t)r_override & 7) || ((uintptr_t)picks_out & 3)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  LayerCounts* cnt = (LayerCounts*)ws->counts;
  const long long* indptr = (const long long*)g->indptr;
  const bf16_t* prob = (const bf16_t*)prob_pos;
  const unsigned long long* rov = (const unsigned long long*)r_override;
  const int V = g->num_nodes, cap_k = ws->cap_k, cap_b = out->cap_b;
  // scratch: csrc/neighbor.hip's -- tickets, bitmap (whole tiles), one count per tile
  unsigned* scr = (unsigned*)scratch;
  unsigned* bitmap = scr + NB_HDR;
  const long long words = nb_bitmap_words(V);
  const int n_tiles = (int)(words / NB_TILE);
  int* tile_cnt = (int*)(bitmap + words);
  const int gt = nb_grid(n_tiles, 1, 1024);
  k_nr_scan<<<1, NB_SCAN_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, cnt, ws->seg_ptr, out->indptr, cap_b,
                                       ws->kept_nid, ws->kept_map, cap_k);
  if (prob)
    k_nr_draw<NB_TPB, true><<<nb_grid(cap_s, 1, 2048), NB_TPB, 0, st>>>(
        indptr, g->indices, g->eid, V, seeds, cnt, fanout, prob, rov, seed, (long long*)step_dev, layer, bump_step, ws->kept_map,
        out->indptr, out->pos, out->dst, out->eid, picks_out, cap_b, bitmap, scr);
  else if (fanout > 0 && fanout <= BLISS_WAVE)                      // a uniform column costs O(fanout): one wave per column
    k_nr_draw<BLISS_WAVE, false><<<nb_grid(cap_s, 1, 8192), BLISS_WAVE, 0, st>>>(
        indptr, g->indices, g->eid, V, seeds, cnt, fanout, prob, rov, seed, (long long*)step_dev, layer, bump_step, ws->kept_map,
        out->indptr, out->pos, out->dst, out->eid, picks_out, cap_b, bitmap, scr);
  else
    k_nr_draw<NB_TPB, false><<<nb_grid(cap_s, 1, 2048), NB_TPB, 0, st>>>(
        indptr, g->indices, g->eid, V, seeds, cnt, fanout, prob, rov, seed, (long long*)step_dev, layer, bump_step, ws->kept_map,
        out->indptr, out->pos, out->dst, out->eid, picks_out, cap_b, bitmap, scr);
  k_nb_count<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, cap_k, tile_cnt, scr + 1);
  k_nb_number<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, tile_cnt, cap_k, ws->kept_nid, ws->kept_map);
  k_nb_tail<<<nb_grid(cap_b, NB_TPB, 2048), NB_TPB, 0, st>>>(g->indices, V, cnt, out->pos, ws->kept_map, out->src,
                                                             (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  k_nb_clean<<<nb_grid(cap_k, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, ws->kept_nid, cap_k, V, ws->kept_map,
                                                              (bf16_t*)ws->node_prob);
  if (prob)
    k_nr_weights<<<nb_grid(cap_s, 1, 2048), NB_TPB, 0, st>>>(cnt, fanout, prob, out->indptr, out->pos, (bf16_t*)out->edge_weights,
                                                             (bf16_t*)out->q_ij, cap_b);
  return (int)hipGetLastError();
}

int64_t bliss_multinomial_draw_replace_scratch_bytes(int32_t cap_c) {
  if (cap_c <= 0) return BLISS_EINVAL;
  // 64-bit words: header, k_mr_max's slots (two per word), one inclusive prefix per chunk, one prefix per candidate
  const int64_t words = MR_HDR + MR_SLOTS / 2 + mr_chunks(cap_c) + (int64_t)cap_c;
  return (words * 8 + 15) & ~(int64_t)15;
}

int bliss_multinomial_draw_replace(const void* p_bf16, const void* counts, int32_t cap_c, int32_t fanout, const uint64_t* r_override,
                                   uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step, void* scratch, int32_t* drawn,
                                   int32_t* picks_out, void* stream) {
  if (!p_bf16 || !counts || !scratch || !drawn || cap_c <= 0 || fanout < 0) return BLISS_EINVAL;
  if (((uintptr_t)scratch & 15) || ((!r_override || bump_step) && !step_dev)) return BLISS_EINVAL;
  if (((uintptr_t)p_bf16 & 1) || ((uintptr_t)r_override & 7) || ((uintptr_t)picks_out & 3) || ((uintptr_t)drawn & 3)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const LayerCounts* cnt = (const LayerCounts*)counts;
  const bf16_t* p = (const bf16_t*)p_bf16;
  unsigned long long* scr = (unsigned long long*)scratch;
  unsigned* slots = (unsigned*)(scr + MR_HDR);
  unsigned long long* chunk_inc = scr + MR_HDR + MR_SLOTS / 2;
  unsigned long long* pre = chunk_inc + mr_chunks(cap_c);
  const int gm = nb_grid(cap_c, MR_TPB * 4, MR_SLOTS), gc = nb_grid(cap_c, MR_CHUNK, 1024);
  k_mr_max<<<gm, MR_TPB, 0, st>>>(p, cnt, cap_c, slots);
  k_mr_sums<<<gc, MR_TPB, 0, st>>>(p, cnt, cap_c, gm, slots, r_override != nullptr, seed, (long long*)step_dev, layer, bump_step, scr,
                                   chunk_inc, pre, drawn);
  k_mr_draw<<<nb_grid(fanout, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, cap_c, fanout, (const unsigned long long*)r_override, scr,
                                                              chunk_inc, pre, drawn, picks_out);
  return (int)hipGetLastError();
}

}  // extern "C"
