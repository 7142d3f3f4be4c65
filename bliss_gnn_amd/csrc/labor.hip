// The LABOR-0 sampler on the device (fit.LaborSampler): the keyed draw of csrc/neighbor.hip with the key on the
// edge's SOURCE NODE instead of its CSC position, and a per-column threshold instead of a per-column select.  One variate per source
// vertex is shared by all seeds of a layer, so the layer keeps `fanout` edges per column in expectation -- as the neighbor sampler
// does exactly -- out of far fewer distinct sources.  The rule is normative, tests/labor_ref.py restates it on the CPU:
//
//   key(u)  = (uint32)(z >> 32),  z = SplitMix64 finaliser of md_key(seed, step, layer') ^ (uint64)u,  u = indices[pos]   (integers only)
//             layer' = layer, or 0 for every layer with layer_dependency
//   column s with CSC positions [a, b), d = b - a:  every edge kept if fanout < 0 or d <= fanout (no key is computed); otherwise
//             thr = ((uint64)fanout << 32) / d  (1 <= thr < 2^32) and the edge at pos is kept iff (uint64)key(indices[pos]) < thr
//             (a multi-edge is kept or dropped as one; a column may keep nothing)
//   block:    columns in seed order, ascending position inside a column; indptr[s + 1] - indptr[s] = c_s, the kept count
//   sources:  the seeds first (local ids 0 .. S-1, in the order given), then the other sources of kept edges in ascending node id
//
// bliss_labor_layer = seven launches on one stream, no host round trip; S, E, B, K are read and written on the device:
//   k_lb_count   workgroups stride over the columns: the seed into kept_nid and kept_map, c_s by a block reduction
//   k_lb_scan    one workgroup: seg_ptr (degrees), indptr (c_s), S / E / B, clamps and error bits, the rest of the counts record
//   k_lb_write   workgroups stride over the columns, an ordered pass of 256-edge chunks: pos / dst / eid at indptr[s] + rank, the
//                edge's source, unless it is a seed, marked in the |V|-bit bitmap; the last workgroup (a ticket) bumps the step
//   k_nb_count, k_nb_number, k_nb_tail, k_nb_clean   the neighbor sampler's tail (csrc/neighbor_tail.cuh), as it stands
// The keys are recomputed from the hash in k_lb_write: no key or mark buffer.  A global atomicOr marks; no output depends on the
// order in which they land.  Every word a replay relies on (the two tickets, the bitmap, kept_map) is left zero / -1 by the kernel
// that used it, also after a flagged capacity overflow; everything else (c_s included) is rewritten by every call before it is read.
#include "labor_scan.cuh"

namespace {

// is the edge at CSC position p kept?  (a source id outside [0, V) -- not a graph this library builds -- is dropped unread)
__device__ __forceinline__ bool lb_take(unsigned long long mk, const unsigned* __restrict__ ov, const int* __restrict__ indices, int V,
                                        int p, unsigned long long thr) {
  const int u = indices[p];
  if ((unsigned)u >= (unsigned)V) return false;
  return (unsigned long long)lb_key(mk, ov, u) < thr;
}

__global__ void __launch_bounds__(NB_TPB) k_lb_count(const long long* __restrict__ g_indptr, const int* __restrict__ indices, int V,
                                                     const int* __restrict__ seeds, int S_host, const int* __restrict__ S_dev,
                                                     int cap_s, int fanout, const unsigned* __restrict__ ov, unsigned long long seed,
                                                     const long long* __restrict__ step_dev, int layer, int* __restrict__ kept_nid,
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
    int tot = 0;
    if (valid) {
      const long long a64 = g_indptr[nid];
      const int a = (int)a64, d = (int)(g_indptr[nid + 1] - a64);
      if (fanout < 0 || d <= fanout) {
        tot = d;
      } else {
        const unsigned long long thr = ((unsigned long long)(unsigned)fanout << 32) / (unsigned long long)d;
        int c = 0;
        for (int i = tid; i < d; i += NB_TPB) c += lb_take(mk, ov, indices, V, a + i, thr) ? 1 : 0;
        block_excl_scan(c, sh, &tot);
      }
    }
    if (tid == 0) col_cnt[s] = tot;
  }
}

__global__ void __launch_bounds__(NB_TPB) k_lb_write(const long long* __restrict__ g_indptr, const int* __restrict__ indices,
                                                     const int* __restrict__ g_eid, int V, const int* __restrict__ seeds,
                                                     const LayerCounts* __restrict__ cnt, int fanout,
                                                     const unsigned* __restrict__ ov, unsigned long long seed, long long* step_dev,
                                                     int layer, int bump_step, const int* __restrict__ kept_map,
                                                     const int* __restrict__ b_indptr, int* __restrict__ b_pos, int* __restrict__ b_dst,
                                                     int* __restrict__ b_eid, int cap_b, unsigned* bitmap, unsigned* ticket) {
  __shared__ int sh[17];
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
    const unsigned long long thr = all ? 0ull : ((unsigned long long)(unsigned)fanout << 32) / (unsigned long long)d;
    int run = 0;
    for (int base = 0; base < d; base += NB_TPB) {
      const int i = base + tid;
      bool take = all && i < d;
      int rank = i;
      if (!all) {
        take = i < d && lb_take(mk, ov, indices, V, a + i, thr);
        int tot;
        rank = run + block_excl_scan(take ? 1 : 0, sh, &tot);
        run += tot;
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

}  // namespace

extern "C" {

int64_t bliss_labor_scratch_bytes(int32_t num_nodes, int32_t cap_s) {
  if (num_nodes <= 0 || cap_s <= 0) return BLISS_EINVAL;
  const long long words = nb_bitmap_words(num_nodes);
  return (int64_t)(((NB_HDR + words + words / NB_TILE + (long long)cap_s) * 4 + 15) & ~15ll);
}

int bliss_labor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                      int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step,
                      int layer_dependency, const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* scratch, void* stream) {
  if (!g || !seeds || !ws || !out || !scratch || cap_s <= 0 || fanout == 0) return BLISS_EINVAL;
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
  unsigned* scr = (unsigned*)scratch;
  unsigned* bitmap = scr + NB_HDR;
  const long long words = nb_bitmap_words(V);
  const int n_tiles = (int)(words / NB_TILE);
  int* tile_cnt = (int*)(bitmap + words);
  int* col_cnt = tile_cnt + n_tiles;
  const int gt = nb_grid(n_tiles, 1, 1024), gs = nb_grid(cap_s, 1, 2048);
  k_lb_count<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, keys_override, seed,
                                    (const long long*)step_dev, key_layer, ws->kept_nid, ws->kept_map, cap_k, col_cnt);
  k_lb_scan<<<1, NB_SCAN_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, col_cnt, cnt, ws->seg_ptr, out->indptr, cap_b,
                                       cap_k);
  k_lb_write<<<gs, NB_TPB, 0, st>>>(indptr, g->indices, g->eid, V, seeds, cnt, fanout, keys_override, seed, (long long*)step_dev,
                                    key_layer, bump_step, ws->kept_map, out->indptr, out->pos, out->dst, out->eid, cap_b, bitmap, scr);
  k_nb_count<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, cap_k, tile_cnt, scr + 1);
  k_nb_number<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, tile_cnt, cap_k, ws->kept_nid, ws->kept_map);
  k_nb_tail<<<nb_grid(cap_b, NB_TPB, 2048), NB_TPB, 0, st>>>(g->indices, V, cnt, out->pos, ws->kept_map, out->src,
                                                             (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  k_nb_clean<<<nb_grid(cap_k, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, ws->kept_nid, cap_k, V, ws->kept_map,
                                                              (bf16_t*)ws->node_prob);
  return (int)hipGetLastError();
}

}  // extern "C"
