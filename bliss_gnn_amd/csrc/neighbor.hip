// The neighbor sampler on the device (fit.NeighborSampler with draw="device"): up to `fanout` in-edges per
// seed column, uniformly without replacement, as a keyed draw -- the defined-mode arrangement of csrc/mn_draw.hip with the key on
// the EDGE instead of the node.  The rule is normative, tests/neighbor_ref.py restates it on the CPU:
//
//   key(pos) = (uint32)(z >> 32),  z = SplitMix64 finaliser of md_key(seed, step, layer) ^ (uint64)pos       (integers only)
//   column s with CSC positions [a, b), d = b - a:  k = d if fanout < 0 or d <= fanout, else fanout
//   kept = the k smallest pairs (key(pos), pos); in the block they stand in ascending position at indptr[s] .. indptr[s] + k
//   sources: the seeds first (local ids 0 .. S-1, in the order given), then the other sources of kept edges in ascending node id
//
// bliss_neighbor_layer = six launches on one stream, no host round trip; S, E, B, K are read and written on the device:
//   k_nb_scan    one workgroup: seg_ptr (degrees), indptr (min(fanout, d)), S / E / B, the seeds into kept_nid and kept_map
//   k_nb_select  one workgroup per column: copy through, or a radix select of the 32-bit keys (4 passes of 8 bits, LDS bins,
//                keys recomputed from the hash in every pass) and an ordered pass that writes pos / dst / eid at indptr[s] + rank
//                and marks the edge's source, unless it is a seed, in a |V|-bit bitmap; the last workgroup (a ticket) bumps the step
//   k_nb_count   popcount per bitmap tile; the last workgroup (a ticket, k_md_pass's hand-over) scans the tile counts and writes K
//   k_nb_number  ordered numbering: new sources get kept_nid[S + rank] and kept_map; every bitmap word read here is left ZERO
//   k_nb_tail    src = kept_map[indices[pos]], unit weights
//   k_nb_clean   kept_map back to -1 at kept_nid[0 .. K); kept_nid[K .. cap_k) = 0 (capacity padding), node_prob = 1
// Counting uses integer LDS atomics and a global atomicOr into the bitmap; no output depends on the order in which they land.
// Every word a replay relies on (the two tickets, the bitmap, kept_map) is left zero / -1 by the kernel that used it; everything
// else is rewritten by every call before it is read.
#include "neighbor_tail.cuh"       // every kernel named above (shared with csrc/neighbor_w.hip and csrc/labor.hip), nb_mdkey, nb_scan64

extern "C" {

int64_t bliss_neighbor_scratch_bytes(int32_t num_nodes, int32_t cap_s) {
  if (num_nodes <= 0 || cap_s <= 0) return BLISS_EINVAL;
  const long long words = nb_bitmap_words(num_nodes);
  return (int64_t)(((NB_HDR + words + words / NB_TILE) * 4 + 15) & ~15ll);
}

int bliss_neighbor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                         int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer,
                         int bump_step, const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* scratch, void* stream) {
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
  unsigned* scr = (unsigned*)scratch;
  unsigned* bitmap = scr + NB_HDR;
  const long long words = nb_bitmap_words(V);
  const int n_tiles = (int)(words / NB_TILE);
  int* tile_cnt = (int*)(bitmap + words);
  const int gt = nb_grid(n_tiles, 1, 1024);
  k_nb_scan<<<1, NB_SCAN_TPB, 0, st>>>(indptr, V, seeds, n_seeds, n_seeds_dev, cap_s, fanout, cnt, ws->seg_ptr, out->indptr, cap_b,
                                       ws->kept_nid, ws->kept_map, cap_k);
  k_nb_select<<<nb_grid(cap_s, 1, 2048), NB_TPB, 0, st>>>(indptr, g->indices, g->eid, V, seeds, cnt, fanout, keys_override, seed,
                                                           (long long*)step_dev, layer, bump_step, ws->kept_map, out->indptr, out->pos,
                                                           out->dst, out->eid, cap_b, bitmap, scr);
  k_nb_count<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, cap_k, tile_cnt, scr + 1);
  k_nb_number<<<gt, NB_TPB, 0, st>>>(bitmap, n_tiles, cnt, tile_cnt, cap_k, ws->kept_nid, ws->kept_map);
  k_nb_tail<<<nb_grid(cap_b, NB_TPB, 2048), NB_TPB, 0, st>>>(g->indices, V, cnt, out->pos, ws->kept_map, out->src,
                                                             (bf16_t*)out->edge_weights, (bf16_t*)out->q_ij, cap_b);
  k_nb_clean<<<nb_grid(cap_k, NB_TPB, 1024), NB_TPB, 0, st>>>(cnt, ws->kept_nid, cap_k, V, ws->kept_map,
                                                              (bf16_t*)ws->node_prob);
  return (int)hipGetLastError();
}

}  // extern "C"
