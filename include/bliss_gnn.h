/* bliss_gnn.h -- C ABI of libbliss_gnn.so, the MI355X (gfx950) implementation of the BLISS-GNN
 * hot path: layer-wise bandit / LADIES block sampling, per-block weighted SpMM, EXP3 update.
 *
 * The reference (linhthi/BLISS-GNN) has no FFI of its own: its boundary is the Python protocol
 * between dgl.dataloading.DataLoader / Lightning and the sampler + model classes.
 * Each entry point below therefore names the reference METHOD whose body it replaces; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and is what
 * bliss_gnn_amd/_lib.py does.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it points to one of the small descriptor structs
 *     below, which live on the host and only carry device pointers and sizes;
 *   - "bf16" = raw bfloat16 bits (uint16_t), passed as void*;
 *   - node / edge ids are int32 (train_lightning.py:340-342 casts the graph to int32), CSC
 *     indptr is int64;
 *   - `stream` is a hipStream_t cast to void* (NULL = default stream); nothing here
 *     synchronises, allocates or frees: all entry points are graph-capturable;
 *   - return value: 0 on success, a hipError_t (> 0) from the runtime, or BLISS_E* (< 0).
 *     Data-dependent failures (capacity, non-finite weights) are reported through the `err`
 *     word of the per-layer counts record, read by the caller together with the sizes.
 */
#ifndef BLISS_GNN_H
#define BLISS_GNN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLISS_EINVAL (-1)

#define BLISS_MODE_BANDIT 0   /* EXP3 edge probabilities  (bandit_sampler.py) */
#define BLISS_MODE_LADIES 1   /* static edge weights      (ladies_sampler.py) */
#define BLISS_ROWSUM_SLOTS 32
#define BLISS_NORM_SCRATCH (2 + 3 * BLISS_ROWSUM_SLOTS)
#define BLISS_MODE_UNIFORM_NODES 4   /* OR-ed in: importance_sampling=False, p_j = [j has an out-edge] (bandit_sampler.py:77-81) */
#define BLISS_MODE_PARTIALS 8        /* OR-ed in (bliss_frontier_prob, binned pipeline only): stop after the per-source reduction --
                                      * a destination-range shard owns only some columns, so its sums over sources are PARTIAL:
                                      * seeds' sums in seed_acc (fifth int64 array), the others as (first position << 32 | node,
                                      * sum) in touched_key / touched_sum, their number in bin_cursor[n_bins]; exact Q.44 integers
                                      * that the source owners add up (bliss_gnn_amd/shard.py) */

/* The message graph g as the sampler sees it (train_lightning.py:373: CSC only). */
typedef struct {
  const int64_t* indptr;    /* [num_nodes + 1] */
  const int32_t* indices;   /* [num_edges] source of every in-edge, grouped by destination */
  const int32_t* eid;       /* [num_edges] edge id of every CSC position, or NULL = identity */
  int32_t num_nodes;
  int64_t num_edges;
} bliss_graph_t;

/* Dense per-node scratch, owned by one sampler, clean between calls
 * (local_id = -1, first_pos = 0xFFFFFFFF, acc_p2 = 0). */
typedef struct {
  int32_t* local_id;        /* [num_nodes] */
  uint32_t* first_pos;      /* [num_nodes] */
  uint64_t* acc_p2;         /* [num_nodes] */
} bliss_node_maps_t;

/* Per-layer counts record (device).  Layout fixed: 8 x int32 then one double. */
typedef struct {
  int32_t S, E, C, K, B;    /* seeds, frontier edges, candidates, kept nodes, block edges */
  int32_t err;              /* BLISS_ERR_* bits, 0 = ok */
  int32_t iters;            /* evaluations of the Poisson fixed point (bandit_sampler.py:396) */
  int32_t all_one;          /* 1 if C <= fanout (bandit_sampler.py:392) */
  double c;                 /* Poisson scale */
} bliss_layer_counts_t;

/* Per-layer workspace (all device memory, caller allocated). */
typedef struct {
  void* counts;             /* bliss_layer_counts_t */
  int32_t* seg_ptr;         /* [cap_s + 1] start of every seed's column in the frontier */
  void* seed_acc;           /* [72 * cap_s + 64 bytes] exact per-seed accumulators, column bases, per-seed coefficients, long-column list */
  int32_t* chunk_cnt;       /* [max(frontier_bound, cap_c) / 1024 + 2] */
  int32_t* cand_nid;        /* [cap_c] global id of every candidate, seeds first (ndata[NID]) */
  void* p;                  /* bf16 [cap_c] LADIES importance p_j */
  void* P;                  /* bf16 [cap_c] inclusion probability P_j */
  int32_t* new_id;          /* [cap_c] block-local id of a kept candidate, -1 otherwise */
  int32_t* kept_nid;        /* [cap_k] global id of every kept node (block srcdata[NID]) */
  void* node_prob;          /* bf16 [cap_k] srcdata['node_prob'] */
  int32_t* hist;            /* [32768] counts per bf16 bit pattern of p; zero on entry, left zero */
  int32_t* src_cnt;         /* [cap_k + 1] edges per block source / fill cursor of the by-source index, or NULL */
  int32_t cap_c, cap_k;
  /* Binned candidate pipeline (optional; n_bins = 0 selects the atomic passes, which need no extra memory).
   * n_bins: power of two <= 1024 with ceil(num_nodes / n_bins) * 12 bytes <= 64 KiB of LDS.  The buffers may be shared
   * by all layers of a call (they are dead once bliss_frontier_prob's kernels have run). */
  int32_t n_bins;
  int64_t bin_cap;          /* records per bin; a bin that overflows raises BLISS_ERR_CAP_CAND */
  int32_t* bin_cursor;      /* [n_bins + 1] */
  uint64_t* bin_rec;        /* [n_bins * bin_cap] frontier position (32) | source / n_bins (17) | bf16 term of p_j^2 (15) */
  uint32_t* bitmap;         /* [frontier_bound / 32 rounded up to 128 words, + 4] first appearances by frontier position */
  int32_t* word_prefix;     /* [2048 + same length] 2048 tile totals, then the exclusive popcount prefix of the bitmap words (per 4096-word tile) */
  uint64_t* touched_key;    /* [cap_c] (first position << 32 | source id) of every non-seed frontier source */
  uint64_t* touched_sum;    /* [cap_c] its exact sum */
  int32_t* span_seg;        /* [frontier_bound / 256 + 2] seed column in which every 256th frontier position lies */
  void* kept_rec;           /* [kept_rec_positions * 16 bytes] optional: bliss_build_block's first pass leaves its per-span kept-edge */
  int32_t* span_cnt;        /* [kept_rec_positions / 256 + 4]   lists here so that the second pass need not walk the frontier again; */
  int64_t kept_rec_positions; /* used when frontier_bound <= kept_rec_positions (a multiple of 1024), else ignored (NULL = never) */
  int32_t* kept_map;        /* [num_nodes] block-local id of a kept node, -1 everywhere on entry and on exit of
                               bliss_build_block; NULL = look kept sources up through local_id + new_id (two gathers) */
  int32_t* entry_flag;      /* optional: set to 1 by the first kernel of bliss_frontier_prob, i.e. once everything enqueued before
                               this layer has completed -- the hand-off bliss_flag_wait consumes on another stream */
  /* optional (binned pipeline only): fs_ticket != NULL (int32 device word, zero, left zero) makes the last workgroup of
     bliss_frontier_prob's final kernel compute the Poisson scale, and bliss_poisson_select skips its own scale launch; the
     other fs_* fields are then the fanout / eps / rng_ctl / uniforms_offset_dev / is_last / rng_cap_total arguments that
     bliss_poisson_select will be called with */
  int32_t* fs_ticket; int32_t fs_fanout, fs_is_last, fs_rng_cap, fs_reserved; double fs_eps; int32_t* fs_rng_ctl; int32_t* fs_layer_off;
  int32_t* block_ready_flag; /* optional: bliss_build_block raises it (bliss_flag_wait's protocol) as soon as the block's forward
                               arrays (indptr, src, dst, pos, eid, edge_weights, q_ij, counts) and the dense maps are final --
                               before the by-source index, which only a backward pass reads, is sorted */
} bliss_layer_ws_t;

/* The block (MFG) of one layer, CSR by destination, edges in frontier order. */
typedef struct {
  int32_t* indptr;          /* [cap_s + 1] */
  int32_t* src;             /* [cap_b] block-local source id */
  int32_t* dst;             /* [cap_b] block-local destination id (= seed index) */
  int32_t* pos;             /* [cap_b] CSC position in g of every block edge */
  int32_t* eid;             /* [cap_b] edata[dgl.EID] */
  void* edge_weights;       /* bf16 [cap_b] edata['edge_weights'] */
  void* q_ij;               /* bf16 [cap_b] edata['q_ij'] (bandit) / the static weight (ladies) */
  int32_t* t_indptr;        /* [cap_k + 1] by-SOURCE index of the same edges (the SpMM backward gathers through it), */
  int32_t* t_edge;          /* [cap_b]     ascending edge index inside a source; NULL = do not build it              */
  int32_t* t_scratch;       /* [cap_b]     scratch for building it (needs ws->src_cnt and cap_s <= 32768)            */
  int32_t cap_b;
} bliss_block_out_t;

int bliss_layer_counts_bytes(void);

/* Cross-stream ordering without an event (no reference counterpart).  An event between two kernels of one stream cuts a
 * captured HIP graph in two, and every graph launch costs ~20 us on the stream it is launched on; a flag does not.
 * Enqueues a one-wave kernel on `stream` that waits until *flag != 0 (raised through bliss_layer_ws_t.entry_flag), then
 * resets it to 0.  One producer and one consumer per flag and round.  The wait is bounded (~1 s): on a timeout bit 256
 * is OR-ed into *err_word (optional) and the stream continues. */
int bliss_flag_wait(int32_t* flag, int32_t* err_word, void* stream);
/* The bound of the waits enqueued from now on, in polls (~0.25 us each; default 2^22).  A loop whose flags wait on work that
 * contains collectives raises it: a peer rank's hiccup must not read as "the flag never came". */
int bliss_flag_set_spin_bound(int64_t spins);
/* Raise *flag from `stream` (a one-thread kernel).  The hot path raises its flags from kernels it runs anyway
 * (entry_flag); this entry point exists so that a caller can PROBE, with harmless kernels, whether a wait enqueued on one
 * stream and a raise enqueued later on another really run side by side (they do not when the two streams share a
 * hardware queue, or under a profiler that serialises kernels) before it relies on flags for ordering. */
int bliss_flag_raise(int32_t* flag, void* stream);

/* exp3_probabilities + BanditLadiesSampler.compute_prob      bandit_sampler.py:101-138, :47-82
 * LadiesSampler.compute_prob                                 ladies_sampler.py:34-52
 * In: seeds (unique); their count is n_seeds if >= 0, else *n_seeds_dev (e.g. the K of the previous
 * layer's counts record, so that consecutive layers need no host round trip); cap_s >= count sizes
 * seg_ptr / seed_acc.  w_pos: bf16 [num_edges] in CSC-position order -- the layer's
 * exp3_weights row (BANDIT) or g.edata['w'] (LADIES).  eta_f = (float)eta,
 * one_minus_eta_f = (float)(1.0 - eta).  frontier_bound >= number of in-edges of the seeds
 * (num_edges is always valid).  Out (in ws): counts{S,E,C}, seg_ptr, cand_nid, p; the node maps
 * hold local ids of all candidates until bliss_build_block cleans them.  More than cap_c candidates: error bit 2 and a list that
 * is invalid but complete below counts.C -- the seeds only (binned pipeline) or the first cap_c candidates (atomic passes). */
int bliss_frontier_prob(const bliss_graph_t* g, const bliss_node_maps_t* maps, const void* w_pos,
                        const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s, int mode,
                        float eta_f, float one_minus_eta_f, int64_t frontier_bound, const bliss_layer_ws_t* ws,
                        void* stream);

/* PoissonBanditLadiesSampler.compute_prob (scale c, :391-406) + select_neighbors (:408-425).
 * uniforms: fp32 [>= C], the values torch.rand(C) draws from the CPU generator (ATen's serial
 * Bernoulli kernel consumes the same 24-bit stream); the C numbers start at uniforms[*uniforms_offset_dev]
 * (NULL = 0).  With rng_ctl (bliss_rng_stream_begin) the call itself waits for the streaming generator and
 * writes the offset, exactly like bliss_rng_stream_wait.  Out: counts{K,c,iters,all_one}, P, new_id,
 * kept_nid, node_prob. */
int bliss_poisson_select(const bliss_layer_ws_t* ws, int32_t fanout, double eps, const float* uniforms,
                         int32_t* uniforms_offset_dev, int32_t* rng_ctl, int is_last, int32_t rng_cap_total,
                         int64_t cand_bound, void* stream);

/* bliss_poisson_select with a KEYED draw (draw="device" of the two Poisson samplers): the same two launches
 * (the scale, unless fs_ticket has it computed by bliss_frontier_prob; the select with its ordered look-back compaction), but the
 * uniform of candidate j is not read from a buffer:
 *   u_j = keyed_uniform(seed, *step_dev, layer, cand_nid[j])     SplitMix64 finaliser, top 24 bits, u = r * 2^-24 in [0, 1)
 *   j is kept iff u_j < float(P_j), P_j exactly bliss_poisson_select's (seeds and the all_one early-out: P = 1, always kept)
 * (oracle/bliss_oracle.py:keyed_uniform; the draw bliss_keyed_select makes for the sharded samplers).  No generator, rng_ctl or
 * uniforms offset takes part: with fs_ticket set, fs_rng_ctl and fs_layer_off must be NULL.  `layer`: the sampling layer mixed
 * into the key, 0 .. 255 (pass 0 for every layer to draw one variate per node and step: layer dependency).  bump_step != 0 (the
 * LAST select of a sampler call): the workgroup that draws the launch's last ticket -- every workgroup has read the step by then
 * -- writes *step_dev + 1, so a replayed graph advances the draw step; no extra launch, wait or spin.  step_dev: int64 device
 * word.  Everything else (outputs, clamps, error bits, cand_bound) as bliss_poisson_select.
 * BLISS_EINVAL, before any launch: ws or step_dev NULL, fanout < 0, layer outside 0 .. 255. */
int bliss_poisson_select_keyed(const bliss_layer_ws_t* ws, int32_t fanout, double eps, uint64_t seed, int64_t* step_dev,
                               int32_t layer, int bump_step, int64_t cand_bound, void* stream);

/* The non-Poisson samplers: `chosen` [n_chosen] = candidate-local ids drawn by select_neighbors
 * (torch.multinomial(prob, min(num, C)), bandit_sampler.py:98 / ladies_sampler.py:68 -- its random stream is MKL's
 * inside ATen's CPU kernel, so the draw itself stays with torch on the host, on the device-computed ws->p).  Marks
 * union(chosen, seeds) as block sources, only drawn nodes as edge sources (bandit_sampler.py:287-298), P = p (:309). */
int bliss_multinomial_select(const bliss_layer_ws_t* ws, const int32_t* chosen, int32_t n_chosen, void* stream);

/* The same samplers' draw ON THE DEVICE (draw="device"; no reference counterpart: a defined-mode keyed draw like
 * bliss_keyed_select, restated on the CPU by tests/mn_draw_ref.py).  The exponential race torch.multinomial runs on the CPU,
 * with counter-based uniforms:
 *   u_j   = keyed_uniform(seed, *step_dev, layer, cand_nid[j]) + 2^-24   (in (0, 1]; or uniforms[j] when uniforms != NULL)
 *   key_j = (float)(-log((double)u_j) / (double)p_j), +inf unless p_j > 0
 *   drawn = the k = min(fanout, C) smallest (bits of key_j, j), ties to the lower position; C = counts->C, read on the device.
 * Out: keys fp32 [cap_c] and drawn int32 [cap_c] (1 = drawn, 0 = not; entries [0, C) are written) -- the mark format
 * bliss_multinomial_select_marked reads from ws->new_id.  bump_step: the last workgroup of the first kernel increments
 * *step_dev once.  scratch: bliss_multinomial_draw_scratch_bytes(cap_c) bytes, 16-byte aligned, zero-initialised ONCE; every
 * call leaves it ready for the next (also when replayed from a captured graph).  Five launches, no host round trip.
 * BLISS_EINVAL: a null pointer (uniforms may be NULL; step_dev only with uniforms and without bump_step), fanout < 0,
 * cap_c <= 0, misaligned scratch. */
int64_t bliss_multinomial_draw_scratch_bytes(int32_t cap_c);
int bliss_multinomial_draw(const int32_t* cand_nid, const void* p_bf16, const void* counts, int32_t cap_c, int32_t fanout,
                           const float* uniforms, uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step, void* scratch,
                           float* keys, int32_t* drawn, void* stream);
/* The tail of bliss_multinomial_select for marks that are already in ws->new_id (1 = drawn, 0 = not, for the C candidates):
 * P = p (:309), union(drawn, seeds) numbered as block sources, kept_nid / node_prob / K.  No host-side count. */
int bliss_multinomial_select_marked(const bliss_layer_ws_t* ws, void* stream);

/* CLAMPED BLOCKS.  A static-shape step reads its error words only after its consumers (SpMM, GCN, GATv2, the EXP3 update, the
 * by-source index) have walked the block, so "clamped" must still mean "a block": invalid numbers, valid plumbing.  The following
 * holds for the outputs of every layer entry point below (bliss_neighbor_layer, bliss_wneighbor_layer, bliss_neighbor_replace_layer,
 * bliss_labor_layer, bliss_labor_is_layer, bliss_wlabor_layer), of the select calls above followed by bliss_build_block, and of
 * bliss_block_transpose on such a block -- WHETHER OR NOT an error bit is set.  (S, K, B, C) are the counts record.
 *   I1  0 <= S <= cap_s, 0 <= K <= cap_k, 0 <= B <= cap_b, C <= cap_c; BLISS_ERR_CAP_SEEDS / _KEPT / _EDGES / _CAND is set exactly
 *       when the unclamped count was larger, and the clamped count then equals its capacity.
 *   I2  indptr[0] = 0, indptr non-decreasing over [0, cap_s], indptr[S] = B, indptr[r] = B for S <= r <= cap_s.
 *   I3  for every e < B: dst[e] is the row r with indptr[r] <= e < indptr[r + 1]; 0 <= src[e] < K; 0 <= pos[e] < num_edges;
 *       eid[e] = g->eid[pos[e]] (pos[e] when g->eid == NULL).
 *   I4  kept_nid[0, K) are valid, pairwise distinct node ids, the first min(S, K) the layer's seeds in order; kept_nid[K, cap_k) = 0.
 *   I5  an edge is CONSISTENT if kept_nid[src[e]] = g->indices[pos[e]].  Only S, B or C clamped: every edge is.  K clamped: every
 *       edge whose true source is in kept_nid[0, K) is; the node-wise layers keep the others at source 0 (a seed: it exists wherever
 *       an edge does), the select + bliss_build_block chain does not emit them.  They need I3 only.
 *   I6  by-source index: t_indptr[0] = 0, non-decreasing over [0, cap_k], t_indptr[j] = B for K <= j <= cap_k; t_edge[0, B) is a
 *       permutation of 0 .. B-1; list j holds exactly the edges with src = j, in ascending edge index.
 *   I7  edge_weights[0, B), q_ij[0, B), p_ij[0, B) where the layer writes it, node_prob[0, cap_k): no NaN, no infinity.
 *   I8  what the next call (a replayed graph) relies on is as an unclamped call leaves it: kept_map and local_id all -1, the
 *       node-wise tickets and node bitmap, fs_ticket and (after a Poisson select, which consumes it) hist zero, the draw step
 *       bumped exactly once (bump_step) / the generator state advanced by the numbers the call's candidates took.
 * Nothing is written beyond a capacity.  tests/block_invariants.py states I1 - I7 in NumPy; tests/test_gpu_clamped_blocks.py holds
 * every kind of layer to them with each capacity of each layer one below the truth. */

/* dgl.dataloading.NeighborSampler(fanouts) ON THE DEVICE, one layer (fit.NeighborSampler with draw="device"; a defined-mode keyed
 * draw like bliss_multinomial_draw with the key on the EDGE, restated on the CPU by tests/neighbor_ref.py):
 *   key(pos) = (uint32)(z >> 32), z = SplitMix64 finaliser of mix(seed, *step_dev, layer) ^ (uint64)pos  -- bliss_multinomial_draw's
 *              (seed, step, layer) mixing with the CSC position in the node id's place; keys_override[pos] when keys_override != NULL
 *              (uint32 [num_edges], by CSC position: lets a test plant ties)
 *   seed column s, CSC positions [a, b), d = b - a:  k = d if fanout < 0 or d <= fanout, else fanout; kept = the k smallest pairs
 *              (key(pos), pos), ties to the lower position
 *   block:     edges column by column in seed order, ascending position inside a column; indptr[s + 1] - indptr[s] = k;
 *              sources = the seeds (local ids 0 .. S-1 in the order given), then the other sources of kept edges, each once, in
 *              ascending node id; edge_weights = q_ij = 1; eid = g->eid[pos], or pos when g->eid == NULL
 * Seeds (unique) and their count as in bliss_frontier_prob: n_seeds if >= 0, else *n_seeds_dev; cap_s >= count sizes seg_ptr / indptr.
 * Read from ws: counts, seg_ptr, kept_nid, kept_map, cap_k, node_prob (optional).  Read from out: indptr, src, dst, pos, eid, edge_weights, q_ij, cap_b
 * (the by-source index is not built here: bliss_block_transpose on out->src with the record's B).  Every other field is ignored.
 * Out: counts{S, E = sum d, C = K, K, B, err}, seg_ptr, kept_nid, the block arrays; capacity padding as bliss_build_block leaves it
 * (indptr rows S .. cap_s empty, kept_nid[K .. cap_k) = 0); ws->node_prob, when not NULL, = 1 for all cap_k entries.  A count beyond cap_s / cap_k / cap_b raises
 * the matching BLISS_ERR_CAP_* bit and is clamped; nothing is written beyond a capacity, and what is written is still a block
 * ("clamped blocks" above, I1 - I8).  ws->kept_map: [num_nodes], -1 everywhere
 * on entry and on exit.  bump_step: the last workgroup of the select kernel increments *step_dev once, after every workgroup has
 * read it.  scratch: bliss_neighbor_scratch_bytes(num_nodes, cap_s) bytes (cap_s > 0 is checked; nothing is sized by it), 16-byte aligned, zero-initialised ONCE; its words are
 * [0, 16) tickets, then the node bitmap (ceil(num_nodes / 32) words rounded up to a multiple of 1024) -- both left zero by every
 * call, also a replayed one -- then one offset per 1024 bitmap words, rewritten by every call.  Six launches, no host round trip.
 * BLISS_EINVAL before any launch: a null pointer (keys_override may be NULL; n_seeds_dev with n_seeds >= 0; step_dev only with
 * keys_override and without bump_step), cap_s <= 0, fanout == 0, ws->cap_k <= 0, num_edges > INT32_MAX, misaligned scratch. */
int64_t bliss_neighbor_scratch_bytes(int32_t num_nodes, int32_t cap_s);
int bliss_neighbor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                         int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer,
                         int bump_step, const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* scratch, void* stream);

/* bliss_neighbor_layer with edge probabilities: a WEIGHTED draw without replacement per seed column (fit.NeighborSampler(draw="device",
 * prob=...) and fit.BanditNeighborSampler; a defined-mode keyed exponential race, restated on the CPU by tests/wneighbor_ref.py;
 * DESIGN.md section 17).
 *   q_pos   = prob_pos[pos] (mode BLISS_WN_RAW: bf16 [num_edges] by CSC position, unnormalised, used as given), or
 *             eta / n_i + (1 - eta) * w_pos / sum_col(w) (mode BLISS_WN_EXP3: prob_pos = the EXP3 row w by CSC position; the
 *             roundings of bliss_frontier_prob's q_ij -- the column sum exact, rounded once to bf16, (1 / n_i) * eta and the product
 *             each rounded to bf16 -- with eta and one_minus_eta the fp32 values of eta and 1 - eta)
 *   u_pos   = ((key(pos) >> 8) + 1) * 2^-24 with bliss_neighbor_layer's key(pos); in (0, 1], exact in fp32
 *   key_pos = (float)(-log((double)u_pos) / (double)q_pos), the sign of zero dropped; +inf unless q_pos > 0 (a NaN q gives +inf);
 *             keys_override[pos] when keys_override != NULL (uint32 [num_edges]: fp32 bit patterns by CSC position)
 *   seed column s, CSC positions [a, b), d = b - a:  k = d if fanout < 0 or d <= fanout (a WHOLE column: no key is computed), else
 *             k = fanout and kept = the k smallest pairs (bits of key_pos, pos): an edge with q <= 0 is taken only as a filler
 *   block, sources, counts record {S, E, C = K, K, B, err}, capacity padding, clamps, BLISS_ERR_CAP_* bits, ws->kept_map, bump_step
 *             (here the last workgroup of the key kernel): bliss_neighbor_layer's.
 *   q_ij = q_pos for every kept edge, whole columns included; edge_weights = the Hajek weight under the mean aggregation,
 *             W_e = (1 / q_e) * k_s / sum_{kept e' of column s} (1 / q_e') from the bf16 q in fp64 (the sum in a fixed order, so a
 *             replay is bit-equal), rounded once to bf16; exactly 1 in a whole column and in a column that keeps an edge whose q is
 *             not a positive finite number; node_prob = 1.  EXP3 mode: a non-finite weight raises BLISS_ERR_NONFINITE.
 * keys_out (optional, a test hook: NULL in every product path): uint32 [num_edges]; the key bits of every position of a non-whole
 * seed column are stored there.  scratch: bliss_wneighbor_scratch_bytes(num_nodes, cap_s, num_edges) bytes, 16-byte aligned,
 * zero-initialised ONCE: bliss_neighbor_layer's words (tickets and bitmap left zero by every call, also a replayed one, one that
 * flagged an overflow and one with a seed id out of range; one offset per 1024 bitmap words), then cap_s per-seed records and
 * num_edges staged keys, rewritten by every call before they are read.  Eight launches, no host round trip.
 * BLISS_EINVAL before any launch: the set bliss_neighbor_layer refuses, prob_pos NULL or not 2-byte aligned, a mode other than the
 * two, keys_override / keys_out not 4-byte aligned, eta or one_minus_eta negative or NaN in EXP3 mode; the scratch size also
 * num_edges < 0 or > INT32_MAX. */
#define BLISS_WN_RAW 0
#define BLISS_WN_EXP3 1
int64_t bliss_wneighbor_scratch_bytes(int32_t num_nodes, int32_t cap_s, int64_t num_edges);
int bliss_wneighbor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                          int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer,
                          int bump_step, int32_t mode, const void* prob_pos, float eta, float one_minus_eta, uint32_t* keys_out,
                          const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* scratch, void* stream);

/* Draws WITH REPLACEMENT (csrc/replace_draw.hip; a defined-mode keyed categorical draw in integers only, restated on the CPU by
 * tests/replace_ref.py).  Shared by the two entry points below:
 *   fin(z)  = the SplitMix64 finaliser of bliss_neighbor_layer's key; mk = its mix(seed, *step_dev, layer)
 *   h       = fin(mk ^ (uint64)(uint32)ident); r_j = fin(h ^ ((uint64)(j + 1) * 0x9E3779B97F4A7C15)), the variate of draw j = 0, 1, ...
 *   weights of a group of bf16 probabilities: E = floor(log2(largest positive finite value)); w_i = floor(x_i * 2^(23 - E)) for a
 *             positive finite x_i, else 0 (<= 0, NaN, +-inf); the largest lands in [2^23, 2^24), values below 2^(E - 23) become 0 and
 *             are never drawn (the mode's resolution); W = sum w_i in uint64
 *   one draw over a group of m entries: W > 0: t = mulhi64(r_j, W), the pick is the smallest i whose inclusive prefix sum of w
 *             exceeds t (an entry of weight zero is never picked); W == 0, or no probabilities: the pick is mulhi64(r_j, m).
 *
 * bliss_neighbor_replace_layer: dgl.dataloading.NeighborSampler(fanouts, replace=True) on the device, one layer
 * (fit.NeighborSampler(draw="device", replace=True)), uniform (prob_pos == NULL) or with edge probabilities (prob_pos: bf16
 * [num_edges] by CSC position, unnormalised, as bliss_wneighbor_layer's raw mode).  ident = the node id of the seed column, so a
 * column's draws depend on (seed, step, layer, node id, j) and on nothing else.
 *   seed column s, CSC positions [a, a + d):  k_s = d if fanout < 0 (a WHOLE column: no draw), 0 if d == 0, else fanout -- also
 *             when d <= fanout; the drawn positions are a + pick_j, j < fanout
 *   block:     edges column by column in seed order, inside a column in ascending (position, j): repeats are separate, adjacent
 *             edges with the same pos and eid; indptr[s + 1] - indptr[s] = k_s, so B = sum k_s is known before the draw
 *   sources, eid / pos / dst, the counts record {S, E = sum d, C = K, K, B, err}, capacity padding, clamps, BLISS_ERR_CAP_* bits,
 *             ws->kept_map, node_prob = 1 and bump_step (the last workgroup of the draw kernel): bliss_neighbor_layer's.
 *   with prob_pos: q_ij = prob_pos[pos] on every edge; edge_weights W_e = (1 / q_e) * k_s / sum over the column's edges e', repeats
 *             counted, of (1 / q_e'), fp64 in a fixed order, rounded once to bf16 (1 / q is the exact per-draw importance weight);
 *             exactly 1 in a whole column and in a column that fell back to the uniform pick.  Without: edge_weights = q_ij = 1.
 * r_override (optional, a test hook that plants variates): uint64 [cap_s * fanout], r_j of column s at s * fanout + j.  picks_out
 * (optional, a test hook: NULL in every product path): int32 [cap_b], pick_j of every block edge (the index inside a whole column).
 * scratch: bliss_neighbor_replace_scratch_bytes(num_nodes, cap_s) bytes, 16-byte aligned, zero-initialised ONCE:
 * bliss_neighbor_layer's words, left idle by every call, also a replayed one and one that flagged an overflow.  Six launches, seven
 * with probabilities; no host round trip.
 * BLISS_EINVAL before any launch: the set bliss_neighbor_layer refuses (step_dev may be NULL only with r_override and without
 * bump_step), fanout > BLISS_NR_MAX_FANOUT (a column's draws are ordered in LDS), prob_pos / r_override / picks_out not aligned to
 * their element size (2 / 8 / 4 bytes). */
#define BLISS_NR_MAX_FANOUT 1024
int64_t bliss_neighbor_replace_scratch_bytes(int32_t num_nodes, int32_t cap_s);
int bliss_neighbor_replace_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev,
                                 int32_t cap_s, int32_t fanout, const uint64_t* r_override, uint64_t seed, int64_t* step_dev,
                                 int32_t layer, int bump_step, const void* prob_pos, int32_t* picks_out, const bliss_layer_ws_t* ws,
                                 const bliss_block_out_t* out, void* scratch, void* stream);

/* bliss_multinomial_draw WITH replacement (LadiesSampler / BanditLadiesSampler with draw="device-replace";
 * torch.multinomial(p, min(num, C), replacement=True) followed by the reference's union, which drops the duplicates): the rule
 * above over ONE group, the layer's C = counts->C candidates in the order of the candidate list with importances p_bf16, ident =
 * 0xFFFFFFFF (no node id), n = min(fanout, C) draws.
 * Out: drawn int32 [cap_c], entries [0, C): 1 if any draw picked the candidate, else 0 -- the mark format
 * bliss_multinomial_select_marked reads from ws->new_id.  r_override (optional, a test hook): uint64 [fanout].  picks_out
 * (optional, a test hook): int32 [fanout], entries [0, n) written.  bump_step: *step_dev is read once, by the one workgroup that
 * then increments it.  scratch: bliss_multinomial_draw_replace_scratch_bytes(cap_c) bytes, 16-byte aligned, zero-initialised ONCE;
 * every call leaves it ready for the next (also when replayed from a captured graph).  Three launches, no host round trip.
 * BLISS_EINVAL: a null pointer (r_override and picks_out may be NULL; step_dev only with r_override and without bump_step),
 * fanout < 0, cap_c <= 0, misaligned scratch, r_override / picks_out / drawn not aligned to their element size. */
int64_t bliss_multinomial_draw_replace_scratch_bytes(int32_t cap_c);
int bliss_multinomial_draw_replace(const void* p_bf16, const void* counts, int32_t cap_c, int32_t fanout, const uint64_t* r_override,
                                   uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step, void* scratch, int32_t* drawn,
                                   int32_t* picks_out, void* stream);

/* dgl.dataloading.LaborSampler(fanouts, importance_sampling=0) ON THE DEVICE, one layer (fit.LaborSampler; LABOR-0: a defined-mode
 * keyed draw like bliss_neighbor_layer with the key on the edge's SOURCE NODE and a per-column threshold instead of a per-column
 * select, restated on the CPU by tests/labor_ref.py).  Integers only:
 *   key(u)  = (uint32)(z >> 32), z = SplitMix64 finaliser of mix(seed, *step_dev, layer') ^ (uint64)u, u = g->indices[pos] --
 *             bliss_neighbor_layer's mixing; layer' = layer, or 0 for every layer when layer_dependency != 0 (the same variate per
 *             vertex in all layers of a step); keys_override[u] when keys_override != NULL (uint32 [num_nodes], by NODE ID)
 *   seed column s, CSC positions [a, b), d = b - a:  if fanout < 0 or d <= fanout every edge is kept and no key is computed;
 *             otherwise thr = ((uint64)fanout << 32) / d (integer division, 1 <= thr < 2^32) and the edge at pos is kept iff
 *             (uint64)key(indices[pos]) < thr.  The edges of a multi-edge are kept or dropped together; a column may keep NO edge.
 *   block:    edges column by column in seed order, ascending position inside a column; indptr[s + 1] - indptr[s] = c_s, the kept
 *             count of column s, B = sum c_s (data dependent: neither is known before the draw); sources = the seeds (local ids
 *             0 .. S-1 in the order given), then the other sources of kept edges, each once, in ascending node id;
 *             edge_weights = q_ij = 1 (every kept edge of a column has the same inclusion probability: the Hajek weight under the
 *             mean aggregation is exactly 1); eid = g->eid[pos], or pos when g->eid == NULL
 * Seeds, ws, out, the counts record {S, E = sum d, C = K, K, B, err}, the capacity padding, the clamps and BLISS_ERR_CAP_* bits,
 * ws->kept_map (-1 on entry and on exit) and bump_step (the last workgroup of the writing kernel increments *step_dev once, after
 * every workgroup has read it) are bliss_neighbor_layer's; no source is marked for an edge that was not written.  scratch:
 * bliss_labor_scratch_bytes(num_nodes, cap_s) bytes, 16-byte aligned, zero-initialised ONCE: bliss_neighbor_layer's words (tickets
 * and bitmap left zero by every call, also a replayed one and one that flagged an overflow; one offset per 1024 bitmap words) and
 * then cap_s words for c_s, rewritten by every call.  Seven launches, no host round trip.
 * BLISS_EINVAL before any launch: the set bliss_neighbor_layer refuses -- a null pointer (keys_override may be NULL; n_seeds_dev
 * with n_seeds >= 0; step_dev only with keys_override and without bump_step), cap_s <= 0, fanout == 0, ws->cap_k <= 0,
 * num_edges > INT32_MAX, misaligned scratch. */
int64_t bliss_labor_scratch_bytes(int32_t num_nodes, int32_t cap_s);
int bliss_labor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                      int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step,
                      int layer_dependency, const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* scratch, void* stream);

/* LABOR-i ON THE DEVICE, one layer (fit.ImportanceLaborSampler; the LABOR paper's importance iterations on bliss_labor_layer's keyed
 * per-source draw, restated on the CPU by tests/labor_is_ref.py).  Unsigned integers up to the weights, ONE = 2^32:
 *   seed column s, CSC positions [a, b), d = b - a, is WHOLE if fanout < 0 or d <= fanout: every edge is kept, no key is computed.
 *   Every position is its own term below (a multi-edge is m equal terms, kept or dropped as one).
 *   pi^(0)_u = ONE;  c_s(pi) = the largest c in [0, ONE - 1] with sum_pos (c * pi_{indices[pos]}) >> 32 <= fanout * ONE (non-whole columns)
 *   `iterations` (0 .. 8) times:  pi^(i+1)_u = max(1, max over the frontier edges u -> s of P),  P = ONE if s is whole, else
 *             (c_s(pi^(i)) * pi^(i)_u) >> 32 -- the maximum over the new values only; vertices outside the frontier are never read
 *   draw:     p_pos = (c_s(pi^(I)) * pi^(I)_u) >> 32 (< ONE); the edge at pos is kept iff (uint64)key(u) < p_pos, key = bliss_labor_layer's
 *             (keys_override by NODE ID, layer_dependency as there).  iterations = 0 is bliss_labor_layer's rule bit for bit.
 *   block, sources, counts record, capacity padding, clamps, BLISS_ERR_CAP_* bits, ws->kept_map, bump_step: bliss_labor_layer's.
 *   q_ij = bf16(fp32(p_pos) * 2^-32), both roundings to nearest even; edge_weights = the Hajek weight under the mean aggregation,
 *             W_e = (ONE / p_e) * k_s / sum_{kept e' of column s} (ONE / p_e'), k_s the column's kept count, evaluated in fp64 (the sum
 *             in a fixed order, so a replay is bit-equal) and rounded once to bf16; both exactly 1 in whole columns; node_prob = 1.
 * scratch: bliss_labor_is_scratch_bytes(num_nodes, cap_s, cap_b) bytes for cap_b = out->cap_b, 16-byte aligned, zero-initialised
 * ONCE: tickets, bitmap, tile offsets, TWO num_nodes-word importance buffers (pi - 1 per vertex) -- tickets, bitmap and both
 * buffers are left zero by every call, also a replayed one, one that flagged an overflow and one with a seed id out of range --
 * then cap_s kept counts, cap_s scales and cap_b words of p_e, rewritten by every call.  8 launches for iterations = 0, else
 * 2 * iterations + 9; no host round trip.  BLISS_EINVAL before any launch: the set bliss_labor_layer refuses, cap_b < 0 and
 * iterations outside 0 .. 8. */
int64_t bliss_labor_is_scratch_bytes(int32_t num_nodes, int32_t cap_s, int32_t cap_b);
int bliss_labor_is_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                         int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer,
                         int bump_step, int layer_dependency, int32_t iterations, const bliss_layer_ws_t* ws,
                         const bliss_block_out_t* out, void* scratch, void* stream);

/* LABOR WITH EDGE PROBABILITIES ON THE DEVICE, one layer (fit.WeightedLaborSampler -- dgl.dataloading.LaborSampler(fanouts, prob=...),
 * importance_sampling = 0 -- and fit.BanditLaborSampler; bliss_labor_layer's keyed per-source draw with a per-edge inclusion
 * probability proportional to q, clamped below ONE = 2^32; a defined mode restated on the CPU by tests/wlabor_ref.py; DESIGN.md
 * section 19).  Unsigned integers from the bf16 bits of q up to the weights:
 *   q_pos   = bliss_wneighbor_layer's: prob_pos[pos] (mode BLISS_WN_RAW: bf16 [num_edges] by CSC position, unnormalised), or the EXP3
 *             edge probability eta / n_i + (1 - eta) * w_pos / sum_col(w) with that entry point's roundings (mode BLISS_WN_EXP3)
 *   seed column s, CSC positions [a, b), d = b - a, is WHOLE if fanout < 0 or d <= fanout: every edge is kept, no key is computed.
 *   An edge of a non-whole column is VALID iff q_pos is positive and finite.  From the bf16 bits of q_pos (exponent field E, 7-bit
 *             mantissa M): m = E ? 128 + M : M, e = max(E, 1); e_max = the largest e over the column's valid edges;
 *             a_pos = (m << 24) >> (e_max - e), 0 when the shift is >= 32 and for an invalid edge (a_pos < ONE)
 *   p_pos(c) = min(ONE - 1, (c * a_pos) >> 24) in 64 bits; c_s = the largest c in [0, ONE - 1] with sum_pos p_pos(c) <= fanout * ONE,
 *             by 32 bisection steps from bit 31 down (the sum is nondecreasing in c; for c_s < ONE - 1 it exceeds
 *             fanout * ONE - 256 d).  A column with fewer than `fanout` edges whose a_pos reaches 2^24 ends at c_s = ONE - 1 and keeps
 *             fewer than `fanout` edges in expectation
 *   draw:     the edge at pos is kept iff (uint64)key(u) < p_pos(c_s), u = g->indices[pos], key = bliss_labor_layer's (keys_override by
 *             NODE ID, layer_dependency as there).  An edge with a_pos = 0 is never kept in a non-whole column (no filler rule)
 *   block, sources, counts record, capacity padding, clamps, BLISS_ERR_CAP_* bits, ws->kept_map, bump_step: bliss_labor_layer's.
 *   q_ij = q_pos for every kept edge, whole columns included; p_ij (bf16 [out->cap_b], a buffer of the caller's beside out->q_ij)
 *             = bf16(fp32(p_pos) * 2^-32), both roundings to nearest even, 1 in whole columns; edge_weights = the Hajek weight under
 *             the mean aggregation from the TRUE inclusion probability, W_e = (ONE / p_e) * k_s / sum_{kept e' of column s} (ONE / p_e'),
 *             in fp64 with bliss_labor_is_layer's order of summation, rounded once to bf16, 1 in whole columns; node_prob = 1.
 *             EXP3 mode: a non-finite weight raises BLISS_ERR_NONFINITE.
 * scratch: bliss_wlabor_scratch_bytes(num_nodes, cap_s, cap_b) bytes for cap_b = out->cap_b, 16-byte aligned, zero-initialised ONCE:
 * bliss_neighbor_layer's words (tickets, here also word 2 for pending error bits, and bitmap: all left zero by every call, also a
 * replayed one, one that flagged an overflow and one with a seed id out of range; one offset per 1024 bitmap words), then per seed
 * the (sum, eta / n) record, the (c_s, e_max) record and the kept count, and cap_b words of p_e, rewritten by every call before they
 * are read.  9 launches in raw mode, 10 in EXP3 mode; no host round trip.  BLISS_EINVAL before any launch: the sets
 * bliss_labor_layer and bliss_wneighbor_layer refuse (prob_pos NULL or not 2-byte aligned, a mode other than the two,
 * keys_override not 4-byte aligned, eta or one_minus_eta negative or NaN in EXP3 mode), p_ij NULL or not 2-byte aligned; the
 * scratch size: num_nodes <= 0, cap_s <= 0, cap_b < 0. */
int64_t bliss_wlabor_scratch_bytes(int32_t num_nodes, int32_t cap_s, int32_t cap_b);
int bliss_wlabor_layer(const bliss_graph_t* g, const int32_t* seeds, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t cap_s,
                       int32_t fanout, const uint32_t* keys_override, uint64_t seed, int64_t* step_dev, int32_t layer, int bump_step,
                       int layer_dependency, int32_t mode, const void* prob_pos, float eta, float one_minus_eta,
                       const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* p_ij, void* scratch, void* stream);

/* generate_block    bandit_sampler.py:269-339 (BANDIT: Hajek weights) / ladies_sampler.py:71-107.
 * Same g, maps, w_pos, seeds, eta as the matching bliss_frontier_prob call.  Out: counts{B}, the block;
 * leaves the node maps clean.  More than cap_b kept edges: BLISS_ERR_CAP_EDGES, B = cap_b, the block is the first cap_b kept edges
 * in frontier order -- indptr ends at cap_b, the by-source index is the index of those edges ("clamped blocks" above). */
int bliss_build_block(const bliss_graph_t* g, const bliss_node_maps_t* maps, const void* w_pos,
                      const int32_t* seeds, int32_t cap_s, int mode, float eta_f, float one_minus_eta_f,
                      int64_t frontier_bound, const bliss_layer_ws_t* ws, const bliss_block_out_t* out, void* stream);

/* at::mt19937 on the device: n = n_dev[n_word_offset] uniforms u = (r & 0xFFFFFF) * 2^-24 from the
 * generator state (uint32[626]: 624 state words, left, next -- the fields torch.get_rng_state()
 * exposes), advanced in place.  Same numbers as torch.rand(n) / torch.bernoulli draw on the CPU. */
int bliss_mt19937_uniform(void* state, const int32_t* n_dev, int32_t n_word_offset, float* out, int32_t cap, void* stream);

/* The same generator as ONE streaming kernel per sample_blocks call, on a library-owned side stream, so that the
 * serial MT19937 recurrence overlaps the sampling kernels (eagerly and inside a captured HIP graph):
 *   begin: fork the generator from `stream`; it writes uniforms into out[cap_total + 1248] in stream order, keeps the raw
 *          state blocks in raw[624 * (cap_total / 624 + 3)] and publishes its progress in ctl (int32[8]; [5] = "initialised for the current call");
 *   wait:  (per layer, on `stream`) block `stream` until the next C numbers exist, C = the layer's counts record;
 *          *layer_off = where they start in `out`; is_last tells the generator where to stop;
 *   end:   join, then advance `state` by exactly the number of draws the layers consumed; a stream that ran
 *          short or a generator that made no progress sets bit 128 in *err_word (a counts record's err). */
int bliss_rng_stream_begin(const void* state, int32_t* ctl, float* out, uint32_t* raw, int32_t cap_total, void* stream);
/* Optional, once per cap_total, outside any stream capture (allocates, copies): lets `begin` / `chain` generate the stream
 * of a call with SEVERAL workgroups -- MT19937 jump-ahead: the state n words ahead is a fixed GF(2) convolution of the word
 * sequence with t^(n-1) mod the generator's characteristic polynomial (csrc/mt_jump.hip) -- instead of one wave walking
 * the recurrence: same numbers, same out / raw layout.  plan4 = {first parallel block, blocks per stretch, stretches (0 =
 * serial), total blocks}; `out` and `raw` must then hold 624 * (total blocks + 2) elements.  BLISS_RNG_SERIAL=1 keeps the
 * serial generator.  bliss_mt_jump_poly (host only, no GPU): the 19937 coefficients of t^n_words mod phi as 624 uint32. */
int bliss_rng_prepare(int32_t cap_total, int32_t* plan4);
int bliss_mt_jump_poly(int64_t n_words, uint32_t* poly_words);
int bliss_rng_stream_wait(int32_t* ctl, const void* counts, int32_t* layer_off, int is_last, int32_t cap_total, void* stream);
int bliss_rng_stream_end(void* state, const int32_t* ctl, const uint32_t* raw, int32_t cap_total, int32_t* err_word,
                         void* stream);
/* For a loop that samples batch after batch without a host round trip (no reference counterpart: the reference syncs
 * at every draw): `end` of the generator started last and `begin` of the next one in ONE kernel on the generator's own
 * stream, ordered after everything enqueued on `stream` so far (the sampler that consumed the numbers).  That kernel also
 * copies the finished call's counts records (counts_dev, n_count_words int32, LayerCounts::err of the first record
 * receives bit 128 as in `end`) to counts_host, which must be pinned, device-visible host memory.  Nothing is enqueued on
 * `stream` except an event record.  The sampler that consumes the new generator needs no ordering after this call: its
 * first wait (bliss_poisson_select / bliss_rng_stream_wait) also waits for the control block to be the new one (ctl[5]).
 * `ready` (optional, stricter): make `stream` itself wait until that control block is initialised. */
int bliss_rng_stream_chain(void* state, int32_t* ctl, float* out, uint32_t* raw, int32_t cap_total, int32_t* counts_dev,
                           int32_t n_count_words, int32_t* counts_host, void* stream);
int bliss_rng_stream_ready(void* stream);
/* The library-owned generator stream as an integer (hipStream_t; created on first use), so that a caller can record an
 * event behind the kernels `chain` enqueued there -- e.g. to know when counts_host has been written. */
int64_t bliss_rng_stream_handle(void);

/* ---- destination-range shards (no reference counterpart: the reference is single-device) ----------
 * The by-source reduction of compute_prob (bandit_sampler.py:67-75) crosses shards; everything per candidate then happens at
 * the candidate's owner on plain lists:
 *   bliss_cand_importance: p_j = sqrt(bf16(exact sum)) (:75) from the summed Q.44 partials (uniform_nodes: [sum != 0], :79-81);
 *   bliss_poisson_scale:   the fixed point c of :391-401 from the GLOBAL histogram of p's bit patterns (hist int32[32768],
 *                          left zeroed) and the global candidate count counts->C; writes counts->{c, iters, all_one};
 *                          scratch: int32[(counts->C + 1023) / 1024 + 2], left zeroed;
 *   bliss_keyed_select:    P_j = seed ? 1 : min(c p_j, 1) (:403-406) and the Poisson draw u < P (:422-424) with the
 *                          counter-based uniform of (seed, step, layer, node id) -- SplitMix64 finaliser, top 24 bits -- since
 *                          shards cannot share torch's serial stream; keep[j] = 1 iff drawn. */
int bliss_cand_importance(const int64_t* sums, int32_t n, int uniform_nodes, void* p_bf16, int32_t* err, void* stream);
int bliss_poisson_scale(int32_t* hist, void* counts, int32_t fanout, double eps, int32_t* scratch, void* stream);
int bliss_keyed_select(const int32_t* nid, const void* p_bf16, const uint8_t* is_seed, int32_t n, const void* counts,
                       uint64_t seed, uint64_t step, int32_t layer, void* P_bf16, uint8_t* keep, void* stream);
/* The STATIC-SHAPE sharded sampler (csrc/shard_dense.hip, bliss_gnn_amd/shard_static.py): the same split as above with every
 * exchange made dense, so that a layer has ONE collective of a fixed shape and no size ever reaches the host:
 *   bliss_shard_local_seeds:      the seeds of the global list (n_seeds, or *n_seeds_dev when n_seeds < 0) that lie in [lo, hi),
 *                                 order kept -> seeds_l (padded to cap_s with the list's first entry: a block's destination ids at capacity;
 *                                 and a second, unpadded copy: what bliss_build_block's clean-up walks),
 *                                 seed_pos[i] = position in the global list (0 beyond the count), *n_local_dev;
 *   bliss_shard_zero_dense:       dense (int64 [2 * num_nodes]) to zero, by a kernel (once, after allocation: the calls below keep it zero
 *                                 between uses);
 *   bliss_shard_scatter_partials: into a ZERO dense buffer, scatters the per-source partial sums that
 *                                 bliss_frontier_prob(BLISS_MODE_PARTIALS) left (seeds: seed_p2; others: touched_key / touched_sum,
 *                                 their count in *n_touched_dev) into dense[2 v], with dense[2 v + 1] = 1 (+ 2^32 for a seed): sum and mark side by side.
 *                                 The caller all-reduces dense (integer sums: exact for any shard count, any order);
 *   bliss_shard_candidates:       candidates = nodes with a non-zero mark, ascending id: cand_nid, p_j = sqrt(bf16(sum)) (:75); every
 *                                 entry of dense it read goes back to zero (the next bliss_shard_scatter_partials finds it clean);
 *                                 is_seed, the histogram of p's bit patterns, counts->C -- one launch, the ordered compaction by decoupled
 *                                 look-back over one 64-bit status word per 1024 nodes.  scratch: 8-byte aligned, uint64[ceil(num_nodes /
 *                                 1024) + ceil(cap_c / 1024) + 1], zero-initialised once and SHARED with bliss_shard_select_kept (each of
 *                                 the two calls returns the other's words to zero, so they alternate: candidates, select, candidates ...);
 *   (bliss_poisson_scale on that histogram and counts)
 *   bliss_shard_select_kept:      P_j and the keyed draw (as bliss_keyed_select, the step read from *step_dev), kept list =
 *                                 the seeds in seed order, then the drawn non-seeds in node order: kept_nid, node_prob, kept_map
 *                                 [kept_nid[i]] = i, layer_counts->K, layer_counts->C = *n_local_dev (bliss_build_block's clean-up
 *                                 bound); scratch: the array bliss_shard_candidates was given (same num_nodes and cap_c; ONE more 64-bit word behind the
 *                                 status words: a ticket).  When the launch's last workgroup has finished: bump_step != 0 adds 1 to *step_dev
 *                                 (a sampler's last layer), done_flag (optional) is raised (bliss_flag_wait's protocol).
 * (source: bandit_sampler.py:47-82, 381-425; no reference counterpart for the split itself -- SURVEY.md section 8e) */
int bliss_shard_local_seeds(const int32_t* seeds_g, int32_t n_seeds, const int32_t* n_seeds_dev, int32_t lo, int32_t hi, int32_t cap_s,
                            int32_t* seeds_l, int32_t* seeds_l_copy, int32_t* seed_pos, int32_t* n_local_dev, int32_t* err, void* stream);
int bliss_shard_scatter_partials(const int32_t* seeds_l, const int64_t* seed_p2, const int32_t* n_local_dev, const int64_t* touched_key,
                                 const int64_t* touched_sum, const int32_t* n_touched_dev, int64_t* dense, int32_t num_nodes,
                                 int32_t* err, void* stream);
/* block inputs, owner side (train_lightning.py:138 over shards): out[i, :] = table[nid[i] - lo, :] for the rows i < *n_rows_dev whose
 * node this rank owns (lo <= nid[i] < hi), +0 bits elsewhere -- the zero-padded buffer the ranks then sum as integer words.  bf16 rows
 * of even length, 4-byte aligned. */
int bliss_shard_pack_rows(const int32_t* nid, const int32_t* n_rows_dev, int32_t cap_rows, int32_t lo, int32_t hi, const void* table_bf16,
                          int64_t table_stride, int32_t row_len, void* out_bf16, int64_t out_stride, void* stream);
/* rows between a rank's own list and a block's list (model.py:318-332 over shards: the inputs of the layers behind the first, the
 * destination rows h[:num_dst] of every layer, and the gradients on the way back).  pos[j], j < *n_dev (<= cap_s): the position of this
 * rank's j-th row in the block's list, ASCENDING.  bf16 rows of even length, 4-byte aligned (fp32 source: 8-byte).
 *   bliss_shard_place_rows: out[r, :] = src[j, :] where pos[j] == r, +0 bits for every other row r < n_rows -- the zero-padded buffer
 *                           that is then summed over the ranks as integer words, in one launch;
 *   bliss_shard_take_rows:  out[j, :] = bf16(src[pos[j], :]) for j < *n_dev (n_dev NULL: all cap_s rows), +0 bits behind; src is bf16,
 *                           or fp32 rounded to nearest even (the all-reduced gradient buffer). */
int bliss_shard_place_rows(const void* src_bf16, int64_t src_stride, const int32_t* pos, const int32_t* n_dev, int32_t cap_s, void* out_bf16,
                           int64_t out_stride, int32_t n_rows, int32_t row_len, void* stream);
int bliss_shard_take_rows(const void* src, int32_t src_is_f32, int64_t src_stride, int32_t n_src_rows, const int32_t* pos, const int32_t* n_dev,
                          int32_t cap_s, void* out_bf16, int64_t out_stride, int32_t row_len, void* stream);
int bliss_shard_zero_dense(int64_t* dense, int32_t num_nodes, void* stream);
int bliss_shard_candidates(int64_t* dense, int32_t num_nodes, int32_t uniform_nodes, int32_t* cand_nid, void* p_bf16, uint8_t* is_seed,
                           int32_t* hist, void* counts, int32_t cap_c, int32_t* scratch, int32_t* err, void* stream);
int bliss_shard_select_kept(const int32_t* cand_nid, const void* p_bf16, const uint8_t* is_seed, const void* counts, uint64_t seed,
                            int64_t* step_dev, int32_t layer, const int32_t* seeds_g, int32_t n_seeds, const int32_t* n_seeds_dev,
                            void* P_bf16, int32_t* kept_nid, void* node_prob_bf16, int32_t* kept_map, int32_t cap_k, int32_t cap_c,
                            int32_t num_nodes, void* layer_counts, const int32_t* n_local_dev, int32_t* scratch, int32_t bump_step,
                            int32_t* done_flag, int32_t* err, void* stream);
/* bliss_exp3_normalize with the norm taken from norm_limbs (int64[3 * BLISS_ROWSUM_SLOTS], e.g. the all-reduced row sums of
 * all shards) instead of row_sum; row_sum receives the exact sum of THIS row part after the division. */
int bliss_exp3_normalize_global(void* w_pos, int64_t num_edges, int64_t* row_sum, const int64_t* norm_limbs, int64_t* scratch,
                                void* norm_out_bf16, void* stream);

/* The Linear layers of dglnn.SAGEConv (model.py:303-308, 321-329; fc_neigh / fc_self) on the matrix cores, one launch:
 *   out[r, :] = epilogue( A1[r, :] . W1^T (+ A2[r, :] . W2^T) + bias ),   r < min(m_bound, *m_dev)
 * bf16 in, fp32 accumulation (v_mfma_f32_32x32x16_bf16), one rounding to bf16; W as nn.Linear stores it ([n, k], row stride
 * w_stride elements).  ids != NULL: row r of A1 is a1[ids[r]] (the feature gather of train_lightning.py:138 as the operand
 * load); a_copy (optional) receives those rows (the weight gradients need them).  in_norm / out_norm (optional): bf16 row
 * norms of the A1 rows / of the stored output rows (model.py:318-320), in bliss_embed_norm's summation order.  relu,
 * drop_p > 0 (drop_ctr: device uint64[2] launch counter + ticket, zero-initialised; drop_seed): model.py:330-332.  Rows at or
 * beyond *m_dev (capacity padding) are written as zeros.  k1, k2 <= 1024, n <= 256.  Two argument sets may share one launch. */
typedef struct {
  const void* a1; int64_t a1_stride; const int32_t* ids;
  const void* w1; int64_t w1_stride; int32_t k1;
  const void* a2; int64_t a2_stride; const void* w2; int64_t w2_stride; int32_t k2;
  const void* bias;
  int32_t m_bound; const int32_t* m_dev; int32_t n;
  void* out; int64_t out_stride;
  void* a_copy; int64_t copy_stride;
  void* in_norm; void* out_norm;
  int32_t relu; float drop_p; uint32_t drop_seed; void* drop_ctr;
} bliss_tile_gemm_t;
int bliss_tile_gemm(const bliss_tile_gemm_t* first, const bliss_tile_gemm_t* second_or_null, void* stream);
/* bliss_tile_gemm with 1 <= k1 <= BLISS_WIDE_MAX_K and 0 <= k2 <= BLISS_WIDE_MAX_K (a Cora-like input layer: 1433 columns); every other
 * limit and argument check is bliss_tile_gemm's (n <= 256, BLISS_EINVAL before any launch).  A workgroup walks K in panels of 1024
 * columns, the last one shorter, ONE operand panel in LDS at a time (66 KB plus the W slab at any K); the fp32 accumulators stay in
 * registers across the panels and across both products, one rounding to bf16 at the end.  The k order is bliss_tile_gemm's with
 * unbounded LDS: ascending 16-steps, operand 1 before operand 2.  At k1, k2 <= 1024 it runs one panel per operand and returns the
 * BITS of bliss_tile_gemm on the same arguments (out, in_norm, out_norm, a_copy, zero rows, dropout from an equal counter) -- also
 * where bliss_tile_gemm refuses k1 + k2 for its LDS.  in_norm is bit-equal to bliss_embed_norm of the rows at every K (per-lane
 * partial sums carried over the panels, one butterfly), a_copy receives every panel.  The alignment fast paths are chosen per
 * panel on the panel's base pointer and width: a misaligned or odd-length operand changes no bit (it is staged element-wise). */
#define BLISS_WIDE_MAX_K 16384
int bliss_tile_gemm_wide(const bliss_tile_gemm_t* first, const bliss_tile_gemm_t* second_or_null, void* stream);

/* The BACKWARD products of those Linear layers on the matrix cores (csrc/sage_bwd.hip) -- what autograd derives for
 * fc_neigh / fc_self of dglnn.SAGEConv (model.py:303-308, 321-329); W = [out, in] as nn.Linear stores it.
 *   bliss_sage_dgrad:  out[r, :] = A1[r, :] . W1 (+ A2[r, :] . W2 for r < min(m2_bound, *m2_dev)),  r < min(m_bound, *m_dev):
 *                      the gradient w.r.t. a layer's input rows -- A = gradient rows [m, k], W = [k, n] (k = the layer's out
 *                      features <= 256, n = its in features), fp32 accumulation over both products, one rounding to bf16;
 *                      rows at or beyond *m_dev are written as zeros.
 *   bliss_sage_wgrad:  for up to two problems in one launch pair:  dW[n, c] = sum_r D[r, n] X[r, c]  (bf16 [n_out, k_in]) and,
 *                      with db != NULL, db[n] = sum_r D[r, n]; r < min(rows_bound, *rows_dev); n_out <= 256.  fp32 partial
 *                      tiles per chunk of rows in `partials` (bliss_sage_wgrad_workspace floats, 16-byte aligned), summed in
 *                      chunk order and rounded once: bitwise reproducible. */
typedef struct {
  const void* a1; int64_t a1_stride; const void* w1; int64_t w1_stride; int32_t k1;
  const void* a2; int64_t a2_stride; const void* w2; int64_t w2_stride; int32_t k2; int32_t m2_bound; const int32_t* m2_dev;
  int32_t m_bound; const int32_t* m_dev; int32_t n;
  void* out; int64_t out_stride;
} bliss_dgrad_t;
int bliss_sage_dgrad(const bliss_dgrad_t* args, void* stream);
/* bliss_sage_dgrad with k1, k2 <= 1024: the input gradient of a GATv2 layer's fc_src / res_fc, whose gradient rows have
 * heads * head_dim columns (csrc/sage_bwd.hip: the same kernel, its k-loop run further; the existing entry point and its bits are
 * untouched).  BLISS_EINVAL when both staged operands and a W slab do not fit a workgroup's 160 KiB of LDS. */
int bliss_gat_dgrad(const bliss_dgrad_t* args, void* stream);
/* The same kernel with its k walked in panels of 1024 (rows of W, which is [k, n] here): 1 <= k1 <= BLISS_WIDE_MAX_K,
 * 0 <= k2 <= BLISS_WIDE_MAX_K, one operand panel in LDS at a time, so no k1 + k2 is refused for LDS.  The weight-first forward product
 * of a wide input layer (A = the feature rows, k = in_feats) and any out = A . W with a long reduction.  Same argument checks, same k
 * order; at k1, k2 <= 1024 the bits of bliss_gat_dgrad. */
int bliss_dgrad_wide(const bliss_dgrad_t* args, void* stream);
typedef struct {
  const void* d; int64_t d_stride; int32_t n_out;
  const void* x; int64_t x_stride; int32_t k_in;
  int32_t rows_bound; const int32_t* rows_dev;
  void* dw; int64_t dw_stride; void* db;
} bliss_wgrad_t;
int64_t bliss_sage_wgrad_workspace(const bliss_wgrad_t* probs, int32_t n_probs);
int bliss_sage_wgrad(const bliss_wgrad_t* probs, int32_t n_probs, float* partials, int64_t partial_floats, void* stream);

/* nn.CrossEntropyLoss() (mean) on bf16 logits [n_rows, n_cls] and int64 labels (train_lightning.py:77-79, :142), forward and
 * gradient in one launch: *loss_out = mean_r (logsumexp(x_r) - x_r[y_r]) in fp32, dlogits = (softmax(x) - onehot(y)) / n_rows in
 * bf16.  row_loss: float[n_rows] scratch; ticket: zero-initialised uint32 (left zero); a label outside [0, n_cls) sets bit 2 in *err. */
int bliss_cross_entropy(const void* logits, int64_t stride, const int64_t* labels, int32_t n_rows, int32_t n_cls,
                        float* row_loss, void* dlogits, int64_t d_stride, float* loss_out, uint32_t* ticket, int32_t* err,
                        void* stream);
/* The same with the two launches in front of it taken in: logits2 != NULL: the logits are bf16(logits + logits2) -- the output
 * layer's `rst = fc_self + h_neigh` (model.py:321-329); dlogits is then the gradient of both addends.  label_ids != NULL: row r's
 * label is label_table[label_ids[r]] -- mfgs[-1].dstdata['labels'] (train_lightning.py:139) without the gather.  At least one
 * of the two must be given. */
int bliss_cross_entropy_sum(const void* logits, int64_t stride, const void* logits2, int64_t stride2, const int64_t* label_table,
                            const int32_t* label_ids, int32_t n_rows, int32_t n_cls, float* row_loss, void* dlogits, int64_t d_stride,
                            float* loss_out, uint32_t* ticket, int32_t* err, void* stream);
/* The same for a rank of a sharded step (train_lightning.py:139-142 over destination-range shards): only the first *n_rows_dev of
 * the n_rows (capacity) rows are this rank's output seeds -- the others get a zero gradient row and no loss --, the labels are
 * label_table[label_ids[r] - id_off] (global node ids into the owner's table of n_table rows), and the divisor is `denom` (the
 * GLOBAL batch): *loss_out = sum_r loss_r / denom, so that the ranks' losses and gradients ADD to the global mean.  logits2 may be
 * NULL. */
int bliss_cross_entropy_masked(const void* logits, int64_t stride, const void* logits2, int64_t stride2, const int64_t* label_table,
                               int32_t n_table, const int32_t* label_ids, int32_t id_off, int32_t n_rows, const int32_t* n_rows_dev,
                               float denom, int32_t n_cls, float* row_loss, void* dlogits, int64_t d_stride, float* loss_out,
                               uint32_t* ticket, int32_t* err, void* stream);

/* The same under a LIVE row count: n_rows is the capacity (the launch bound) and, with
 * n = min(max(*n_rows_dev, 0), n_rows), rows r < n get exactly the loss term and gradient row bliss_cross_entropy_sum produces
 * when called with n_rows = n -- the divisor is n, formed on the device; the rounding points and the fixed order of the final sum
 * are the same, so *loss_out and gradient rows 0 .. n-1 are bit-equal to that call.  Rows r >= n get a zero gradient row and
 * nothing of their logits, label ids or labels is read.  n == 0: *loss_out = 0 and all-zero gradients, no NaN.  One launch, no
 * host read, capturable: one captured launch serves every batch size up to n_rows.  Error bits and BLISS_EINVAL cases are
 * bliss_cross_entropy_sum's; n_rows_dev == NULL is BLISS_EINVAL too. */
int bliss_cross_entropy_live(const void* logits, int64_t stride, const void* logits2, int64_t stride2, const int64_t* label_table,
                             const int32_t* label_ids, int32_t n_rows, const int32_t* n_rows_dev, int32_t n_cls, float* row_loss,
                             void* dlogits, int64_t d_stride, float* loss_out, uint32_t* ticket, int32_t* err, void* stream);

/* nn.BCEWithLogitsLoss() (mean; no weight, no pos_weight: train_lightning.py:77-79 for the multi-label dataset, load_graph.py:69-71)
 * on bf16 logits [n_rows, n_cls] and fp32 targets [n_rows, n_cls] (rows contiguous), forward and gradient in one launch, in fp32 from
 * e = exp(-|x|): *loss_out = mean (max(x, 0) - x y + log1p(e)), dlogits = bf16((sigmoid(x) - y) / (n_rows n_cls)), one rounding.
 * Logits of any magnitude give a finite gradient; an infinite logit gives the limit values (loss 0 where the target agrees with it
 * entirely, infinite elsewhere); NaN propagates.  row_loss: float[n_rows] scratch; ticket: zero-initialised uint32 (left zero). */
int bliss_bce_logits(const void* logits, int64_t stride, const float* targets, int32_t n_rows, int32_t n_cls, float* row_loss,
                     void* dlogits, int64_t d_stride, float* loss_out, uint32_t* ticket, int32_t* err, void* stream);
/* The same with the two launches in front of it taken in, as bliss_cross_entropy_sum: logits2 != NULL: the logits are
 * bf16(logits + logits2), dlogits the gradient of both addends; label_ids != NULL: row r's targets are row label_ids[r] of
 * target_table ([V, n_cls] floats, rows contiguous).  At least one of the two must be given. */
int bliss_bce_logits_sum(const void* logits, int64_t stride, const void* logits2, int64_t stride2, const float* target_table,
                         const int32_t* label_ids, int32_t n_rows, int32_t n_cls, float* row_loss, void* dlogits, int64_t d_stride,
                         float* loss_out, uint32_t* ticket, int32_t* err, void* stream);
/* The same for a rank of a sharded step, as bliss_cross_entropy_masked: only the first *n_rows_dev of the n_rows (capacity) rows
 * count -- the others get a zero gradient row and no loss, whatever their logits hold --, row r's targets are row
 * label_ids[r] - id_off of the owner's target_table (n_table rows; an id outside it sets bit 2 in *err and the row counts for
 * nothing), and the divisor is `denom`, the GLOBAL number of (row, class) pairs (batch x world x n_cls): the ranks' losses and
 * gradients ADD to the global mean.  logits2 may be NULL. */
int bliss_bce_logits_masked(const void* logits, int64_t stride, const void* logits2, int64_t stride2, const float* target_table,
                            int32_t n_table, const int32_t* label_ids, int32_t id_off, int32_t n_rows, const int32_t* n_rows_dev,
                            float denom, int32_t n_cls, float* row_loss, void* dlogits, int64_t d_stride, float* loss_out,
                            uint32_t* ticket, int32_t* err, void* stream);

/* The same under a LIVE row count, as bliss_cross_entropy_live: with n = min(max(*n_rows_dev, 0), n_rows), rows r < n get the
 * loss terms and gradient row of bliss_bce_logits_sum called with n_rows = n (divisor (float)n * (float)n_cls, formed on the
 * device as the host forms it), bit for bit; rows r >= n get a zero gradient row and nothing of theirs is read; n == 0: loss 0,
 * zero gradients, no NaN.  Error bits and BLISS_EINVAL cases are bliss_bce_logits_sum's; n_rows_dev == NULL is BLISS_EINVAL too. */
int bliss_bce_logits_live(const void* logits, int64_t stride, const void* logits2, int64_t stride2, const float* target_table,
                          const int32_t* label_ids, int32_t n_rows, const int32_t* n_rows_dev, int32_t n_cls, float* row_loss,
                          void* dlogits, int64_t d_stride, float* loss_out, uint32_t* ticket, int32_t* err, void* stream);

/* Micro-F1 (torchmetrics Multiclass / MultilabelF1Score(average='micro'), train_lightning.py:68-70, :143, :179-203) as counts on
 * the device: one launch ADDS this batch's {tp, fp, fn, n} to counts[0..3] (int64; never overwritten) with 64-bit integer atomics,
 * at most one per workgroup and counter -- integer adds commute, so the result does not depend on the schedule.  Nothing allocates,
 * syncs or reads back; the kernels keep no state besides counts and err, so a captured launch replays as it is.
 *
 *   logits       bf16 [*, n_cls], row stride `stride` (>= n_cls) elements; n_pred_rows: how many rows it holds (0 = not checked)
 *   row_ids      NULL: row r reads logits row r.  int32 [n_rows]: row r reads logits row row_ids[r] (pred[nid] never materialised)
 *   labels       direct: row r's label is labels[r]  (int64 [n_rows] / fp32 [n_rows, n_cls], rows contiguous)
 *   label_table, label_ids   or: row r's label is label_table[label_ids[r]] (int32 ids; n_table rows, 0 = not checked) -- the form
 *                bliss_cross_entropy_sum / bliss_bce_logits_sum take.  Exactly one of the two forms must be given.
 *   n_rows       host bound (and launch size); n_rows_dev != NULL: only the first min(max(*n_rows_dev, 0), n_rows) rows count
 *                (the convention of the masked losses); nothing of the other rows is read.
 *
 * The rule (normative):
 *   single-label  The prediction of a row is the FIRST index of its largest logit.  A NaN logit counts as larger than everything
 *                 and the first NaN wins (torch.argmax).  +0 and -0 are equal.  A row of -inf predicts 0.  A correct row adds
 *                 tp += 1, a wrong row fp += 1 and fn += 1, every counted row n += 1.  A label outside [0, n_cls) sets bit 2 of
 *                 *err and the row is left out of all four counts (the loss's "no loss term"); so does a label id outside a
 *                 checked table or a row id outside a checked prediction.
 *   multi-label   Per (row, class) pair: hit = x > 0, y = target > 0.5; tp = hit & y, fp = hit & !y, fn = !hit & y; n += n_cls per
 *                 counted row.  x > 0 is the exact statement of sigmoid(x) > 0.5 (a sigmoid evaluated in fp32 rounds to 0.5 for
 *                 0 < x < 2^-23: the one difference to such an implementation).  NaN is no hit and no positive target; x = +-0 is
 *                 no hit.  Ids outside a checked table / prediction: as above.
 *   micro-F1 = 2 tp / max(2 tp + fp + fn, 1).
 *
 * Launch shape: single-label one wave per row (256 threads = 4 rows per workgroup), multi-label one thread per pair; both loop
 * with the grid as stride under a cap of BLISS_F1_MAX_WORKGROUPS workgroups (4096 rows / 262144 pairs per trip).
 * BLISS_EINVAL before any launch: logits, counts or err NULL, n_cls <= 0, n_rows < 0, stride < n_cls, n_pred_rows or n_table < 0,
 * neither or both label forms.  n_rows == 0 launches nothing and returns 0. */
#define BLISS_F1_MAX_WORKGROUPS 1024
int bliss_f1_multiclass(const void* logits, int64_t stride, int32_t n_pred_rows, const int32_t* row_ids, const int64_t* labels,
                        const int64_t* label_table, int32_t n_table, const int32_t* label_ids, int32_t n_rows,
                        const int32_t* n_rows_dev, int32_t n_cls, int64_t* counts, int32_t* err, void* stream);
int bliss_f1_multilabel(const void* logits, int64_t stride, int32_t n_pred_rows, const int32_t* row_ids, const float* labels,
                        const float* label_table, int32_t n_table, const int32_t* label_ids, int32_t n_rows,
                        const int32_t* n_rows_dev, int32_t n_cls, int64_t* counts, int32_t* err, void* stream);

/* th.optim.Adam(self.parameters(), lr) (train_lightning.py:205-206) for a bf16 module: parameters, gradients and both moment
 * buffers bf16, one launch over all tensors, math in fp32, one rounding per stored value.  state: float[4] on the device --
 * [0] step count (incremented by the launch), [1] learning rate (the caller rewrites it when its scheduler does,
 * train_lightning.py:208: a captured graph keeps working), [2] internal ticket (zero-initialised). */
#define BLISS_ADAM_MAX_TENSORS 32
typedef struct {
  void* param[BLISS_ADAM_MAX_TENSORS];
  const void* grad[BLISS_ADAM_MAX_TENSORS];
  void* exp_avg[BLISS_ADAM_MAX_TENSORS];
  void* exp_avg_sq[BLISS_ADAM_MAX_TENSORS];
  int64_t numel[BLISS_ADAM_MAX_TENSORS];
  int32_t count;
} bliss_adam_t;
int bliss_adam_step(const bliss_adam_t* tensors, float* state, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* Step ledger (csrc/ledger.hip): ONE launch of one 64-thread workgroup at the end of a train step folds the finished step into a
 * device-resident record -- the epoch's loss sum, the reference's sampled-size averages (train_lightning.py:76-136), high-water
 * marks, the OR of the sampler's error words and an early warning -- so that a loop of replayed steps needs no host read per step.
 * Plain fixed-order arithmetic, no atomics, no flags; every pointer is fixed at launch and every value read is on the device, so
 * the launch sits inside a captured graph.
 *
 * The record (8-byte aligned; L = n_layers; bliss_step_ledger_bytes(L) = 80 + 16 L + 8 ceil(12 L / 8) bytes):
 *   offset  0  uint64 steps_epoch        16  double loss_last         32  uint64 nonfinite        48  int64 first_bad_step
 *           8  uint64 steps_total        24  double loss_sum          40  double cum_out          56  int64 first_near_step
 *          64  int32 err     68  int32 near     72  int32 n_layers (the caller's; not read)     76  int32 reserved
 *          80  double cum_nodes[L], double cum_edges[L], int32 hw_K[L], int32 hw_B[L], int32 hw_E[L], zero padding to 8 bytes
 * A fresh record is all zero except first_bad_step = first_near_step = -1 (and n_layers).  Layers are in SAMPLING order, the
 * order of the counts record.
 *
 * The rule (normative; restated by tests/ledger_ref.py) -- mode BLISS_LEDGER_STEP, counts = bliss_layer_counts_t[L]:
 *   loss_last = the loss widened exactly to fp64;  loss_sum += loss_last (one fp64 add);  nonfinite += 1 if it is not finite
 *   cum_nodes[n] = cum_nodes[n] * w + (double)K_n;  cum_edges[n] = cum_edges[n] * w + (double)B_n;
 *   cum_out = cum_out * w + (double)S_0            -- an fp64 product, then an fp64 sum, never fused
 *   hw_K[n], hw_B[n], hw_E[n] = running maxima of K_n, B_n, E_n
 *   e = OR of every layer's err word;  err |= e;  first_bad_step = steps_total (before its increment) at the first step with e != 0
 *   near = 1 once any (double)K_n > regrow_at * (double)cap_K_n or (double)B_n > regrow_at * (double)cap_B_n;
 *                                         first_near_step = steps_total (before its increment) at the first such step
 *   steps_epoch += 1;  steps_total += 1
 * mode BLISS_LEDGER_RESET_EPOCH: steps_epoch = 0, loss_sum = 0, nonfinite = 0, nothing else (only `ledger` is read).
 * mode BLISS_LEDGER_REARM: near = 0, first_near_step = -1, nothing else (after the capacities were re-fixed).
 *
 * caps: HOST array int32 [3 L] = {cap_K, cap_B, cap_E} per layer, taken by value at the call (cap_E takes part in no comparison:
 * E sizes launch grids only).  loss_dtype: BLISS_LEDGER_LOSS_BF16 / _F32, one scalar on the device.
 * BLISS_EINVAL before any launch: ledger NULL; n_layers outside 1 .. BLISS_LEDGER_MAX_LAYERS; an unknown mode; in mode STEP loss,
 * counts or caps NULL or an unknown loss_dtype.  bliss_step_ledger_bytes: BLISS_EINVAL for n_layers outside that range. */
#define BLISS_LEDGER_MAX_LAYERS 8
#define BLISS_LEDGER_STEP 0
#define BLISS_LEDGER_RESET_EPOCH 1
#define BLISS_LEDGER_REARM 2
#define BLISS_LEDGER_LOSS_BF16 0
#define BLISS_LEDGER_LOSS_F32 1
int bliss_step_ledger_bytes(int n_layers);
int bliss_step_ledger(int mode, const void* loss, int loss_dtype, const int32_t* counts, int n_layers, const int32_t* caps,
                      double w, double regrow_at, void* ledger, void* stream);

/* Batch statistics (csrc/ledger.hip): ONE launch of one wave folds the finished step's input-layer source
 * count into a 32-byte device record -- the running mean and variance BatchSizeCallback keeps on the host
 * (train_lightning.py:425-486), so that a loop of replayed steps can steer its batch size from one read per epoch.
 *
 * The record (8-byte aligned, BLISS_BATCH_STATS_BYTES):  0 uint64 n    8 double m    16 double s    24 uint64 reserved (zero)
 * A fresh record is all zero.
 *
 * The rule (normative; restated by tests/batch_stats_ref.py) -- mode BLISS_BATCH_STATS_PUSH, counts = bliss_layer_counts_t[],
 * x = (double)K of record `layer` (the LAST-sampled layer is the input layer: mfgs[0].num_src_nodes(), :467):
 *   n += 1;  m_old = m;  m += (x - m_old) / (double)n;  s += (x - m_old) * (x - m)
 * -- a difference, a quotient, a sum, a difference, a product, a sum: separate fp64 operations, never fused (:437-441 in Python
 * floats give the same bits).  mode BLISS_BATCH_STATS_CLEAR: the record is zeroed (only `record` is read).
 * The step ledger's record, its size and bliss_step_ledger are untouched by this.
 * BLISS_EINVAL before any launch: record NULL; an unknown mode; in mode PUSH counts NULL or layer outside
 * 0 .. BLISS_LEDGER_MAX_LAYERS - 1. */
#define BLISS_BATCH_STATS_BYTES 32
#define BLISS_BATCH_STATS_PUSH 0
#define BLISS_BATCH_STATS_CLEAR 1
int bliss_batch_stats(int mode, const int32_t* counts, int layer, void* record, void* stream);

/* normalized_edata    bandit_sampler.py:20-27: w_pos[p] = bf16(1 / bf16(indeg(dst(p)))). */
int bliss_normalized_edata(const bliss_graph_t* g, void* w_pos, void* stream);

/* Feature gather      train_lightning.py:138 (blocks[0].srcdata['features'], DGL's lazy slice of g.ndata by ndata[NID]):
 * out[r, :] = feat[ids[r], :] for r < n_rows, bf16 rows of `dim` elements (strides in elements).  norm_out (optional, bf16
 * [n_rows]) receives the row norms of the gathered rows with exactly the bits bliss_embed_norm(out, ...) would produce --
 * the embed_norm model.py:318-320 takes of the same rows right afterwards.  ids must be valid row numbers (padded rows of
 * a static-shape block point at row 0).  The copy runs 8, 4 or 2 bytes at a time, as feat, out and both strides allow; the
 * norm's summation order follows dim, out_stride and the address of `out` alone (bliss_embed_norm's rule).  norm_out NULL: the
 * copy alone.  BLISS_EINVAL before any launch: feat, ids or out NULL; dim <= 0; a stride below dim; dim above what one wave
 * stages in LDS (6144 elements: exactly 48 KiB a workgroup).  n_rows <= 0 returns 0. */
int bliss_gather_rows(const void* feat, int64_t feat_stride, const int32_t* ids, int32_t n_rows, int32_t dim, void* out,
                      int64_t out_stride, void* norm_out, void* stream);

/* th.norm(h, dim=1)   model.py:318-320: embed_norm[j] = ||h_j||_2, fp32 accumulation, bf16 out.  The summation order (and with
 * it the bits) follows how the rows are stored: four columns per lane (4 lane + 256 j) when dim % 4 == 0, row_stride % 4 == 0 and
 * h is 8-byte aligned, else one (lane + 64 j); then the xor butterfly over the 64 lanes.  BLISS_EINVAL:
 * h or out NULL.  n_rows <= 0 returns 0. */
int bliss_embed_norm(const void* h, int32_t n_rows, int32_t dim, int64_t row_stride, void* out, void* stream);

/* SAGEConv 'mean' message passing with edge weights [DGL-recalled: update_all(u_mul_e, mean)],
 * model.py:321-329.  out[i,:] = (1/max(deg_i,1)) * sum_{e in row i} w_e * h[src_e,:]  (mean != 0)
 * or the plain weighted sum (mean == 0).  h bf16 [n_src, dim] (row stride in elements), w bf16
 * [nnz] or NULL (= 1), out bf16 (out_fp32 == 0) or fp32 [n_dst, dim]; src/dst [nnz] = the block's edges
 * (CSR order: dst non-decreasing).  nnz_dev (optional): the true edge count on the device, with nnz an
 * upper bound (capacity-padded arrays; rows past the true n_dst must be empty in indptr). */
int bliss_spmm_chunk_edges(int32_t nnz_bound);
int bliss_spmm_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const void* h,
                   int64_t h_stride, int32_t n_dst, const int32_t* nnz_dev, int32_t nnz, int32_t dim, int mean, void* out,
                   int64_t out_stride, int out_fp32, float* partials, void* stream);

/* Backward of the above w.r.t. h: gh[j,:] = sum_{e: src_e = j} (w_e / max(deg_dst(e),1)) * gout[dst_e,:].
 * t_indptr [n_src+1], t_edge [nnz]: the block's edges grouped by SOURCE in ascending edge order.
 * partials (both calls): fp32 scratch [2 * ceil(nnz / EC) * dim] for rows cut by the EC-edge work chunks,
 * EC = bliss_spmm_chunk_edges(nnz) with the same nnz (bound) as passed to the call. */
int bliss_spmm_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst,
                   const int32_t* indptr, const void* w, const void* gout, int64_t gout_stride, int32_t n_src,
                   const int32_t* nnz_dev, int32_t nnz, int32_t dim, int mean, void* gh, int64_t gh_stride, int out_fp32,
                   float* partials, void* stream);

/* SAGEConv 'pool' message passing [DGL-recalled: update_all(u_mul_e | copy_u, max)], csrc/spmm_max.hip, DESIGN.md section 30:
 *   m_e[c]    = bf16(float(w_e) * float(h[src_e, c]))   (w == NULL: m_e = h[src_e])
 *   arg[i, c] = the lowest edge index e among the in-edges of row i whose m_e[c] is largest (float compare, strict >)
 *   out[i, c] = m_arg[c];   a row without edges (degree 0, capacity padding, edges at or past *nnz_dev): out = 0, arg = -1
 * h, out bf16, arg int32 [n_dst, dim] or NULL (forward only: inference), strides in elements; indptr / src / dst / w / nnz_dev /
 * nnz as for bliss_spmm_fwd.  Inputs are finite (NaN ordering is not defined).
 * bliss_spmm_max_bwd: gh[j, c] = bf16( sum_{e : src_e = j and arg[dst_e, c] == e} float(w_e) * float(gout[dst_e, c]) ), fp32
 * sums in by-source order inside a work chunk, chunk partials added in chunk order; gh bf16 [n_src, dim], sources that receive
 * nothing are zeros; t_indptr / t_edge as for bliss_spmm_bwd.  No float atomics: both calls are bitwise reproducible.
 * partials (both calls): bliss_spmm_max_partial_bytes(nnz, dim) bytes with the same nnz (bound) as passed to the call
 * (per chunk of bliss_spmm_chunk_edges(nnz) edges a head and a tail slot of dim fp32 values + dim int32 args); may be NULL
 * when nnz is at most one chunk.  A negative result of bliss_spmm_max_partial_bytes is BLISS_EINVAL (nnz_bound < 0, dim <= 0).
 * BLISS_EINVAL before any launch: a NULL required pointer (indptr / t_indptr, h / gout, out / gh, the backward's arg; the edge
 * arrays when nnz > 0), a negative count, dim <= 0, a stride below dim, partials NULL with more than one chunk. */
int64_t bliss_spmm_max_partial_bytes(int32_t nnz_bound, int32_t dim);
int bliss_spmm_max_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const void* h,
                       int64_t h_stride, int32_t n_dst, const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* out,
                       int64_t out_stride, int32_t* arg, int64_t arg_stride, void* partials, void* stream);
int bliss_spmm_max_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w,
                       const void* gout, int64_t gout_stride, const int32_t* arg, int64_t arg_stride, int32_t n_src,
                       const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, void* partials, void* stream);

/* bliss_spmm_max_bwd with the ReLU mask of the maximised rows folded in (the pool layer on the tile kernels).
 * act bf16 [n_src, dim], row stride act_stride in elements: the rows the forward maximised over, relu(fc_pool(h)).
 *   gh[j, c] = act[j, c] > 0 ? bf16( sum_{e : src_e = j and arg[dst_e, c] == e} float(w_e) * float(gout[dst_e, c]) ) : +0
 * Where the mask passes: the sums, their order and the single rounding of bliss_spmm_max_bwd; the result is bit-equal to
 * where(act > 0, bliss_spmm_max_bwd's result, +0).  act = +0 and act = -0 both mask.  The mask is applied where a finished row is
 * rounded and stored, never to the fp32 chunk partials; act is read once per source row of a work chunk, where the row begins.  A source with no entry
 * below the live edge count (rows past the live source count of a capacity-padded block included) is cleared WITHOUT reading its
 * act row, which may hold anything.  partials as for bliss_spmm_max_bwd.  BLISS_EINVAL before any launch: every case of
 * bliss_spmm_max_bwd, act == NULL, act_stride < dim. */
int bliss_spmm_max_bwd_relu(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w,
                            const void* gout, int64_t gout_stride, const int32_t* arg, int64_t arg_stride, const void* act,
                            int64_t act_stride, int32_t n_src, const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh,
                            int64_t gh_stride, void* partials, void* stream);

/* SAGEConv 'gcn' message passing [DGL-recalled: update_all(u_mul_e | copy_u, sum), then (neigh + h_dst) / (in_degrees + 1)],
 * csrc/spmm_self.hip, DESIGN.md section 34 -- one rounding where DGL keeps three bf16 intermediates:
 *   out[i, :] = bf16( (sum_{e in row i} float(w_e) * float(h[src_e, :]) + float(h_self[i, :])) * (1.0f / (float)(deg_i + 1)) )
 * deg_i = indptr[i + 1] - indptr[i] (edges with multiplicity, never a sum of weights); w == NULL: w_e = 1.  The messages are
 * summed in fp32 by edge inside a work chunk, chunk partials in chunk order; the self row is added LAST, in fp32; one rounding
 * at the store.  A live row without in-edges: out[i] = h_self[i] bit for bit.  n_dst_dev (optional): the live destination count
 * on the device (bliss_layer_counts_t word 0), n_dst an upper bound -- rows at or past it are stored as +0 WITHOUT reading
 * their self row, which may hold anything; nnz_dev / nnz as for bliss_spmm_fwd (edges at or past *nnz_dev do not exist).
 * h bf16 [n_src, dim], h_self bf16 [n_dst, dim] (may alias h: the destinations of a block are its leading source rows), out
 * bf16 [n_dst, dim] (aliases neither); strides in elements.
 * bliss_spmm_self_bwd, w.r.t. h with the self term folded into the leading rows (h_self aliasing h):
 *   gh[j, :] = bf16( sum_{e : src_e = j} (float(w_e) / (float)(deg_{dst_e} + 1)) * float(gout[dst_e, :])
 *                    + (j < live n_dst ? (1.0f / (float)(deg_j + 1)) * float(gout[j, :]) : 0) )
 * fp32 sums in by-source order inside a work chunk, chunk partials in chunk order, the self term added last where the finished
 * row is rounded and stored (never to the fp32 partials).  gh bf16 [n_src, dim]; sources that receive nothing and rows past the
 * live source count are zeros; t_indptr / t_edge as for bliss_spmm_bwd, indptr = the block's CSR by destination (the degrees).
 * No float atomics: both calls are bitwise reproducible.
 * partials (both calls): as for bliss_spmm_fwd, fp32 [2 * ceil(nnz / EC) * dim]; may be NULL when nnz is at most one chunk.
 * BLISS_EINVAL before any launch: a NULL required pointer (indptr, t_indptr, h / gout, h_self, out / gh; the edge arrays when
 * nnz > 0), a negative count, dim <= 0, a stride below dim, partials NULL with more than one chunk; the backward: n_dst > n_src. */
int bliss_spmm_self_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const void* h, int64_t h_stride,
                        const void* h_self, int64_t h_self_stride, int32_t n_dst, const int32_t* n_dst_dev, const int32_t* nnz_dev,
                        int32_t nnz, int32_t dim, void* out, int64_t out_stride, float* partials, void* stream);
int bliss_spmm_self_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const int32_t* indptr,
                        const void* w, const void* gout, int64_t gout_stride, int32_t n_src, int32_t n_dst, const int32_t* n_dst_dev,
                        const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, float* partials, void* stream);

/* Per-edge dot product of two gathered rows (SDDMM), csrc/sddmm.hip, DESIGN.md section 36: the gradient of the aggregation ops
 * above w.r.t. their per-edge weights (a = d out, b = h) and fn.u_dot_v.  For live edge e with s = src[e], d = dst[e]:
 *   dot_e  = sum_c float(a[d, c]) * float(b[s, c])            (BLISS_SDDMM_MAX: only the columns c with arg[d, c] == e)
 *   out[e] = round(dot_e * coef_e)                             one rounding, to bf16, or none when out_fp32 (out is then float)
 *   coef_e = 1                              BLISS_SDDMM_SUM, BLISS_SDDMM_MAX
 *            1.0f / (float)max(deg_d, 1)    BLISS_SDDMM_MEAN      deg_d = indptr[d + 1] - indptr[d]
 *            1.0f / (float)(deg_d + 1)      BLISS_SDDMM_SELF
 * a bf16 [>= n_dst, dim] by destination, b bf16 [>= n_src, dim] by source, arg int32 [>= n_dst, dim] the winner table of
 * bliss_spmm_max_fwd; strides in elements; any alignment (16-byte, 8-byte and scalar loads give the same bits).
 * Sum order, fp32, never contracted: the columns are cut into groups of 8; group g belongs to lane g % 16 of the edge's 16 lanes;
 * a lane starts from +0 and adds its products one by one in ascending column order (a masked-out column adds +0); the 16 lane
 * sums are added as a balanced tree of neighbours ((p15 + p14) + (p13 + p12)) + ... (four steps: distance 1, 2, 4, 8); then
 * the coefficient, then the rounding.  No float atomics: bitwise reproducible.
 * nnz_dev (optional): the live edge count on the device, nnz an upper bound: live = min(*nnz_dev, nnz).  out[live .. nnz) is
 * written as +0 and nothing -- no endpoint, row, degree or arg entry -- is read for an edge at or past the live count.
 * nnz == 0 returns 0 without a launch.  BLISS_EINVAL before any launch: a NULL required pointer (src, dst, a, b, out when
 * nnz > 0; indptr for MEAN and SELF; arg for MAX), nnz < 0, dim <= 0, a stride below dim, an unknown mode. */
#define BLISS_SDDMM_SUM  0
#define BLISS_SDDMM_MEAN 1
#define BLISS_SDDMM_SELF 2
#define BLISS_SDDMM_MAX  3
int bliss_sddmm_dot(const int32_t* src, const int32_t* dst, const int32_t* indptr, const int32_t* nnz_dev, int32_t nnz, const void* a,
                    int64_t a_stride, const void* b, int64_t b_stride, const int32_t* arg, int64_t arg_stride, int32_t dim, int32_t mode,
                    void* out, int32_t out_fp32, void* stream);

/* Recurrent neighbour aggregation, SAGEConv 'lstm' [DGL-recalled: the mailbox of each destination through nn.LSTM(D, D), the last
 * hidden state kept], csrc/lstm.hip, DESIGN.md section 37.  The input projection is the caller's: p = bf16(h @ W_ih^T), bf16
 * [>= n_src, 4 dim] (gate order i, f, g, o; column k dim + u).  For destination d with live in-edges e_0 .. e_{L-1} in row order:
 *   pre_k = ((float(w_e) * float(p[src_e, k dim + u])) + (float(b_ih) + float(b_hh))) + bf16(h_{t-1}) . w_hh[k dim + u, :]
 *   i, f, o = sigmoid(pre), g = tanh(pre_g); c_t = f c_{t-1} + i g; h_t = o tanh(c_t)      fp32; h_{-1} = c_{-1} = 0
 *   out[d] = bf16(h_{L-1}); +0 for a row without live in-edges and for rows at or past the live destination count
 * The recurrent product runs on MFMA (bf16 operands, fp32 accumulation); the operand h_{t-1} is h rounded to bf16, c and the
 * gates stay fp32.  A workgroup owns bliss_lstm_tile_rows() consecutive destinations and walks to the tile's largest degree; a
 * row whose degree is at or below the step is frozen.  w (bf16 [nnz]) NULL: w_e = 1; b_ih, b_hh (bf16 [4 dim]) NULL: zeros.
 * w_hh bf16 [4 dim, dim]; strides in elements.  1 <= dim <= BLISS_LSTM_MAX_DIM, any dim (padded internally with zero weights).
 * gates (fp32 [nnz, 4 dim]), cell (fp32 [nnz, dim]), hprev (bf16 [nnz, dim]): all three NULL (inference) or all three given
 * (training): per live edge the gate activations, c_t and the operand bf16(h_{t-1}) (+0 at a row's first edge), 22 dim bytes
 * per edge; hprev[live, nnz) is written as +0, gates and cell past the live count are left unwritten and are never read.
 * Live counts: n_dst_dev ? min(*n_dst_dev, n_dst) : n_dst and nnz_dev ? min(*nnz_dev, nnz) : nnz; nothing is read for a row or
 * edge at or past them.  nnz == 0 still writes the +0 rows.
 * bliss_lstm_agg_bwd: the same tiles, t descending; dgate bf16 [nnz, 4 dim] = the gradient at the gate pre-activations per live
 * edge (+0 on [live, nnz)), from gout bf16 [n_dst, dim] = d out and the saved state; d h_{t-1} = dgate_t . w_hh on MFMA, read
 * from w_hh_t = w_hh^T, bf16 [dim, 4 dim].
 * bliss_lstm_edge_reduce: dp[s] = bf16(sum over the out-edges e of s, ascending in the by-source index, float(w_e) *
 * float(dgate[e])), dp bf16 [n_src, 4 dim], fp32 from +0, one wave per source row; sources without a live entry get +0.
 * No float atomics: all three are bitwise reproducible.
 * BLISS_EINVAL before any launch: a NULL required pointer (indptr, w_hh / w_hh_t, out / gout, t_indptr, dp; src and p, the saved
 * state and dgate, t_edge when nnz > 0), a negative count, dim outside 1 .. BLISS_LSTM_MAX_DIM, a stride below the width, one or
 * two of gates / cell / hprev. */
#define BLISS_LSTM_MAX_DIM 256
int bliss_lstm_tile_rows(void);
int bliss_lstm_agg_fwd(const int32_t* indptr, const int32_t* src, const void* w, const void* p, int64_t p_stride, const void* w_hh,
                       int64_t w_hh_stride, const void* b_ih, const void* b_hh, int32_t n_dst, const int32_t* n_dst_dev,
                       const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* out, int64_t out_stride, float* gates, float* cell,
                       void* hprev, void* stream);
int bliss_lstm_agg_bwd(const int32_t* indptr, const void* gout, int64_t gout_stride, const void* w_hh_t, int64_t w_hh_t_stride,
                       const float* gates, const float* cell, int32_t n_dst, const int32_t* n_dst_dev, const int32_t* nnz_dev,
                       int32_t nnz, int32_t dim, void* dgate, void* stream);
int bliss_lstm_edge_reduce(const int32_t* t_indptr, const int32_t* t_edge, const void* w, const void* dgate, int32_t n_src,
                           const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* dp, int64_t dp_stride, void* stream);

/* The element-wise tail of a hidden SAGE layer in one pass (model.py:321-333 and :318-320 of the next layer):
 * out = dropout_p(relu(a + b)) row by row, norm_out[row] = ||out[row,:]||_2 (bf16, may be NULL).  a, b, out: bf16
 * [n_rows, dim].  p_drop = 0 (evaluation) makes it deterministic.  ctr: device uint64[66], zero-initialised once: the
 * dropout stream's launch counter + tickets (bumped by every call with p_drop > 0) -- counter-based bits, not torch's generator.
 * norm_out has the bits of bliss_embed_norm(out, n_rows, dim, out_stride): its summation order follows dim, out_stride and the
 * address of `out` alone, whatever the alignment of a and b lets the loads be.  A sum that is NaN stores +0 (it is not positive).
 * The ReLU is part of the contract: there is no p_drop > 0 without it, because
 * _bwd: din = bf16(dout * (1 / (1 - p))) where out > 0, else +0 (the gradient w.r.t. both a and b) takes BOTH masks from the
 * stored `out`.  That is the gradient only behind a ReLU, where a kept element is positive or has a zero gradient anyway; behind a
 * dropout WITHOUT ReLU it would zero the gradient of every kept negative element (nn.py refuses that combination).
 * BLISS_EINVAL before any launch: a, b, out (dout, out, din) NULL; dim <= 0; n_rows < 0; p_drop outside [0, 1); p_drop > 0 with
 * ctr NULL.  n_rows == 0 returns 0; at p_drop == 0 ctr may be NULL and is not touched. */
int bliss_sage_epilogue_fwd(const void* a, int64_t a_stride, const void* b, int64_t b_stride, int32_t n_rows, int32_t dim,
                            float p_drop, uint32_t seed, uint64_t* ctr, void* out, int64_t out_stride, void* norm_out, void* stream);
/* (the mask is `out > 0`: right only where `out` went through the ReLU, see above) */
int bliss_sage_epilogue_bwd(const void* dout, int64_t dout_stride, const void* out, int64_t out_stride, int32_t n_rows, int32_t dim,
                            float p_drop, void* din, int64_t din_stride, void* stream);

/* The by-source index the backward needs: t_edge [cap_b] = edge indices grouped by source, ascending
 * inside a source; t_indptr [n_src_cap + 1].  The edge count is *nnz_dev if given (arrays padded to
 * cap_b; how static-shape / HIP-graph callers work), else nnz.  temp: bliss_block_transpose_temp_bytes. */
int64_t bliss_block_transpose_temp_bytes(int32_t cap_b, int32_t n_src_cap);
int bliss_block_transpose(const int32_t* src, const int32_t* nnz_dev, int32_t nnz, int32_t cap_b, int32_t n_src_cap,
                          int32_t* t_indptr, int32_t* t_edge, void* temp, int64_t temp_bytes, void* stream);

/* Graph preparation: edge list -> the int32 CSC graph the samplers read.  Replaces
 * dgl.remove_self_loop + dgl.add_self_loop (+ g.add_edges(dst, src) when undirected) + g.int() + g.formats(['csc'])
 * of train_lightning.py:334-341, 373.  Edge ids follow DGL: surviving edges renumbered in order, then the V self loops,
 * then (undirected) the reverse of every edge; columns hold their edges in ascending edge id (self loop last).
 * Outputs are sized bliss_graph_prepare_capacity() = (n_edges + V) * (undirected ? 2 : 1) (must stay < 2^31); the true
 * edge count is written to the device word n_out; err (device int32, caller-zeroed) gets bit 1 if an endpoint is outside
 * [0, V).  No host synchronisation. */
int64_t bliss_graph_prepare_capacity(int64_t n_edges, int32_t num_nodes, int undirected);
int64_t bliss_graph_prepare_temp_bytes(int64_t n_edges, int32_t num_nodes, int undirected);
int bliss_graph_prepare(const int32_t* coo_src, const int32_t* coo_dst, int64_t n_edges, int32_t num_nodes, int undirected,
                        int64_t* indptr, int32_t* indices, int32_t* eid, int64_t* n_out, int32_t* err, void* temp,
                        int64_t temp_bytes, void* stream);

/* calculate_alpha (SAGE/GCN) + calculate_rewards + update_exp3_weights up to the scatter,
 * bandit_sampler.py:157, :180-193, :221-248.  One launch per block.
 * edge_w_pos: g.edata['w'] by CSC position.  w_pos: the layer's exp3 row (updated in place).
 * row_sum: int64[3 * BLISS_ROWSUM_SLOTS] exact running sum of the row (32-bit limbs, value * 2^64; the sum is the total
 * over BLISS_ROWSUM_SLOTS replicas of three limbs, which keeps concurrent waves off a single address), updated.
 * rewards_out: bf16 [n_edges] edata['rewards'] or NULL.  factor_out: bf16 [n_edges] exp(min(1, delta r/(P n)))
 * or NULL.  apply == 0 computes rewards/factors only and leaves w_pos and row_sum untouched. */
int bliss_exp3_update(const bliss_graph_t* g, const void* edge_w_pos, void* w_pos, int64_t* row_sum,
                      const int32_t* blk_indptr, const int32_t* blk_src, const int32_t* blk_dst,
                      const int32_t* blk_pos, const void* q_ij, const void* node_prob, const void* embed_norm,
                      const void* alpha_or_null, const int32_t* dst_nid, int32_t n_dst, const int32_t* n_edges_dev,
                      int32_t edges_bound, float delta_f, void* rewards_out, void* factor_out, int apply,
                      int32_t* err, void* stream);

/* sampler.exp3(mfgs, g) (bandit_sampler.py:251-267) for ALL blocks of a step in two launches: one bliss_exp3_update
 * (apply = 1) over every block and one bliss_exp3_normalize over every layer's row.  Fields as the arguments of those
 * two calls; every block has its own w_pos row, row_sum and scratch. */
#define BLISS_EXP3_MAX_BLOCKS 8
typedef struct {
  void* w_pos; int64_t* row_sum; int64_t* scratch; void* norm_out;
  const int32_t *blk_indptr, *blk_src, *blk_dst, *blk_pos;
  const void *q_ij, *node_prob, *embed_norm, *alpha_or_null;
  const int32_t* dst_nid; const int32_t* n_edges_dev;
  void* rewards_out;
  int32_t edges_bound;
} bliss_exp3_block_t;
int bliss_exp3_step(const bliss_graph_t* g, const void* edge_w_pos, const bliss_exp3_block_t* blocks, int32_t n_blocks,
                    float delta_f, int32_t* err, void* stream);
/* Only the first of the two launches: the updates of all blocks, rows and row sums left un-normalised -- for rows that are
 * spread over several shards, whose norm is the all-reduced sum (bliss_exp3_normalize_global). */
int bliss_exp3_update_blocks(const bliss_graph_t* g, const void* edge_w_pos, const bliss_exp3_block_t* blocks, int32_t n_blocks,
                             float delta_f, int32_t* err, void* stream);
/* bliss_exp3_normalize_global for several rows in ONE launch (fields used: w_pos, row_sum, scratch, norm_out); row r's all-reduced
 * limbs at norm_limbs + r * limb_stride. */
int bliss_exp3_normalize_global_rows(const bliss_exp3_block_t* rows, int32_t n_rows, int64_t num_edges, const int64_t* norm_limbs,
                                     int64_t limb_stride, void* stream);

/* The scatter half of update_exp3_weights (bandit_sampler.py:248) for factors computed elsewhere -- used
 * when several ranks keep replicas of the bandit state: w_pos[pos[e]] *= factor[e] for e < *n_dev, and
 * row_sum follows.  pos must be unique within one call; calls apply in stream order. */
int bliss_exp3_apply(void* w_pos, int64_t* row_sum, const int32_t* pos, const void* factor, const int32_t* n_dev,
                     int32_t n_bound, int32_t* err, void* stream);

/* The same for the lists of ALL ranks and ALL blocks of a step in ONE launch (replicas).  `gathered`
 * holds n_ranks packed buffers of rank_stride_words int32 words each (what an all-gather of every rank's buffer leaves);
 * inside a rank's buffer block b has its positions at pos_off_words[b] (int32 [bound[b]]), its bf16 factors at element
 * factor_off_bf16[b] of the buffer viewed as bf16, and its true list length at count_off_words[b].  Ranks are applied in
 * rank order (grid barrier between them: the bf16 products do not commute), blocks of one rank side by side; a position may
 * occur in several ranks' lists.  barrier: int32[2], zero on first use, left zero.  Bits identical to n_ranks x n_blocks
 * bliss_exp3_apply calls in rank order. */
typedef struct {
  void* w_pos[BLISS_EXP3_MAX_BLOCKS];
  int64_t* row_sum[BLISS_EXP3_MAX_BLOCKS];
  int32_t pos_off_words[BLISS_EXP3_MAX_BLOCKS], factor_off_bf16[BLISS_EXP3_MAX_BLOCKS], count_off_words[BLISS_EXP3_MAX_BLOCKS],
      bound[BLISS_EXP3_MAX_BLOCKS];
  int32_t n_blocks, n_ranks;
  int64_t rank_stride_words;
} bliss_exp3_rank_lists_t;
int bliss_exp3_apply_ranks(const bliss_exp3_rank_lists_t* lists, const int32_t* gathered, int32_t* barrier, int32_t* err, void* stream);

/* Fill one rank's packed buffer for that exchange in ONE launch: for every block the first min(*n_dev[b], bound[b])
 * positions (blk_pos) go to buf + pos_off_words[b], the true count *n_dev[b] to buf[count_off_words[b]] (the factors are
 * written in place by bliss_exp3_update's factor_out). */
typedef struct {
  const int32_t* pos[BLISS_EXP3_MAX_BLOCKS];
  const int32_t* n_dev[BLISS_EXP3_MAX_BLOCKS];
  int32_t pos_off_words[BLISS_EXP3_MAX_BLOCKS], count_off_words[BLISS_EXP3_MAX_BLOCKS], bound[BLISS_EXP3_MAX_BLOCKS];
  int32_t n_blocks;
} bliss_pack_lists_t;
int bliss_pack_lists(const bliss_pack_lists_t* lists, int32_t* buf, void* stream);

/* F.normalize(row, p=1, dim=0), bandit_sampler.py:249, bit-exact: norm = bf16(exact sum).  The pass
 * over the row is skipped on the device when norm == 1.0 (x / 1.0 == x).  scratch: int64[BLISS_NORM_SCRATCH], zero-initialised
 * once by the caller and left zero ([0] afterwards holds norm bits | skip << 16 | err << 20). */
int bliss_exp3_normalize(void* w_pos, int64_t num_edges, int64_t* row_sum, int64_t* scratch, void* norm_out_bf16,
                         void* stream);

/* Exact row sum from scratch (initialisation / verification): row_sum int64[3 * BLISS_ROWSUM_SLOTS]. */
int bliss_row_sum(const void* w_pos, int64_t num_edges, int64_t* row_sum, void* stream);

/* ---- GATv2 attention path (custom_GATv2Conv.forward, model.py:48-112) ------------------------------------------
 * feat: bf16 [n_src, heads*head_dim] = fc_src(h) (shared weights: the destinations are its first n_dst rows);
 * edge arrays src/dst [nnz] of the block (CSR order); nnz_dev optional as for bliss_spmm_fwd.
 *   bliss_gat_logits        e[e,h] = attn[h,:] . leaky_relu(feat[src_e,h,:] + feat[dst_e,h,:])   -> bf16 [nnz, heads]  (:82-86)
 *   bliss_gat_edge_softmax  a = softmax of x over the in-edges of every destination (:88-90), or with backward != 0
 *                           de = a * (x - sum_{e'} a x) where x = d_a
 *   bliss_gat_rows          row sums of per-edge vectors, never materialised.  which bit 0: rows are sources (through
 *                           t_edge, the by-source index) instead of destinations; bit 1: the vector is the logits
 *                           backward  coef[e,h]*attn[col]*lrelu'(feat[src]+feat[dst])  instead of  coef[e,h]*feat[nbr,col]
 *                           (which = 0 is the forward aggregation of :98, 1 its backward w.r.t. feat, 2 / 3 the two halves of
 *                           the logits backward; with which = 2 and d_attn != NULL also d_attn[col] += sum_e coef*lrelu(x)).
 *                           partials: fp32 [2 * ceil(nnz / bliss_gat_chunk_edges()) * heads*head_dim].
 *   bliss_gat_edge_dot      out[e,h] = g[dst_e,h,:] . feat[src_e,h,:]   (d_a of the aggregation)
 *   bliss_gat_alpha         calculate_alpha, model == 'gat' (bandit_sampler.py:146-154), exact sums, bf16 [nnz]. */
/* edges per work chunk of bliss_gat_rows: its partials buffer holds 2 * ceil(nnz / chunk) * heads * head_dim floats */
int bliss_gat_chunk_edges(void);
int bliss_gat_logits(const int32_t* src, const int32_t* dst, const int32_t* nnz_dev, int32_t nnz, const void* feat,
                     int64_t feat_stride, const void* attn, int32_t heads, int32_t head_dim, float negative_slope, void* e_out,
                     void* stream);
/* The same message passing with ONE workgroup per destination row (csrc/gat_fused.hip): bliss_gat_fused_fwd = logits + edge
 * softmax (+ attention dropout, model.py:88) + aggregation in one launch -- e, a, a_drop [nnz, heads] bf16 and rst [n_dst,
 * heads*head_dim] bf16 come out with the bits of the three separate kernels above; bliss_gat_fused_bwd_dst = d a, the softmax
 * backward (de [nnz, heads]), d er [n_dst, heads*head_dim] and d attn (float [heads*head_dim], summed over the rows in row order:
 * dattn_part float [n_dst, heads*head_dim], block_sums float [ceil(n_dst / 32), heads*head_dim], ticket unused) in
 * three launches.  The by-source half of the backward is bliss_gat_rows(which = 3) with g / a_drop given (see below).
 * n_dst_dev (optional) = the true row count of a capacity-padded block; drop_p > 0: drop_ctr = device uint64[2] (launch
 * counter + ticket, zero-initialised), drop_ctr_used (optional uint32) receives the counter value this launch used.
 * Supported when heads <= 8 and heads*head_dim <= 1024 (head_dim % 4 == 0) or <= 256: bliss_gat_fused_supported. */
typedef struct {
  const int32_t* indptr; const int32_t* src; int32_t n_dst; const int32_t* n_dst_dev;
  const void* feat; int64_t feat_stride; const void* attn; int32_t heads; int32_t head_dim; float negative_slope;
  void* e; void* a; void* a_drop;
  void* rst; int64_t rst_stride;
  float drop_p; uint32_t drop_seed; void* drop_ctr; void* drop_ctr_used;
  const void* g; int64_t g_stride; void* de; void* d_er; int64_t d_er_stride; float* dattn_part;
  /* virtual workgroups (required): a destination with more than bliss_gat_segment_edges() in-edges is shared by several
   * workgroups.  wg_row int32 [cap_wg, 4], 16-byte aligned (row, first edge, end, G << 16 | segment per virtual workgroup; the
   * shared rows first) + n_wg_dev from bliss_gat_segments; row_ws uint32 [n_dst * 32],
   * zero-initialised once (the kernels return it to zero); seg_part float [cap_wg * (heads*head_dim + 8)] scratch; dattn_part
   * then holds cap_wg rows and block_sums ceil(cap_wg / 32) rows; err receives BLISS_ERR_FLAG_TIMEOUT if a row's workgroups
   * fail to meet. */
  const int32_t* wg_row; const int32_t* n_wg_dev; int32_t cap_wg; void* row_ws; float* seg_part; int32_t* err;
} bliss_gat_fused_t;
int bliss_gat_segment_edges(void);
/* measurement hook (scratch/gatbench.py): while `stamps` / `stamps_bwd` is not NULL every virtual workgroup of bliss_gat_fused_fwd /
 * bliss_gat_fused_bwd_dst writes eight 100 MHz device timestamps (start, row resolved, pass 1 done, after its barrier, after the
 * exchange, pass 2 done, pass 3 done, end) to stamps[8 * workgroup ..]; NULL switches it off again.  Not part of the data path. */
int bliss_gat_fused_stamps(long long* stamps, long long* stamps_bwd);
/* the virtual workgroups' descriptors for the two kernels below: row r gets max(1, ceil(deg_r / bliss_gat_segment_edges()))
 * consecutive ids; cap_wg >= n_dst + nnz_bound / bliss_gat_segment_edges() suffices; wg_row holds 4 * cap_wg int32. */
int bliss_gat_segments(const int32_t* indptr, int32_t n_dst, int32_t cap_wg, int32_t* wg_row, int32_t* n_wg_dev, int32_t* err, void* stream);
int bliss_gat_fused_supported(int32_t heads, int32_t head_dim);
/* d el[j, :] = sum over the out-edges e = (j -> i) of  de[e, h] attn lrelu'(feat[j] + feat[i])  +  a_drop[e, h] g[i, :]  -- the
 * by-source half of the GATv2 backward (logits + aggregation) in one merge-style pass; partials as for bliss_gat_rows. */
int bliss_gat_rows_src_fused(const int32_t* t_indptr, int32_t n_src, const int32_t* t_edge, const int32_t* src, const int32_t* dst,
                             const int32_t* nnz_dev, int32_t nnz, const void* de, const void* a_drop, const void* feat, int64_t feat_stride,
                             const void* g, int64_t g_stride, const void* attn, int32_t heads, int32_t head_dim, float negative_slope,
                             void* out, int64_t out_stride, float* partials, void* stream);
int bliss_gat_fused_fwd(const bliss_gat_fused_t* args, void* stream);
int bliss_gat_fused_bwd_dst(const bliss_gat_fused_t* args, float* block_sums, float* d_attn, uint32_t* ticket, void* stream);
/* Full-neighbour inference of one GATv2 layer straight off the graph's CSC (custom_GATv2Conv under model.py:236-289; DESIGN.md
 * section 23): finished layer rows for the destinations row0 .. row0 + n_rows - 1, two launches (the range's workgroup
 * descriptors, then the forward), no block, no id remapping, nothing of edge size written.
 *   indptr  int64 [V + 1], 8-byte aligned; indices int32 [E], 4-byte aligned: the source of CSC position pos is feat[indices[pos]],
 *           row r of the range owns the positions indptr[row0 + r] .. indptr[row0 + r + 1] - 1 and its own feature row is
 *           feat[row0 + r] (shared weights).  row0 >= 0, n_rows >= 0, row0 + n_rows <= V and indices[] < V are the caller's.
 *   n_edges indptr[row0 + n_rows] - indptr[row0] as the host knows it: it sizes the scratch (below) and must be < 2^31 (offsets
 *           inside a range are 32-bit; everything added to a pointer is 64-bit).  The kernels read the offsets from indptr itself;
 *           a range that holds more edges than stated is cut off with BLISS_ERR_CAP_EDGES in *err, never run past the scratch.
 *   feat    bf16 [V, heads*head_dim] = fc_src(h) of ALL nodes, row stride feat_stride >= heads*head_dim elements; attn bf16
 *           [heads, head_dim].  Limits: bliss_gat_fused_supported(heads, head_dim).  feat, attn, res, out 2-byte aligned; a width
 *           above 256 runs on 8-byte loads and needs head_dim % 4 == 0, feat and attn 8-byte aligned, feat_stride % 4 == 0.
 *   res     bf16 [n_rows, heads*head_dim] (row r of the RANGE, stride res_stride) or NULL; act 0 = none, 1 = ELU (alpha 1).
 *   out     bf16 [n_rows, heads*head_dim], stride out_stride >= heads*head_dim:
 *           out[r] = act(bf16(rst[r] + res[r])) rounded to bf16, with rst the bits bliss_gat_fused_fwd(drop_p = 0) gives on the
 *           full-neighbour block of the range and the add / ELU rounded where bliss_gat_glue_fwd rounds them.  A row without
 *           in-edges has rst = 0.  Rows outside the range are not touched.
 *   scratch wg_row int32 [4 * cap_wg], 16-byte aligned, and n_wg_dev int32 [1]: written by the call; cap_wg >= n_rows + n_edges /
 *           bliss_gat_segment_edges(); seg_part float [cap_wg * heads*head_dim]; row_ws uint32 [32 * n_rows], zero-initialised
 *           once (the kernel returns it to zero: launches follow each other without a memset); err (optional) int32, receives
 *           BLISS_ERR_FLAG_TIMEOUT if the workgroups of a shared row fail to meet within the spin bound, as for the fused kernels.
 * n_rows == 0 launches nothing and returns 0 (the scratch may then be NULL).  BLISS_EINVAL, before any launch: args, indptr,
 * indices, feat, attn or out NULL; heads outside 1 .. 8, head_dim <= 0 or a pair bliss_gat_fused_supported refuses; n_rows, row0
 * or n_edges negative; n_edges >= 2^31; act not 0 or 1; a pointer or stride that breaks the alignment above (a width above 256
 * without the 8-byte alignment included); a stride below heads*head_dim; with n_rows > 0 missing or misaligned scratch or a
 * cap_wg below the bound. */
typedef struct {
  const int64_t* indptr; const int32_t* indices; int32_t row0; int32_t n_rows; int64_t n_edges;
  const void* feat; int64_t feat_stride; const void* attn; int32_t heads; int32_t head_dim; float negative_slope;
  const void* res; int64_t res_stride; int32_t act;
  void* out; int64_t out_stride;
  int32_t* wg_row; int32_t* n_wg_dev; int32_t cap_wg; void* row_ws; float* seg_part; int32_t* err;
} bliss_gat_infer_t;
int bliss_gat_infer_fwd(const bliss_gat_infer_t* args, void* stream);
/* bliss_gat_logits without the intermediate bf16 roundings, float result (the north star's 1e-4 check against fp32 math);
 * likewise bliss_gat_edge_softmax with backward == 2 (float logits in, float out) and bliss_gat_rows with which == 4 (the
 * forward aggregation with float coefficients and float output rows, out_stride in floats). */
int bliss_gat_logits_f32(const int32_t* src, const int32_t* dst, const int32_t* nnz_dev, int32_t nnz, const void* feat,
                         int64_t feat_stride, const void* attn, int32_t heads, int32_t head_dim, float negative_slope, float* e_out,
                         void* stream);
int bliss_gat_edge_dot(const int32_t* src, const int32_t* dst, const int32_t* nnz_dev, int32_t nnz, const void* feat,
                       int64_t feat_stride, const void* g, int64_t g_stride, int32_t heads, int32_t head_dim, void* out, void* stream);
int bliss_gat_edge_softmax(const int32_t* indptr, int32_t n_dst, const void* x, const void* a_or_null, int32_t heads, int backward,
                           void* out, void* stream);
int bliss_gat_rows(int which, const int32_t* row_ptr, int32_t n_rows, const int32_t* t_edge, const int32_t* src, const int32_t* dst,
                   const int32_t* nnz_dev, int32_t nnz, const void* coef, const void* feat, int64_t feat_stride, const void* attn,
                   int32_t heads, int32_t head_dim, float negative_slope, void* out, int64_t out_stride, float* partials,
                   float* d_attn, void* stream);
int bliss_gat_alpha(const int32_t* indptr, int32_t n_dst, const void* q_ij, const void* a_ij, void* alpha_out, int32_t* err, void* stream);

/* The element-wise glue around a GATv2 layer's message passing in ONE launch per direction, bounded by a device-side row count
 * (csrc/gat_glue.hip).  For rows r < min(n_rows, *n_rows_dev)  (n_rows_dev NULL: n_rows):
 *   x = rst[r, h, d] (+ res[r, h, d], rounded to bf16);  y = ELU(x) rounded to bf16 (act = 1) or x (act = 0);
 *   z = y as [heads * head_dim] (head_mean = 0) or bf16((sum_h y[h, d]) * (1 / heads)) as [head_dim] (head_mean = 1: fp32 sum,
 *   one rounding);  pre = z (optional);  out = z, or with drop_p > 0:  keep ? bf16(z / (1 - p)) : 0  where keep comes from the
 *   keyed hash of (drop_seed, launch counter, r * width + column) -- the stream of bliss_sage_epilogue_fwd.  drop_ctr: device
 *   uint64[2], zero-initialised once (bumped behind every launch with drop_p > 0); drop_ctr_used: device uint32, receives the
 *   counter the launch used (the backward reads it there).
 * Rows at or past the live count are written as zeros and nothing of their inputs is read.  heads = 1, act = 0, res = NULL is a
 * dropout-only pass over [n_rows, head_dim].
 * _bwd: din [n_rows, heads * head_dim] = the gradient w.r.t. rst (and, unchanged, w.r.t. res) from dout [n_rows, width]: mask and
 * scale, the transpose of the flatten / head mean, the ELU derivative taken from x (g * exp(x) for x <= 0, as torch's elu does),
 * each rounded to bf16 where the tensor ops round; zero rows at or past the count.  rst / res are read only when act = 1.
 * bliss_gat_head_mean: out[e] = bf16((sum_h x[e, h]) * (1 / heads)) for e < min(n_edges, *n_edges_dev); the tail is left alone. */
typedef struct {
  const void* rst; int64_t rst_stride;
  const void* res; int64_t res_stride;
  int32_t n_rows; const int32_t* n_rows_dev;
  int32_t heads; int32_t head_dim; int32_t act; int32_t head_mean;
  float drop_p; uint32_t drop_seed; uint64_t* drop_ctr; uint32_t* drop_ctr_used;
  void* out; int64_t out_stride;
  void* pre; int64_t pre_stride;
  const void* dout; int64_t dout_stride;
  void* din; int64_t din_stride;
} bliss_gat_glue_t;
int bliss_gat_glue_fwd(const bliss_gat_glue_t* args, void* stream);
int bliss_gat_glue_bwd(const bliss_gat_glue_t* args, void* stream);
int bliss_gat_head_mean(const void* x, int32_t heads, int32_t n_edges, const int32_t* n_edges_dev, void* out, void* stream);

/* dglnn.GraphConv(norm='both') message passing with sampler edge weights on bounded kernels (csrc/gcn.hip, DESIGN.md section 26;
 * model.py:386-439):
 *   ns[j] = 1 / sqrt(max(outdeg_j, 1)),  outdeg_j = t_indptr[j+1] - t_indptr[j]  (the block's by-source index)
 *   nd[i] = 1 / sqrt(max(indeg_i, 1)),   indeg_i  = indptr[i+1] - indptr[i]
 *   fwd:  out[i, :] = bf16( nd[i] * sum_{e in row i}    (float(w_e) * ns[src_e]) * h[src_e, :] )
 *   bwd:  gh[j, :]  = bf16( ns[j] * sum_{e : src_e = j} (float(w_e) * nd[dst_e]) * gout[dst_e, :] )
 * ns, nd fp32 (IEEE sqrt, one division); the coefficient is one fp32 product; fp32 accumulation in edge order inside a work
 * chunk, chunk partials added in chunk order; one rounding to bf16 at the store.  w bf16 [nnz] or NULL (= 1).
 * bliss_gcn_norms: one launch, ns[n_src] and nd[n_dst]; rows past the live counts are empty in both index arrays (norm 1).
 * bliss_gcn_spmm_fwd / _bwd: arguments as bliss_spmm_fwd / bliss_spmm_bwd plus the two norm vectors; nnz_dev (optional): the
 * live edge count, nothing at or past it is read; partials: fp32 scratch [2 * ceil(nnz / EC) * dim], EC =
 * bliss_spmm_chunk_edges(nnz).  Rows without edges (capacity padding included) are written as zeros. */
int bliss_gcn_norms(const int32_t* indptr, int32_t n_dst, const int32_t* t_indptr, int32_t n_src, float* nd, float* ns, void* stream);
int bliss_gcn_spmm_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const float* ns, const float* nd,
                       const void* h, int64_t h_stride, int32_t n_dst, const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* out,
                       int64_t out_stride, float* partials, void* stream);
int bliss_gcn_spmm_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w,
                       const float* ns, const float* nd, const void* gout, int64_t gout_stride, int32_t n_src, const int32_t* nnz_dev,
                       int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, float* partials, void* stream);

/* The row-wise tail of a GraphConv layer, bounded by a device-side row count.  For r < min(n_rows, *rows_dev) (rows_dev NULL:
 * n_rows):  x = bf16(a[r, c] + bias[c]) (bias NULL: a[r, c]);  relu != 0: max(x, 0);  drop_p > 0:  keep ? bf16(x / (1 - p)) : 0
 * with keep from the keyed hash of (drop_seed, launch counter, r * width + c) -- the stream of bliss_gat_glue_fwd: drop_ctr is a
 * device uint64[2], zero-initialised once and bumped behind every launch with drop_p > 0; drop_ctr_used (device uint32) receives
 * the counter the launch used.  norm_out (optional, bf16 [n_rows]): the row norms of the stored rows in bliss_embed_norm's
 * summation order.  Rows at or past the count are written as zeros (norm 0) and nothing of their inputs is read.
 * _bwd: din[r, c] = dout[r, c] masked and scaled as the forward did, then zero where the stored out[r, c] <= 0 (relu != 0);
 * zero rows at or past the count;  db (optional, bf16 [width]) = sum_{r < live} din[r, c]: fp32 sums over chunks of
 * bliss_gcn_db_chunk_rows() rows (a size that does not depend on n_rows) in db_partials (fp32 [ceil(n_rows / chunk) * width]),
 * added in chunk order and rounded once. */
typedef struct {
  const void* a; int64_t a_stride;
  const void* bias;
  int32_t n_rows; const int32_t* rows_dev; int32_t width; int32_t relu;
  float drop_p; uint32_t drop_seed; uint64_t* drop_ctr; uint32_t* drop_ctr_used;
  void* out; int64_t out_stride;
  void* norm_out;
  const void* dout; int64_t dout_stride;
  void* din; int64_t din_stride;
  void* db; float* db_partials;
} bliss_gcn_epilogue_t;
int bliss_gcn_db_chunk_rows(void);
int bliss_gcn_epilogue_fwd(const bliss_gcn_epilogue_t* args, void* stream);
int bliss_gcn_epilogue_bwd(const bliss_gcn_epilogue_t* args, void* stream);

/* GraphConv(norm='both') full-neighbour inference straight off the graph's CSC (csrc/gcn_infer.hip, DESIGN.md section 27;
 * model.py:441-488): the message passing of GCN.inference's batch-by-batch walk without a block.  Batch b is the rows
 * [b * batch_size, min(n_nodes, (b + 1) * batch_size)), its first edge E0_b = indptr[b * batch_size], its n_b edges the CSC
 * positions up to the next batch's first.  For the CSC position e of batch b with source j = indices[e]:
 *   cnt   = positions of batch b whose source is j (parallel edges count once each: the block's out-degree of j)
 *   ns[e] = 1 / sqrt(max(cnt, 1)),   nd[i] = 1 / sqrt(max(indeg_i, 1))          (bliss_gcn_norms' expressions, fp32)
 *   out[i, :] = bf16( nd[i] * sum_{e in row i} ns[e] * h[indices[e], :] )
 * and the fp32 sum is the one bliss_gcn_spmm_fwd produces on the batch's full-neighbour block: the batch's positions are cut
 * into chunks of EC_b = bliss_spmm_chunk_edges(n_b) counted from E0_b, a row's terms inside a chunk are added in edge order
 * starting from zero, a row's chunk partials are added in chunk order starting from the first; one product with nd[i], one
 * rounding.  Rows without edges are zeros.  Bitwise reproducible: no float atomics, no tickets, no spin waits.
 * Both calls work on a destination range of whole batches: row0 % batch_size == 0 and row0 + n_rows a multiple of batch_size
 * or n_nodes.  edge0 = indptr[row0] and n_edges = indptr[row0 + n_rows] - edge0 as the HOST knows them; n_edges < 2^31
 * (offsets inside a range are 32-bit, everything added to a pointer is 64-bit).  indices[] < n_nodes is the caller's.
 *   indptr int64 [n_nodes + 1], 8-byte aligned; indices int32, 4-byte aligned; ns fp32 [n_edges]: ns[e - edge0].
 * bliss_gcn_infer_src_norms writes ns for the range: bliss_block_transpose on indices[edge0 .. edge0 + n_edges) with n_nodes
 *   source slots, then one launch with a thread per edge (its row by bisection of indptr, cnt as two lower bounds in its
 *   source's ascending position list).  Scratch: t_indptr int32 [n_nodes + 1], t_edge int32 [n_edges], temp of temp_bytes >=
 *   bliss_block_transpose_temp_bytes(n_edges, n_nodes).  h / dim / out are not looked at.  Nothing to do (returns 0, scratch may be
 *   NULL) when n_rows or n_edges is 0.
 * bliss_gcn_infer_spmm reads ns and gathers rows of h (bf16 [n_nodes, dim], row stride h_stride >= dim) into out (bf16
 *   [n_rows, dim]: row r of the RANGE, stride out_stride >= dim); one launch, a wave per row.  8-byte accesses when dim % 4 == 0,
 *   both strides % 4 == 0 and h, out 8-byte aligned; one feature per lane otherwise (same bits).  A row whose batch does not lie
 *   inside [edge0, edge0 + n_edges) is left untouched.  The scratch fields are not looked at.  n_rows == 0 returns 0.
 * bliss_gcn_infer_chunk_edges(n_b): the EC_b the kernel uses (= bliss_spmm_chunk_edges).
 * BLISS_EINVAL before any launch: args, indptr or indices NULL; n_nodes <= 0; batch_size < 1; row0 or n_rows negative or past
 * n_nodes; a range that cuts a batch; edge0 or n_edges negative, n_edges >= 2^31; ns NULL with n_edges > 0; a misaligned
 * pointer; src_norms: missing or misaligned scratch, temp_bytes too small; spmm: h or out NULL, dim <= 0, a stride below dim. */
typedef struct {
  const int64_t* indptr; const int32_t* indices; int32_t n_nodes; int32_t batch_size;
  int32_t row0; int32_t n_rows; int64_t edge0; int64_t n_edges;
  float* ns;
  int32_t* t_indptr; int32_t* t_edge; void* temp; int64_t temp_bytes;
  const void* h; int64_t h_stride; int32_t dim;
  void* out; int64_t out_stride;
} bliss_gcn_infer_t;
int bliss_gcn_infer_chunk_edges(int32_t n_batch_edges);
int bliss_gcn_infer_src_norms(const bliss_gcn_infer_t* args, void* stream);
int bliss_gcn_infer_spmm(const bliss_gcn_infer_t* args, void* stream);

/* SAGEConv full-neighbour inference straight off the graph's CSC (csrc/sage_infer.hip; model.py:335-383):
 * the message passing of SAGE.inference's batch-by-batch walk without a block, forward only.  The batch structure is that of
 * bliss_gcn_infer_t: batch b is the rows [b * batch_size, min(n_nodes, (b + 1) * batch_size)), its first edge E0_b =
 * indptr[b * batch_size], it has n_b edges, EC_b = bliss_spmm_chunk_edges(n_b).
 *   BLISS_SAGE_INFER_MEAN: out[i, :] = bf16( (1.0f / (float)max(deg_i, 1)) * S_i ), S_i the fp32 sum bliss_spmm_fwd(mean = 1,
 *     w = NULL) produces for row i on the full-neighbour block of i's batch: the batch's CSC positions are cut into chunks of EC_b
 *     counted from E0_b, a row's terms inside a chunk are added in edge order starting from +0, a row's chunk partials are added
 *     in chunk order starting from the first; one product with the scale, one rounding.
 *   BLISS_SAGE_INFER_MAX: out[i, c] = max over the in-edges of h[indices[e], c] by the rule of bliss_spmm_max_fwd(w = NULL,
 *     arg = NULL): the running best starts at the first edge's value and moves on strict > (float compare) in edge order; the
 *     batch structure does not enter the value.  Inputs are finite.  No arg is written.
 *   A row without edges is +0 under both.  Bitwise reproducible: no float atomics, no partial buffer, no fix-up launch.
 * The range rules are bliss_gcn_infer_spmm's: row0 % batch_size == 0 and row0 + n_rows a multiple of batch_size or n_nodes;
 * edge0 = indptr[row0] and n_edges = indptr[row0 + n_rows] - edge0 as the HOST knows them; n_edges < 2^31 (offsets inside a range
 * are 32-bit, everything added to a pointer is 64-bit).  indices[] < n_nodes is the caller's.
 *   indptr int64 [n_nodes + 1], 8-byte aligned; indices int32, 4-byte aligned; h bf16 [n_nodes, dim], row stride h_stride >= dim;
 *   out bf16 [n_rows, dim]: row r of the RANGE, stride out_stride >= dim.
 * One call is one launch, a wave per row.  8-byte accesses when dim % 4 == 0, both strides % 4 == 0 and h, out 8-byte aligned;
 * one feature per lane otherwise (same bits).  A row whose batch does not lie inside [edge0, edge0 + n_edges) is left untouched.
 * n_rows == 0 returns 0.
 * BLISS_EINVAL before any launch: args, indptr, indices, h or out NULL; n_nodes <= 0; batch_size < 1; row0 or n_rows negative or
 * past n_nodes; a range that cuts a batch; edge0 or n_edges negative, n_edges >= 2^31; reduce not 0 or 1; dim <= 0; a stride
 * below dim; a misaligned indptr or indices (h or out at an odd address). */
#define BLISS_SAGE_INFER_MEAN 0
#define BLISS_SAGE_INFER_MAX  1
typedef struct {
  const int64_t* indptr; const int32_t* indices; int32_t n_nodes; int32_t batch_size;
  int32_t row0; int32_t n_rows; int64_t edge0; int64_t n_edges;   /* a range of whole batches, as bliss_gcn_infer_t */
  int32_t reduce;
  const void* h; int64_t h_stride; int32_t dim;                   /* bf16 [n_nodes, dim] */
  void* out; int64_t out_stride;                                  /* bf16 [n_rows, dim]: row r of the RANGE */
} bliss_sage_infer_t;
int bliss_sage_infer_spmm(const bliss_sage_infer_t* args, void* stream);

/* Per-kernel timing with HIP events recorded on the launching stream (bench.py's roofline object).
 * bliss_prof_enable(id): -2 off (default), -1 every kernel, >= 0 one kernel id; names via
 * bliss_prof_kernel_name(id), id < bliss_prof_kernel_count().  bliss_prof_read synchronises on the
 * recorded events and returns the summed duration and the number of launches since the last reset. */
int bliss_prof_enable(int kernel_id);
int bliss_prof_reset(void);
int bliss_prof_read(int kernel_id, double* total_ms, int64_t* launches);
int bliss_prof_kernel_count(void);
const char* bliss_prof_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif
