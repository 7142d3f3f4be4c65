// SAGEConv full-neighbour inference straight off the graph's CSC, gfx950.
//
// SAGE.inference(path="blocks") walks the nodes in contiguous batches of `batch_size` rows and runs every layer on the batch's
// full-neighbour block: bliss_spmm_fwd(mean = 1, w = NULL) for 'mean', bliss_spmm_max_fwd(w = NULL) for 'pool'.  Both cut the
// BATCH's edges into chunks, so the fp32 sum order of a 'mean' row depends on where the row lies in its batch.  The batch structure
// is a pure function of indptr and batch_size, so the block path's bits can be had without building a block:
//     batch b   = rows [b * bs, min(V, (b + 1) * bs)),  first edge E0_b = indptr[b * bs],  n_b edges,  EC_b = spmm_chunk_edges(n_b)
//     mean:  out[i, :] = bf16( (1 / max(deg_i, 1)) * S_i ),  S_i the fp32 sum of h[indices[e], :] over the row's edges: the batch's
//            positions are cut into chunks of EC_b counted from E0_b; inside a chunk a row's terms are added one by one in edge
//            order starting from +0; a row's chunk partials are added in chunk order starting from the first partial; one product
//            with the scale, one rounding at the store.  (The block kernel's unweighted coefficient is 1.0f * x, which is exact:
//            plain additions give its bits.)
//     max:   out[i, c] = h[indices[e], c] of the running best that starts at the row's first edge and moves on strict > (float
//            compare) in edge order: the chunk grid does not enter the value (a chunk's partial is the best of its edges under the
//            same rule, combined in chunk order).  No winning edge is recorded.
//     a row without edges is +0 under both.
//
// k_si_spmm: a wave per destination row, as k_gi_spmm of gcn_infer.hip: the row's indices fetched 64 at a time (coalesced) and
// broadcast by v_readlane, a lane owns 4 consecutive bf16 features (or one: the same bits), eight neighbour rows in flight, a
// partial closed wherever the batch's chunk grid cuts the row.  No block, no dst array, no partial rows in memory, no fix-up
// launch, no float atomics.  A row is one wave's work: a launch lasts at least as long as its longest row.
#include "common.cuh"
#include "spmm_walk.cuh"
#include "bliss_gnn.h"

namespace {

#define SI_TPB 256

using namespace spmm_walk;       // the row primitives, and the chunk rule the block path cuts a batch's edges by

struct Range {
  const long long* indptr; const int* indices; int V, bs, row0, n_rows;
  long long edge0; int n_edges;
};

// mean: a partial ends (a cut of the batch's chunk grid inside the row, or the row's end): the first partial starts the row's
// sum, the later ones are added to it in chunk order
__device__ __forceinline__ void si_close(f4& acc, f4& sum, bool& first) {
  if (first) { sum = acc; first = false; }
  else { sum.x += acc.x; sum.y += acc.y; sum.z += acc.z; sum.w += acc.w; }
  acc.x = acc.y = acc.z = acc.w = 0.f;
}

// max: the row's first edge takes the slot, a later one only on strict >
__device__ __forceinline__ void si_take(float& best, float m, bool row_start) { best = (row_start || m > best) ? m : best; }

// N consecutive edges of a row, lanes j .. j + N - 1 of the fetched window, batch-relative positions q0 .. q0 + N - 1: the N
// neighbour rows leave together, then the terms enter in edge order.  mean: a position on the chunk grid (mask ecm) that is not
// the row's first closes the partial in front of it; acc holds the open partial.  max: acc holds the running best.
template <bool VEC4, bool MAX, int N>
__device__ __forceinline__ void si_group(const bf16_t* __restrict__ h, int64_t h_stride, int col, bool act, int my_n, int j, int q0, int rs,
                                         int ecm, f4& acc, f4& sum, bool& first) {
  int nn[N];
  f4 a[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { nn[k] = bcast_i(my_n, j + k); a[k] = {0.f, 0.f, 0.f, 0.f}; }
  if (act) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (VEC4) a[k] = load4(h + nn[k] * h_stride + col);
      else a[k].x = bf2f(h[nn[k] * h_stride + col]);
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int q = q0 + k;
    if (MAX) {
      const bool start = q == rs;
      si_take(acc.x, a[k].x, start);
      if (VEC4) { si_take(acc.y, a[k].y, start); si_take(acc.z, a[k].z, start); si_take(acc.w, a[k].w, start); }
    } else {
      if ((q & ecm) == 0 && q != rs) si_close(acc, sum, first);
      acc.x += a[k].x;
      if (VEC4) { acc.y += a[k].y; acc.z += a[k].z; acc.w += a[k].w; }
    }
  }
}

template <bool VEC4, bool MAX>
__global__ void __launch_bounds__(SI_TPB) k_si_spmm(Range g, const bf16_t* __restrict__ h, int64_t h_stride, int dim, bf16_t* __restrict__ out,
                                                   int64_t out_stride) {
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (SI_TPB / 64) + (threadIdx.x >> 6));
  if (w >= g.n_rows) return;
  const int r = g.row0 + w;
  const long long rs_abs = g.indptr[r], re_abs = g.indptr[r + 1];
  const long long b0 = (long long)(r / g.bs) * g.bs;
  const long long b1 = b0 + g.bs < g.V ? b0 + g.bs : g.V;
  const long long E0 = g.indptr[b0], E1 = g.indptr[b1];
  if (E0 < g.edge0 || E1 > g.edge0 + g.n_edges || rs_abs < E0 || re_abs > E1) return;     // not the range the caller stated
  bf16_t* po = out + (int64_t)w * out_stride;
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  if (re_abs <= rs_abs) {                                     // a row without edges
    for (int col = lane * W; col < dim; col += 64 * W) store_row<VEC4, false>(po, col, zero, 1.0f);
    return;
  }
  const int EC = spmm_chunk_edges((int)(E1 - E0));
  const int rs = (int)(rs_abs - E0), re = (int)(re_abs - E0);                              // relative to the batch's first edge
  const int deg = re - rs;
  const float scale = MAX ? 1.0f : 1.0f / (float)(deg > 1 ? deg : 1);
  const int* __restrict__ idx = g.indices + E0;
  for (int col0 = 0; col0 < dim; col0 += 64 * W) {
    const int col = col0 + lane * W;
    const bool act = col < dim;
    f4 sum = zero, acc = zero;
    bool first = true;
    for (int t0 = rs; t0 < re; t0 += 64) {
      const int n = re - t0 < 64 ? re - t0 : 64;
      int my_n = 0;
      if (lane < n) my_n = idx[t0 + lane];
      int j = 0;
      for (; j + 8 <= n; j += 8) si_group<VEC4, MAX, 8>(h, h_stride, col, act, my_n, j, t0 + j, rs, EC - 1, acc, sum, first);
      if (j + 4 <= n) { si_group<VEC4, MAX, 4>(h, h_stride, col, act, my_n, j, t0 + j, rs, EC - 1, acc, sum, first); j += 4; }
      for (; j < n; ++j) si_group<VEC4, MAX, 1>(h, h_stride, col, act, my_n, j, t0 + j, rs, EC - 1, acc, sum, first);
    }
    if (MAX) sum = acc;                                       // the best of the row: a bf16 value, stored as it is
    else si_close(acc, sum, first);                           // the row ends: its last partial
    if (act) store_row<VEC4, false>(po, col, sum, scale);
  }
}

bool si_fill(const bliss_sage_infer_t* a, Range* g) {
  if (!a || !a->indptr || !a->indices || a->n_nodes <= 0 || a->batch_size < 1) return false;
  if (a->row0 < 0 || a->n_rows < 0 || (long long)a->row0 + a->n_rows > a->n_nodes) return false;
  if (a->row0 % a->batch_size != 0) return false;                                  // a range holds whole batches
  const long long end = (long long)a->row0 + a->n_rows;
  if (end != a->n_nodes && end % a->batch_size != 0) return false;
  if (a->edge0 < 0 || a->n_edges < 0 || a->n_edges >= (1ll << 31)) return false;
  if (((uintptr_t)a->indptr) % 8 != 0 || ((uintptr_t)a->indices) % 4 != 0) return false;
  if (a->reduce != BLISS_SAGE_INFER_MEAN && a->reduce != BLISS_SAGE_INFER_MAX) return false;
  if (!a->h || !a->out || a->dim <= 0 || a->h_stride < a->dim || a->out_stride < a->dim) return false;
  if (((uintptr_t)a->h) % 2 != 0 || ((uintptr_t)a->out) % 2 != 0) return false;
  g->indptr = (const long long*)a->indptr; g->indices = a->indices; g->V = a->n_nodes; g->bs = a->batch_size;
  g->row0 = a->row0; g->n_rows = a->n_rows; g->edge0 = a->edge0; g->n_edges = (int)a->n_edges;
  return true;
}

}  // namespace

extern "C" {

int bliss_sage_infer_spmm(const bliss_sage_infer_t* args, void* stream) {
  Range g;
  if (!si_fill(args, &g)) return BLISS_EINVAL;
  if (g.n_rows == 0) return 0;
  const int dim = args->dim;
  const bool vec4 = (dim % 4 == 0) && (args->h_stride % 4 == 0) && (args->out_stride % 4 == 0) && (((uintptr_t)args->h) % 8 == 0) &&
                    (((uintptr_t)args->out) % 8 == 0);
  const dim3 grid((g.n_rows + SI_TPB / 64 - 1) / (SI_TPB / 64)), block(SI_TPB);
  hipStream_t st = (hipStream_t)stream;
  const bf16_t* h = (const bf16_t*)args->h;
  bf16_t* out = (bf16_t*)args->out;
#define GO(V, M) k_si_spmm<V, M><<<grid, block, 0, st>>>(g, h, args->h_stride, dim, out, args->out_stride)
  if (args->reduce == BLISS_SAGE_INFER_MAX) { if (vec4) GO(true, true); else GO(false, true); }
  else { if (vec4) GO(true, false); else GO(false, false); }
#undef GO
  return (int)hipGetLastError();
}

}  // extern "C"
