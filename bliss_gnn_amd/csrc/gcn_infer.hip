// GraphConv(norm='both') full-neighbour inference straight off the graph's CSC, gfx950.
//
// GCN.inference walks the nodes in contiguous batches of `batch_size` rows and runs every layer on the batch's full-neighbour
// block; GraphConv divides by the BLOCK's out-degrees, so a row's value depends on which destinations share its batch.  The
// batch structure is a pure function of indptr and batch_size, so the block path's bits can be had without building a block:
//     batch b     = rows [b * bs, min(V, (b + 1) * bs)),  first edge E0_b = indptr[b * bs],  n_b edges
//     cnt(b, j)   = CSC positions in [E0_b, E0_b + n_b) whose source is j          (parallel edges count once each)
//     ns_e        = 1 / sqrt(max(cnt(b, indices[e]), 1))       nd_i = 1 / sqrt(max(indeg_i, 1))      (k_gcn_norms' expressions)
//     out[i, :]   = bf16( nd_i * sum_e ns_e * h[indices[e], :] )
// with the fp32 sum in the order k_gcn_spmm + k_gcn_fixup produce on the batch's block: the batch's edges are cut into chunks of
// EC_b = spmm_chunk_edges(n_b) positions counted from E0_b; a row's terms inside a chunk are added one by one in edge
// order starting from zero, the per-chunk partials of a row are added in chunk order starting from the first partial; one
// product with nd_i and one rounding at the store.
//
// k_gi_src_norms: a thread per edge of a destination range.  The range's slice of `indices` is sorted by source with
// bliss_block_transpose (stable: inside a source's list the positions ascend, hence so do the batches); the thread finds its
// row -- hence its batch -- by bisecting indptr, and cnt as the number of entries of its source's list that lie in the batch's
// position interval: two lower bounds.  Integers only, no atomics, no per-batch counters.
// k_gi_spmm: a wave per destination row.  The wave walks the row's edges 64 at a time (index and coefficient fetched coalesced
// and broadcast by v_readlane, a lane owns 4 consecutive bf16 features, as in k_gcn_spmm; eight neighbour rows in flight: the
// loads of a group do not wait for the chunk grid) and closes a partial wherever the batch's chunk grid cuts the row, so the sum
// above comes out of registers: no partial rows in memory, no fix-up launch, no float atomics, no tickets, no spin waits.
// A row is one wave's work: a launch lasts at least as long as its longest row (DESIGN.md section 27 has the figures).
#include "common.cuh"
#include "spmm_walk.cuh"
#include "bliss_gnn.h"

namespace {

#define GI_TPB 256

using namespace spmm_walk;       // the row primitives, and the chunk rule the block path cuts a batch's edges by

struct Range {
  const long long* indptr; const int* indices; int V, bs, row0, n_rows;
  long long edge0; int n_edges;
};

// first position in list[a, z) whose entry is >= x
__device__ __forceinline__ int lower_bound(const int* __restrict__ list, int a, int z, int x) {
  while (a < z) {
    const int mid = a + ((z - a) >> 1);
    if (list[mid] < x) a = mid + 1; else z = mid;
  }
  return a;
}

__global__ void __launch_bounds__(GI_TPB) k_gi_src_norms(Range g, const int* __restrict__ t_indptr, const int* __restrict__ t_edge,
                                                        float* __restrict__ ns) {
  const long long tt = (long long)blockIdx.x * GI_TPB + threadIdx.x;
  if (tt >= g.n_edges) return;
  const int t = (int)tt;
  const long long p = g.edge0 + t;
  int lo = g.row0, hi = g.row0 + g.n_rows;                   // the last row of the range that starts at or before p
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (g.indptr[mid] <= p) lo = mid; else hi = mid;
  }
  const long long b0 = (long long)(lo / g.bs) * g.bs;
  const long long b1 = b0 + g.bs < g.V ? b0 + g.bs : g.V;
  long long e_lo = g.indptr[b0] - g.edge0, e_hi = g.indptr[b1] - g.edge0;      // the batch's positions, relative to the range
  e_lo = e_lo < 0 ? 0 : (e_lo > g.n_edges ? g.n_edges : e_lo);
  e_hi = e_hi < 0 ? 0 : (e_hi > g.n_edges ? g.n_edges : e_hi);
  const int j = g.indices[p];
  int c = 1;
  if ((unsigned)j < (unsigned)g.V) {
    const int a = t_indptr[j], z = t_indptr[j + 1];
    c = lower_bound(t_edge, a, z, (int)e_hi) - lower_bound(t_edge, a, z, (int)e_lo);
  }
  ns[t] = 1.0f / sqrtf((float)(c > 1 ? c : 1));
}

// a partial ends (a cut of the batch's chunk grid inside the row, or the row's end): the first partial starts the row's sum, the
// later ones are added to it in chunk order
__device__ __forceinline__ void gi_close(f4& acc, f4& sum, bool& first) {
  if (first) { sum = acc; first = false; }
  else { sum.x += acc.x; sum.y += acc.y; sum.z += acc.z; sum.w += acc.w; }
  acc.x = acc.y = acc.z = acc.w = 0.f;
}

// N consecutive edges of a row, lanes j .. j + N - 1 of the fetched window, batch-relative positions q0 .. q0 + N - 1: the N
// neighbour rows leave together, then the terms are added in edge order; a position on the chunk grid (mask ecm) that is not the
// row's first closes the partial in front of it
template <bool VEC4, int N>
__device__ __forceinline__ void gi_group(const bf16_t* __restrict__ h, int64_t h_stride, int col, bool act, int my_n, float my_c, int j,
                                         int q0, int rs, int ecm, f4& acc, f4& sum, bool& first) {
  int nn[N];
  float kk[N];
  f4 a[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { nn[k] = bcast_i(my_n, j + k); kk[k] = bcast_f(my_c, j + k); a[k] = {0.f, 0.f, 0.f, 0.f}; }
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
    if ((q & ecm) == 0 && q != rs) gi_close(acc, sum, first);
    if (act) {
      acc.x += kk[k] * a[k].x;
      if (VEC4) { acc.y += kk[k] * a[k].y; acc.z += kk[k] * a[k].z; acc.w += kk[k] * a[k].w; }
    }
  }
}

template <bool VEC4>
__global__ void __launch_bounds__(GI_TPB) k_gi_spmm(Range g, const float* __restrict__ ns, const bf16_t* __restrict__ h, int64_t h_stride,
                                                   int dim, bf16_t* __restrict__ out, int64_t out_stride) {
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (GI_TPB / 64) + (threadIdx.x >> 6));
  if (w >= g.n_rows) return;
  const int r = g.row0 + w;
  const long long rs_abs = g.indptr[r], re_abs = g.indptr[r + 1];
  bf16_t* po = out + (int64_t)w * out_stride;
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  if (re_abs <= rs_abs) {                                     // a row without edges
    for (int col = lane * W; col < dim; col += 64 * W) store_row<VEC4, false>(po, col, zero, 1.0f);
    return;
  }
  const long long b0 = (long long)(r / g.bs) * g.bs;
  const long long b1 = b0 + g.bs < g.V ? b0 + g.bs : g.V;
  const long long E0 = g.indptr[b0], E1 = g.indptr[b1];
  if (E0 < g.edge0 || E1 > g.edge0 + g.n_edges || rs_abs < E0 || re_abs > E1) return;     // not the range the caller stated
  const int EC = spmm_chunk_edges((int)(E1 - E0));
  const int rs = (int)(rs_abs - E0), re = (int)(re_abs - E0);                              // relative to the batch's first edge
  const int deg = re - rs;
  const float nd = 1.0f / sqrtf((float)(deg > 1 ? deg : 1));
  const int* __restrict__ idx = g.indices + E0;
  const float* __restrict__ cf = ns + (E0 - g.edge0);
  for (int col0 = 0; col0 < dim; col0 += 64 * W) {
    const int col = col0 + lane * W;
    const bool act = col < dim;
    f4 sum = zero, acc = zero;
    bool first = true;
    for (int t0 = rs; t0 < re; t0 += 64) {
      const int n = re - t0 < 64 ? re - t0 : 64;
      int my_n = 0;
      float my_c = 0.f;
      if (lane < n) { my_n = idx[t0 + lane]; my_c = cf[t0 + lane]; }
      int j = 0;
      for (; j + 8 <= n; j += 8) gi_group<VEC4, 8>(h, h_stride, col, act, my_n, my_c, j, t0 + j, rs, EC - 1, acc, sum, first);
      if (j + 4 <= n) { gi_group<VEC4, 4>(h, h_stride, col, act, my_n, my_c, j, t0 + j, rs, EC - 1, acc, sum, first); j += 4; }
      for (; j < n; ++j) gi_group<VEC4, 1>(h, h_stride, col, act, my_n, my_c, j, t0 + j, rs, EC - 1, acc, sum, first);
    }
    gi_close(acc, sum, first);                                // the row ends: its last partial
    if (act) store_row<VEC4, false>(po, col, sum, nd);
  }
}

bool gi_fill(const bliss_gcn_infer_t* a, Range* g) {
  if (!a || !a->indptr || !a->indices || a->n_nodes <= 0 || a->batch_size < 1) return false;
  if (a->row0 < 0 || a->n_rows < 0 || (long long)a->row0 + a->n_rows > a->n_nodes) return false;
  if (a->row0 % a->batch_size != 0) return false;                                  // a range holds whole batches
  const long long end = (long long)a->row0 + a->n_rows;
  if (end != a->n_nodes && end % a->batch_size != 0) return false;
  if (a->edge0 < 0 || a->n_edges < 0 || a->n_edges >= (1ll << 31)) return false;
  if (((uintptr_t)a->indptr) % 8 != 0 || ((uintptr_t)a->indices) % 4 != 0 || ((uintptr_t)a->ns) % 4 != 0) return false;
  if (a->n_edges > 0 && !a->ns) return false;
  g->indptr = (const long long*)a->indptr; g->indices = a->indices; g->V = a->n_nodes; g->bs = a->batch_size;
  g->row0 = a->row0; g->n_rows = a->n_rows; g->edge0 = a->edge0; g->n_edges = (int)a->n_edges;
  return true;
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int bliss_gcn_infer_chunk_edges(int32_t n_batch_edges) { return spmm_chunk_edges(n_batch_edges); }

int bliss_gcn_infer_src_norms(const bliss_gcn_infer_t* args, void* stream) {
  Range g;
  if (!gi_fill(args, &g)) return BLISS_EINVAL;
  if (g.n_rows == 0 || g.n_edges == 0) return 0;
  if (!args->t_indptr || !args->t_edge || !args->temp) return BLISS_EINVAL;
  if (((uintptr_t)args->t_indptr) % 4 != 0 || ((uintptr_t)args->t_edge) % 4 != 0 || ((uintptr_t)args->temp) % 4 != 0) return BLISS_EINVAL;
  if (args->temp_bytes < (int64_t)(3 * up256((size_t)g.n_edges * 4))) return BLISS_EINVAL;
  const int64_t need = bliss_block_transpose_temp_bytes(g.n_edges, g.V);
  if (need < 0 || args->temp_bytes < need) return BLISS_EINVAL;
  const int rc = bliss_block_transpose(g.indices + g.edge0, nullptr, g.n_edges, g.n_edges, g.V, args->t_indptr, args->t_edge, args->temp,
                                       args->temp_bytes, stream);
  if (rc != 0) return rc;
  k_gi_src_norms<<<(unsigned)(((long long)g.n_edges + GI_TPB - 1) / GI_TPB), GI_TPB, 0, (hipStream_t)stream>>>(g, args->t_indptr, args->t_edge,
                                                                                                              args->ns);
  return (int)hipGetLastError();
}

int bliss_gcn_infer_spmm(const bliss_gcn_infer_t* args, void* stream) {
  Range g;
  if (!gi_fill(args, &g)) return BLISS_EINVAL;
  if (!args->h || !args->out || args->dim <= 0 || args->h_stride < args->dim || args->out_stride < args->dim) return BLISS_EINVAL;
  if (((uintptr_t)args->h) % 2 != 0 || ((uintptr_t)args->out) % 2 != 0) return BLISS_EINVAL;
  if (g.n_rows == 0) return 0;
  const int dim = args->dim;
  const bool vec4 = (dim % 4 == 0) && (args->h_stride % 4 == 0) && (args->out_stride % 4 == 0) && (((uintptr_t)args->h) % 8 == 0) &&
                    (((uintptr_t)args->out) % 8 == 0);
  const dim3 grid((g.n_rows + GI_TPB / 64 - 1) / (GI_TPB / 64)), block(GI_TPB);
  hipStream_t st = (hipStream_t)stream;
  if (vec4) k_gi_spmm<true><<<grid, block, 0, st>>>(g, args->ns, (const bf16_t*)args->h, args->h_stride, dim, (bf16_t*)args->out, args->out_stride);
  else k_gi_spmm<false><<<grid, block, 0, st>>>(g, args->ns, (const bf16_t*)args->h, args->h_stride, dim, (bf16_t*)args->out, args->out_stride);
  return (int)hipGetLastError();
}

}  // extern "C"
