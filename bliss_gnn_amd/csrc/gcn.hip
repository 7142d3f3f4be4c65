// dglnn.GraphConv(norm='both') on bounded kernels, gfx950.
//
// The reference's GCN (model.py:386-439) stacks GraphConv layers with the sampler's edge weights.  The library path of
// nn.GraphConv runs the degree normalisation as torch ops (index_add_, pow, two row scalings with bf16 intermediates); here the
// normalisation rides in the message passing itself:
//     ns_j = 1 / sqrt(max(outdeg_j, 1))   outdeg_j = t_indptr[j+1] - t_indptr[j]   (the block's by-source index)
//     nd_i = 1 / sqrt(max(indeg_i, 1))    indeg_i  = indptr[i+1] - indptr[i]
//     fwd:  out[i, :] = bf16( nd_i * sum_{e in row i}    (float(w_e) * ns[src_e]) * h[src_e, :] )
//     bwd:  gh[j, :]  = bf16( ns_j * sum_{e : src_e = j} (float(w_e) * nd[dst_e]) * g[dst_e, :] )
// ns / nd are fp32 (IEEE sqrt, one division), the coefficient is ONE fp32 product, the sum is fp32 in edge order inside a work
// chunk with the chunk partials added in chunk order, and there is ONE rounding to bf16 at the store.  Degrees are structural:
// the edge weights do not enter them.
//
// k_gcn_norms writes both norm vectors in one coalesced launch (computed once per block: looking the degrees up per edge would
// put two more dependent loads into every edge's chain).  k_gcn_spmm is the balanced traversal of spmm_walk.cuh (the one SAGEConv
// runs in spmm.hip) with the coefficient gathered beside the weight (GcnPolicy); k_gcn_fixup is its fix-up: it adds the partials
// of cut rows in chunk order and clears rows without edges.  No float atomics, no tickets, no spin waits; nothing at or past the
// live edge count is read.
//
// k_gcn_epilogue_fwd / _bwd are the row-wise tail of a layer, bounded by the block's live row count: bias add, ReLU, the keyed
// dropout mask of gat_glue.hip (drop_hash(seed, launch counter, r * width + c): no row's mask depends on the capacity), the
// next block's row norms in k_embed_norm's summation order; the backward also reduces the bias gradient over fixed chunks of
// GE_DB_ROWS rows (fp32 partials, summed in chunk order, one rounding).
#include "common.cuh"
#include "spmm_walk.cuh"
#include "bliss_gnn.h"

namespace {

using namespace spmm_walk;

#define GC_TPB 256
#define GE_DB_ROWS 32

// ns[j] (j < n_src) and nd[i] (i < n_dst) in one launch; rows past the live counts are empty in both index arrays: norm 1
__global__ void __launch_bounds__(GC_TPB) k_gcn_norms(const int* __restrict__ indptr, int n_dst, const int* __restrict__ t_indptr, int n_src,
                                                     float* __restrict__ nd, float* __restrict__ ns) {
  const int i = blockIdx.x * GC_TPB + threadIdx.x;
  if (i < n_src) {
    const int d = t_indptr[i + 1] - t_indptr[i];
    ns[i] = 1.0f / sqrtf((float)(d > 1 ? d : 1));
  } else if (i < n_src + n_dst) {
    const int r = i - n_src;
    const int d = indptr[r + 1] - indptr[r];
    nd[r] = 1.0f / sqrtf((float)(d > 1 ? d : 1));
  }
}

// GraphConv's coefficients on the shared walk (spmm_walk.cuh); k_gcn_spmm hands n_nbr / n_row over by direction:
// FWD: coefficient = w[e] * ns[src[e]], store scale nd[row]
// BWD: coefficient = w[e] * nd[dst[e]], store scale ns[row]
template <bool BWD>
struct GcnPolicy {
  const float* n_nbr;
  const float* n_row;
  __device__ __forceinline__ float coef(float c, int s, int d) const { return c * n_nbr[BWD ? d : s]; }
  __device__ __forceinline__ float scale(int r, int rb, int re) const { return n_row[r]; }
};

template <bool VEC4, bool BWD>
__global__ void __launch_bounds__(GC_TPB) k_gcn_spmm(const int* __restrict__ row_ptr, const int* __restrict__ t_edge,
                                                    const int* __restrict__ src, const int* __restrict__ dst,
                                                    const bf16_t* __restrict__ w, const float* __restrict__ n_nbr,
                                                    const float* __restrict__ n_row, const bf16_t* __restrict__ h, int64_t h_stride,
                                                    const int* __restrict__ nnz_dev, int nnz_host, int dim, bf16_t* __restrict__ out,
                                                    int64_t out_stride, float* __restrict__ part, int EC) {
  int nnz = nnz_host;
  if (nnz_dev) { const int t = *nnz_dev; nnz = t < nnz ? t : nnz; }
  if (nnz < 0) nnz = 0;                                     // a negative device count is no edges
  const int ci = blockIdx.x * (GC_TPB / 64) + (threadIdx.x >> 6);
  const int nchunks = (nnz + EC - 1) / EC;
  if (ci >= nchunks) return;
  chunk<VEC4, false, BWD>(GcnPolicy<BWD>{n_nbr, n_row}, ci, nnz, EC, row_ptr, t_edge, src, dst, w, h, h_stride, dim, out, out_stride,
                          part);
}

template <bool VEC4>
__global__ void __launch_bounds__(GC_TPB) k_gcn_fixup(const int* __restrict__ row_ptr, int n_rows, int dim, const float* __restrict__ n_row,
                                                     const float* __restrict__ part, bf16_t* __restrict__ out, int64_t out_stride, int EC) {
  const int r = blockIdx.x * (GC_TPB / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  fixup<VEC4, false>(GcnPolicy<false>{nullptr, n_row}, r, row_ptr, dim, part, out, out_stride, EC);     // the fix-up asks scale() only
}

// What this launcher does differently from spmm.hip's launch_spmm, on purpose:
//   * nnz == 0 launches no main kernel, only the fix-up that clears the rows (SAGE launches one idle chunk);
//   * k_gcn_spmm clamps a negative device-side count to 0 (SAGE takes the count as it is);
//   * the entry points require `partials` whenever nnz > 0 (SAGE: only when nnz > EC);
//   * ONE vec4 decision for both kernels, with the alignment of `part` folded in (SAGE decides the fix-up's separately);
//   * only n_rows == 0 returns early; dim <= 0 is refused by the entry points.
template <bool BWD>
int launch_gcn_spmm(const int* row_ptr, const int* t_edge, const int* src, const int* dst, const void* w, const float* n_nbr,
                    const float* n_row, const void* h, int64_t h_stride, int n_rows, const int* nnz_dev, int nnz, int dim, void* out,
                    int64_t out_stride, float* part, hipStream_t st) {
  if (n_rows == 0) return 0;
  const int EC = spmm_chunk_edges(nnz);
  const bool vec4 = (dim % 4 == 0) && (h_stride % 4 == 0) && (out_stride % 4 == 0) && (((uintptr_t)h) % 8 == 0) &&
                    (((uintptr_t)out) % 8 == 0) && (((uintptr_t)part) % 16 == 0);
  const int nchunks = (nnz + EC - 1) / EC;
  const dim3 block(GC_TPB), gfix((n_rows + GC_TPB / 64 - 1) / (GC_TPB / 64));
  if (nchunks > 0) {
    const dim3 grid((nchunks + GC_TPB / 64 - 1) / (GC_TPB / 64));
    if (vec4) k_gcn_spmm<true, BWD><<<grid, block, 0, st>>>(row_ptr, t_edge, src, dst, (const bf16_t*)w, n_nbr, n_row, (const bf16_t*)h, h_stride,
                                                            nnz_dev, nnz, dim, (bf16_t*)out, out_stride, part, EC);
    else k_gcn_spmm<false, BWD><<<grid, block, 0, st>>>(row_ptr, t_edge, src, dst, (const bf16_t*)w, n_nbr, n_row, (const bf16_t*)h, h_stride,
                                                        nnz_dev, nnz, dim, (bf16_t*)out, out_stride, part, EC);
  }
  if (vec4) k_gcn_fixup<true><<<gfix, block, 0, st>>>(row_ptr, n_rows, dim, n_row, part, (bf16_t*)out, out_stride, EC);
  else k_gcn_fixup<false><<<gfix, block, 0, st>>>(row_ptr, n_rows, dim, n_row, part, (bf16_t*)out, out_stride, EC);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------ epilogue
struct Epi {
  const bf16_t* a; long long a_stride;
  const bf16_t* bias;
  int n_rows; const int* rows_dev; int width; int relu;
  unsigned drop_thresh; float drop_scale; unsigned seed; unsigned long long* ctr; unsigned* ctr_used;
  bf16_t* out; long long out_stride;
  bf16_t* norm_out;
  const bf16_t* dout; long long dout_stride;
  bf16_t* din; long long din_stride;
  bf16_t* db; float* db_part;
  int q4, vec;                 // q4: a lane owns 4 consecutive columns (k_embed_norm's order for this `out`); vec: 8-byte accesses
};

__device__ __forceinline__ int ge_live(const Epi& p) {
  int n = p.n_rows;
  if (p.rows_dev) { const int t = *p.rows_dev; n = t < n ? t : n; }
  return n < 0 ? 0 : n;
}

// one wave per row: x = bf16(a + bias), ReLU, keyed dropout, the row norm of what is stored; zero rows at or past the count
__global__ void __launch_bounds__(GC_TPB) k_gcn_epilogue_fwd(Epi p) {
  const int lane = lane_id();
  const int row = blockIdx.x * (GC_TPB / 64) + (threadIdx.x >> 6);
  const int n = ge_live(p);
  const uint32_t ctr = p.drop_thresh ? (uint32_t)__hip_atomic_load(p.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  if (p.drop_thresh && p.ctr_used && blockIdx.x == 0 && threadIdx.x == 0) *p.ctr_used = ctr;
  if (row >= p.n_rows) return;
  const int W = p.q4 ? 4 : 1, dim = p.width;
  bf16_t* po = p.out + row * p.out_stride;
  if (row >= n) {                                       // capacity padding: zeros, nothing read
    for (int col = lane * W; col < dim; col += 64 * W) {
      if (p.vec) *reinterpret_cast<uint2*>(po + col) = make_uint2(0u, 0u);
      else for (int i = 0; i < W; ++i) po[col + i] = 0;
    }
    if (lane == 0 && p.norm_out) p.norm_out[row] = 0;
    return;
  }
  const bf16_t* pa = p.a + row * p.a_stride;
  float s = 0.f;
  for (int col = lane * W; col < dim; col += 64 * W) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.vec) {
      const f4 x = load4(pa + col);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else for (int i = 0; i < W; ++i) v[i] = bf2f(pa[col + i]);
    for (int i = 0; i < W; ++i) {
      float t = v[i];
      if (p.bias) t = rbf(t + bf2f(p.bias[col + i]));
      if (p.relu) t = t > 0.f ? t : 0.f;
      if (p.drop_thresh) {
        const bool keep = drop_hash(p.seed, ctr, (uint32_t)row * (uint32_t)dim + (uint32_t)(col + i)) >= p.drop_thresh;
        t = keep ? rbf(t * p.drop_scale) : 0.f;
      }
      v[i] = t;
      s += t * t;
    }
    if (p.vec) { f4 o = {v[0], v[1], v[2], v[3]}; store4<false>(po, col, o); }
    else for (int i = 0; i < W; ++i) po[col + i] = f2bf(v[i]);
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0 && p.norm_out) p.norm_out[row] = f2bf(sqrtf(s));
}

__global__ void k_gcn_epilogue_bump(unsigned long long* ctr) { if (threadIdx.x == 0) *ctr += 1ull; }

// one workgroup per chunk of GE_DB_ROWS rows, a thread per column: g_pre = mask / scale, then the ReLU derivative from the
// stored output; zero rows past the count; the chunk's column sums of g_pre (row order, fp32) into db_part[chunk][c]
__global__ void __launch_bounds__(GC_TPB) k_gcn_epilogue_bwd(Epi p) {
  const int n = ge_live(p);
  const int r0 = blockIdx.x * GE_DB_ROWS, r1 = min(p.n_rows, r0 + GE_DB_ROWS);
  const uint32_t ctr = p.drop_thresh ? *p.ctr_used : 0u;
  for (int c = threadIdx.x; c < p.width; c += GC_TPB) {
    float sum = 0.f;
    for (int r = r0; r < r1; ++r) {
      bf16_t* pd = p.din + r * p.din_stride + c;
      if (r >= n) { *pd = 0; continue; }
      float g = bf2f(p.dout[r * p.dout_stride + c]);
      if (p.drop_thresh) g = drop_hash(p.seed, ctr, (uint32_t)r * (uint32_t)p.width + (uint32_t)c) >= p.drop_thresh ? rbf(g * p.drop_scale) : 0.f;
      if (p.relu) g = bf2f(p.out[r * p.out_stride + c]) > 0.f ? g : 0.f;
      *pd = f2bf(g);
      sum += g;
    }
    if (p.db_part && r0 < n) p.db_part[(long long)blockIdx.x * p.width + c] = sum;
  }
}

// db[c] = bf16( sum over the chunks that hold live rows, in chunk order )
__global__ void __launch_bounds__(GC_TPB) k_gcn_db_reduce(Epi p) {
  const int n = ge_live(p);
  const int nch = (n + GE_DB_ROWS - 1) / GE_DB_ROWS;
  const int c = blockIdx.x * GC_TPB + threadIdx.x;
  if (c >= p.width) return;
  float s = 0.f;
  for (int ch = 0; ch < nch; ++ch) s += p.db_part[(long long)ch * p.width + c];
  p.db[c] = f2bf(s);
}

inline bool al8(const void* ptr, long long stride) { return ptr == nullptr || ((((uintptr_t)ptr) % 8 == 0) && (stride % 4 == 0)); }

bool ge_fill(const bliss_gcn_epilogue_t* a, Epi* p, bool backward) {
  if (!a || a->n_rows <= 0 || a->width <= 0 || a->drop_p < 0.f || a->drop_p >= 1.f) return false;
  if ((long long)a->n_rows * a->width >= (1ll << 32)) return false;
  if (!backward && (!a->a || !a->out || a->a_stride < a->width || a->out_stride < a->width)) return false;
  if (!backward && a->drop_p > 0.f && (!a->drop_ctr || !a->drop_ctr_used)) return false;
  if (backward && (!a->dout || !a->din || a->dout_stride < a->width || a->din_stride < a->width)) return false;
  if (backward && a->relu && (!a->out || a->out_stride < a->width)) return false;
  if (backward && a->drop_p > 0.f && !a->drop_ctr_used) return false;
  if (backward && a->db && (!a->db_partials || (((uintptr_t)a->db_partials) % 4) != 0)) return false;
  p->a = (const bf16_t*)a->a; p->a_stride = a->a_stride;
  p->bias = (const bf16_t*)a->bias;
  p->n_rows = a->n_rows; p->rows_dev = a->rows_dev; p->width = a->width; p->relu = a->relu ? 1 : 0;
  p->drop_thresh = a->drop_p > 0.f ? (unsigned)((double)a->drop_p * 4294967296.0) : 0u;
  p->drop_scale = a->drop_p > 0.f ? 1.0f / (1.0f - a->drop_p) : 1.0f;
  p->seed = a->drop_seed; p->ctr = (unsigned long long*)a->drop_ctr; p->ctr_used = a->drop_ctr_used;
  p->out = (bf16_t*)a->out; p->out_stride = a->out_stride;
  p->norm_out = (bf16_t*)a->norm_out;
  p->dout = (const bf16_t*)a->dout; p->dout_stride = a->dout_stride;
  p->din = (bf16_t*)a->din; p->din_stride = a->din_stride;
  p->db = (bf16_t*)a->db; p->db_part = a->db ? a->db_partials : nullptr;
  // the norm's summation order is bliss_embed_norm's for this `out`: 4 columns per lane iff that kernel would take its vec4 path
  p->q4 = (a->width % 4 == 0) && (a->out_stride % 4 == 0) && (((uintptr_t)a->out) % 8 == 0);
  p->vec = p->q4 && al8(a->a, a->a_stride);
  return true;
}

}  // namespace

extern "C" {

int bliss_gcn_db_chunk_rows(void) { return GE_DB_ROWS; }

int bliss_gcn_norms(const int32_t* indptr, int32_t n_dst, const int32_t* t_indptr, int32_t n_src, float* nd, float* ns, void* stream) {
  if (n_dst < 0 || n_src < 0 || (n_dst > 0 && (!indptr || !nd)) || (n_src > 0 && (!t_indptr || !ns))) return BLISS_EINVAL;
  if ((long long)n_dst + n_src >= (1ll << 31)) return BLISS_EINVAL;
  const int total = n_dst + n_src;
  if (total == 0) return 0;
  k_gcn_norms<<<(total + GC_TPB - 1) / GC_TPB, GC_TPB, 0, (hipStream_t)stream>>>(indptr, n_dst, t_indptr, n_src, nd, ns);
  return (int)hipGetLastError();
}

int bliss_gcn_spmm_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const float* ns, const float* nd,
                       const void* h, int64_t h_stride, int32_t n_dst, const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* out,
                       int64_t out_stride, float* partials, void* stream) {
  if (!indptr || !h || !out || !ns || !nd || nnz < 0 || n_dst < 0 || dim <= 0 || h_stride < dim || out_stride < dim) return BLISS_EINVAL;
  if (nnz > 0 && (!src || !dst || !partials)) return BLISS_EINVAL;
  return launch_gcn_spmm<false>(indptr, nullptr, src, dst, w, ns, nd, h, h_stride, n_dst, nnz_dev, nnz, dim, out, out_stride, partials,
                                (hipStream_t)stream);
}

int bliss_gcn_spmm_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w,
                       const float* ns, const float* nd, const void* gout, int64_t gout_stride, int32_t n_src, const int32_t* nnz_dev,
                       int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, float* partials, void* stream) {
  if (!t_indptr || !gout || !gh || !ns || !nd || nnz < 0 || n_src < 0 || dim <= 0 || gout_stride < dim || gh_stride < dim) return BLISS_EINVAL;
  if (nnz > 0 && (!t_edge || !src || !dst || !partials)) return BLISS_EINVAL;
  return launch_gcn_spmm<true>(t_indptr, t_edge, src, dst, w, nd, ns, gout, gout_stride, n_src, nnz_dev, nnz, dim, gh, gh_stride, partials,
                               (hipStream_t)stream);
}

int bliss_gcn_epilogue_fwd(const bliss_gcn_epilogue_t* args, void* stream) {
  Epi p;
  if (!ge_fill(args, &p, false)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  k_gcn_epilogue_fwd<<<(p.n_rows + GC_TPB / 64 - 1) / (GC_TPB / 64), GC_TPB, 0, st>>>(p);
  if (p.drop_thresh) k_gcn_epilogue_bump<<<1, 64, 0, st>>>(p.ctr);
  return (int)hipGetLastError();
}

int bliss_gcn_epilogue_bwd(const bliss_gcn_epilogue_t* args, void* stream) {
  Epi p;
  if (!ge_fill(args, &p, true)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  k_gcn_epilogue_bwd<<<(p.n_rows + GE_DB_ROWS - 1) / GE_DB_ROWS, GC_TPB, 0, st>>>(p);
  if (p.db) k_gcn_db_reduce<<<(p.width + GC_TPB - 1) / GC_TPB, GC_TPB, 0, st>>>(p);
  return (int)hipGetLastError();
}

}  // extern "C"
