// Per-block message passing for SAGEConv('mean') with sampled edge weights, gfx950.
//
// Replaces DGL's g-SpMM behind  graph.update_all(fn.u_mul_e('h','_edge_weight','m'), fn.mean('m','neigh'))
// (dglnn.SAGEConv.forward, called from model.py:321-329) and its autograd backward, plus
// th.norm(h, dim=1) of model.py:318-320.
//
// k_spmm / k_spmm_fixup are the balanced traversal of spmm_walk.cuh with SAGEConv's coefficients (SagePolicy).  The backward
// is a gather too (through the by-source transposed index), so it is deterministic and needs no float atomics.
#include "common.cuh"
#include "spmm_walk.cuh"
#include "bliss_gnn.h"
#include "prof.h"

namespace {

using namespace spmm_walk;

#define SP_TPB 256

// SAGEConv's coefficients on the shared walk (spmm_walk.cuh):
// FWD: coefficient = w[e]            (x 1/deg at the store)
// BWD: coefficient = w[e]/deg(dst[e])
template <bool BWD>
struct SagePolicy {
  const int* blk_indptr;                                    // the block's CSR by destination (BWD with mean only)
  int mean;
  __device__ __forceinline__ float coef(float c, int s, int d) const {
    if (BWD && mean) c = c / (float)max(blk_indptr[d + 1] - blk_indptr[d], 1);
    return c;
  }
  __device__ __forceinline__ float scale(int r, int rb, int re) const {
    return (!BWD && mean) ? 1.0f / (float)max(re - rb, 1) : 1.0f;
  }
};

template <bool VEC4, bool OUT_F32, bool BWD>
__global__ void __launch_bounds__(SP_TPB) k_spmm(const int* __restrict__ row_ptr, const int* __restrict__ t_edge,
                                                const int* __restrict__ src, const int* __restrict__ dst,
                                                const int* __restrict__ blk_indptr, const bf16_t* __restrict__ w,
                                                const bf16_t* __restrict__ h, int64_t h_stride, int n_rows,
                                                const int* __restrict__ nnz_dev, int nnz_host, int dim,
                                                int mean, void* out, int64_t out_stride, float* __restrict__ part, int EC) {
  const int nnz = nnz_dev ? min(*nnz_dev, nnz_host) : nnz_host;
  const int ci = blockIdx.x * (SP_TPB / 64) + (threadIdx.x >> 6);
  const int nchunks = nnz > 0 ? (nnz + EC - 1) / EC : 1;    // no edges: one idle chunk (launch_spmm)
  if (ci >= nchunks) return;
  chunk<VEC4, OUT_F32, BWD>(SagePolicy<BWD>{blk_indptr, mean}, ci, nnz, EC, row_ptr, t_edge, src, dst, w, h, h_stride, dim, out,
                            out_stride, part);
}

template <bool OUT_F32, bool BWD, bool VEC4>
__global__ void __launch_bounds__(SP_TPB) k_spmm_fixup(const int* __restrict__ row_ptr, int n_rows, int dim, int mean,
                                                      const float* __restrict__ part, void* out, int64_t out_stride, int EC) {
  const int r = blockIdx.x * (SP_TPB / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  fixup<VEC4, OUT_F32>(SagePolicy<BWD>{nullptr, mean}, r, row_ptr, dim, part, out, out_stride, EC);
}

// ||h_j||_2 per row  (model.py:318-320)
__global__ void __launch_bounds__(SP_TPB) k_embed_norm(const bf16_t* __restrict__ h, int n_rows, int dim, int64_t stride,
                                                      bf16_t* __restrict__ out, int vec4) {
  const int lane = lane_id();
  const int row = blockIdx.x * (SP_TPB / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const bf16_t* p = h + row * stride;
  float s = 0.f;
  if (vec4) {
    for (int c = lane * 4; c < dim; c += 256) {
      f4 a = load4(p + c);
      s += a.x * a.x; s += a.y * a.y; s += a.z * a.z; s += a.w * a.w;
    }
  } else {
    for (int c = lane; c < dim; c += 64) { float a = bf2f(p[c]); s += a * a; }
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) out[row] = f2bf(sqrtf(s));
}

// ---- feature gather + row norms in one pass ---------------------------------------------------------------------------
// blocks[0].srcdata['features'] = g.ndata['features'][input_nodes] (train_lightning.py:138) and the embed_norm of those rows
// (model.py:318-320): a wave copies one row (W bf16 per lane and access) through its slice of LDS to `out`, then takes the
// sum of squares from LDS in exactly k_embed_norm's order, so the norm has the bits k_embed_norm(out) would give.
// HBM-bound: 2 * K * F bytes in, the same out (SURVEY 8d "feature gather").
template <int W>
__global__ void __launch_bounds__(SP_TPB) k_gather_rows_norm(const bf16_t* __restrict__ feat, int64_t f_stride, const int* __restrict__ ids,
                                                            int n_rows, int dim, bf16_t* __restrict__ out, int64_t o_stride,
                                                            bf16_t* __restrict__ norm_out, int norm_vec4) {
  extern __shared__ __attribute__((aligned(16))) bf16_t rows_sh[];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int row = blockIdx.x * (SP_TPB / 64) + wave;
  if (row >= n_rows) return;                          // wave-uniform; no workgroup barrier below
  const int dpad = (dim + 7) & ~7;
  bf16_t* sh = rows_sh + (size_t)wave * dpad;
  const bf16_t* p = feat + (int64_t)ids[row] * f_stride;
  bf16_t* q = out + (int64_t)row * o_stride;
  if (W == 4) {
    for (int c = lane * 4; c < dim; c += 256) { const uint2 v = *reinterpret_cast<const uint2*>(p + c); *reinterpret_cast<uint2*>(q + c) = v; *reinterpret_cast<uint2*>(sh + c) = v; }
  } else if (W == 2) {
    for (int c = lane * 2; c < dim; c += 128) { const uint32_t v = *reinterpret_cast<const uint32_t*>(p + c); *reinterpret_cast<uint32_t*>(q + c) = v; *reinterpret_cast<uint32_t*>(sh + c) = v; }
  } else {
    for (int c = lane; c < dim; c += 64) { const bf16_t v = p[c]; q[c] = v; sh[c] = v; }
  }
  if (!norm_out) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();                    // the wave's own LDS writes, in order, before its reads
  float s = 0.f;
  if (norm_vec4) {
    for (int c = lane * 4; c < dim; c += 256) {
      const float a = bf2f(sh[c]), b = bf2f(sh[c + 1]), cc = bf2f(sh[c + 2]), d = bf2f(sh[c + 3]);
      s += a * a; s += b * b; s += cc * cc; s += d * d;
    }
  } else {
    for (int c = lane; c < dim; c += 64) { const float a = bf2f(sh[c]); s += a * a; }
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) norm_out[row] = f2bf(sqrtf(s));
}

// ---- SAGE hidden-layer epilogue in one pass ----------------------------------------------------------------------
// model.py:321-333 + :318-320 of the next layer:   rst = fc_self(h_dst) + h_neigh;  h = dropout(relu(rst));  ||h_j||
// The reference runs four element-wise kernels for this; here one wave walks a row once: bf16 add (fp32, one rounding),
// ReLU, dropout (keep with probability 1-p, scale 1/(1-p), one rounding) and the fp32 sum of squares of what it stores
// (the same accumulation order as k_embed_norm).  The dropout bits come from a counter-based hash of (seed, launch
// counter, element index): the same Bernoulli(1-p) law as torch's fused_dropout, a different (device-resident,
// graph-replayable) random stream.  ctr[0] = launch counter, ctr[1] (and ctr[2..65]) = tickets: the last workgroup to finish bumps the
// counter, so every workgroup of a launch has read the same value.  drop_hash: common.cuh.
// VEC4 is the access width (8-byte loads and stores: a, b and out all allow them); NORM4 is the summation order of the norm,
// which follows `out` alone, like bliss_embed_norm(out): a lane owns columns 4l .. 4l + 3 (+ 256 j) and adds their squares in
// turn.  VEC4 implies NORM4.  <false, true> (an `a` or `b` that is only 2-byte aligned beside an aligned `out`) walks the vec4
// order with 2-byte accesses, as k_gather_rows_norm's norm_vec4 does.
template <bool VEC4, bool NORM4>
__global__ void __launch_bounds__(SP_TPB) k_sage_epilogue(const bf16_t* __restrict__ a, int64_t a_stride, const bf16_t* __restrict__ b,
                                                         int64_t b_stride, int n_rows, int dim, uint32_t drop_thresh, float scale,
                                                         uint32_t seed, unsigned long long* ctr, bf16_t* __restrict__ out,
                                                         int64_t out_stride, bf16_t* __restrict__ norm_out) {
  const int lane = lane_id();
  const int row = blockIdx.x * (SP_TPB / 64) + (threadIdx.x >> 6);
  const uint32_t c = drop_thresh ? (uint32_t)__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  if (row < n_rows) {
    const bf16_t *pa = a + row * a_stride, *pb = b + row * b_stride;
    bf16_t* po = out + row * out_stride;
    float s = 0.f;
    static_assert(NORM4 || !VEC4, "8-byte accesses imply the vec4 order");
    constexpr int W = NORM4 ? 4 : 1;
    for (int col = lane * W; col < dim; col += 64 * W) {
      float v[W];
      if (VEC4) {
        const f4 x = load4(pa + col), y = load4(pb + col);
        v[0] = x.x + y.x; v[1 % W] = x.y + y.y; v[2 % W] = x.z + y.z; v[3 % W] = x.w + y.w;
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = bf2f(pa[col + i]) + bf2f(pb[col + i]);     // (NORM4: dim % 4 == 0, col + 3 < dim)
      }
#pragma unroll
      for (int i = 0; i < W; ++i) {
        float t = rbf(v[i]);                                  // the add's bf16 result
        t = t > 0.f ? t : 0.f;                                // relu
        if (drop_thresh) {
          const bool keep = drop_hash(seed, c, (uint32_t)(row * dim + col + i)) >= drop_thresh;
          t = keep ? rbf(t * scale) : 0.f;
        }
        v[i] = t;
        s += t * t;
      }
      if (VEC4) {
        uint2 o;
        o.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1 % W]) << 16);
        o.y = (uint32_t)f2bf(v[2 % W]) | ((uint32_t)f2bf(v[3 % W]) << 16);
        *reinterpret_cast<uint2*>(po + col) = o;
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i) po[col + i] = f2bf(v[i]);
      }
    }
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0 && norm_out) norm_out[row] = f2bf(sqrtf(s));
  }
  if (drop_thresh) {                                          // launch counter: bumped once, by the last workgroup
    // two-level ticket (ctr[2 + g], g = workgroup % 64, then ctr[1]): a same-address atomic costs ~10 ns, and the 1200
    // workgroups of the input layer's launch spent 12 of its 20 us queueing on ONE ticket word
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned G = gridDim.x < 64u ? gridDim.x : 64u, g = blockIdx.x % G;
      const unsigned long long members = (gridDim.x - g + G - 1) / G;
      if (atomicAdd(ctr + 2 + g, 1ull) == members - 1) {
        __hip_atomic_store(ctr + 2 + g, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (atomicAdd(ctr + 1, 1ull) == (unsigned long long)G - 1) {
          __hip_atomic_store(ctr + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          atomicAdd(ctr, 1ull);
        }
      }
    }
  }
}

// d(a) = d(b) = dout * scale where the stored output is positive (kept and past the ReLU), else 0
template <bool VEC4>
__global__ void __launch_bounds__(SP_TPB) k_sage_epilogue_bwd(const bf16_t* __restrict__ dout, int64_t d_stride, const bf16_t* __restrict__ out,
                                                             int64_t out_stride, int n_rows, int dim, float scale,
                                                             bf16_t* __restrict__ din, int64_t din_stride) {
  const int lane = lane_id();
  const int row = blockIdx.x * (SP_TPB / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  constexpr int W = VEC4 ? 4 : 1;
  for (int col = lane * W; col < dim; col += 64 * W) {
    if (VEC4) {
      const f4 g = load4(dout + row * d_stride + col), o = load4(out + row * out_stride + col);
      f4 r;
      r.x = o.x > 0.f ? g.x * scale : 0.f; r.y = o.y > 0.f ? g.y * scale : 0.f;
      r.z = o.z > 0.f ? g.z * scale : 0.f; r.w = o.w > 0.f ? g.w * scale : 0.f;
      store4<false>(din, row * din_stride + col, r);
    } else {
      const float g = bf2f(dout[row * d_stride + col]);
      din[row * din_stride + col] = f2bf(bf2f(out[row * out_stride + col]) > 0.f ? g * scale : 0.f);
    }
  }
}

// What this launcher does differently from gcn.hip's launch_gcn_spmm, on purpose:
//   * nnz == 0 launches ONE idle chunk of k_spmm (GCN launches no main kernel);
//   * a device-side count is taken as it is, the caller keeps it >= 0 (GCN clamps a negative one to 0);
//   * `part` is required only when nnz > EC (GCN: whenever nnz > 0);
//   * the fix-up takes its VEC4 from vec4 AND the alignment of `part` (fv), the walk from vec4 alone (GCN folds the alignment
//     of `part` into the one vec4 of both kernels);
//   * n_rows <= 0 or dim <= 0 returns before anything is looked at.
template <bool BWD>
int launch_spmm(const int* row_ptr, const int* t_edge, const int* src, const int* dst, const int* blk_indptr, const void* w,
                const void* h, int64_t h_stride, int n_rows, const int* nnz_dev, int nnz, int dim, int mean, void* out,
                int64_t out_stride, int out_fp32, float* part, hipStream_t st) {
  if (n_rows <= 0 || dim <= 0) return 0;
  const int EC = spmm_chunk_edges(nnz);
  if (nnz > EC && !part) return BLISS_EINVAL;               // partials only when a row can be cut: more than one chunk
  const bool vec4 = (dim % 4 == 0) && (h_stride % 4 == 0) && (out_stride % 4 == 0) &&
                    (((uintptr_t)h) % 8 == 0) && (((uintptr_t)out) % (out_fp32 ? 16 : 8) == 0);
  const int nchunks = nnz > 0 ? (nnz + EC - 1) / EC : 1;
  dim3 grid((nchunks + SP_TPB / 64 - 1) / (SP_TPB / 64)), block(SP_TPB), gfix((n_rows + SP_TPB / 64 - 1) / (SP_TPB / 64));
#define GO(V, F) PROF_LAUNCH(BWD ? BK_SPMM_BWD : BK_SPMM_FWD, st, k_spmm<V, F, BWD><<<grid, block, 0, st>>>(row_ptr, t_edge, src, dst, blk_indptr, (const bf16_t*)w, (const bf16_t*)h, h_stride, n_rows, nnz_dev, nnz, dim, mean, out, out_stride, part, EC))
  if (vec4) { if (out_fp32) GO(true, true); else GO(true, false); }
  else      { if (out_fp32) GO(false, true); else GO(false, false); }
#undef GO
  {
    const bool fv = vec4 && (((uintptr_t)part) % 16 == 0);
#define FIX(F, V) PROF_LAUNCH(BK_SPMM_FIXUP, st, k_spmm_fixup<F, BWD, V><<<gfix, block, 0, st>>>(row_ptr, n_rows, dim, mean, part, out, out_stride, EC))
    if (out_fp32) { if (fv) FIX(true, true); else FIX(true, false); }
    else          { if (fv) FIX(false, true); else FIX(false, false); }
#undef FIX
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int bliss_spmm_chunk_edges(int32_t nnz_bound) { return spmm_chunk_edges(nnz_bound); }

int bliss_spmm_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const void* h,
                   int64_t h_stride, int32_t n_dst, const int32_t* nnz_dev, int32_t nnz, int32_t dim, int mean, void* out,
                   int64_t out_stride, int out_fp32, float* partials, void* stream) {
  if (!indptr || !h || !out || nnz < 0 || (nnz > 0 && (!src || !dst))) return BLISS_EINVAL;
  return launch_spmm<false>(indptr, nullptr, src, dst, nullptr, w, h, h_stride, n_dst, nnz_dev, nnz, dim, mean, out, out_stride, out_fp32,
                            partials, (hipStream_t)stream);
}

int bliss_spmm_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst,
                   const int32_t* indptr, const void* w, const void* gout, int64_t gout_stride, int32_t n_src,
                   const int32_t* nnz_dev, int32_t nnz, int32_t dim, int mean, void* gh, int64_t gh_stride, int out_fp32,
                   float* partials, void* stream) {
  if (!t_indptr || !indptr || !gout || !gh || nnz < 0 || (nnz > 0 && (!t_edge || !src || !dst))) return BLISS_EINVAL;
  return launch_spmm<true>(t_indptr, t_edge, src, dst, indptr, w, gout, gout_stride, n_src, nnz_dev, nnz, dim, mean, gh, gh_stride,
                           out_fp32, partials, (hipStream_t)stream);
}

int bliss_sage_epilogue_fwd(const void* a, int64_t a_stride, const void* b, int64_t b_stride, int32_t n_rows, int32_t dim,
                            float p_drop, uint32_t seed, uint64_t* ctr, void* out, int64_t out_stride, void* norm_out, void* stream) {
  if (!a || !b || !out || n_rows < 0 || dim <= 0 || !(p_drop >= 0.f && p_drop < 1.f) || (p_drop > 0.f && !ctr)) return BLISS_EINVAL;   // (NaN too)
  if (n_rows == 0) return 0;
  const bool v4 = dim % 4 == 0 && a_stride % 4 == 0 && b_stride % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)a) % 8 == 0 &&
                  ((uintptr_t)b) % 8 == 0 && ((uintptr_t)out) % 8 == 0;
  const uint32_t thresh = p_drop > 0.f ? (uint32_t)((double)p_drop * 4294967296.0) : 0u;
  const float scale = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  hipStream_t st = (hipStream_t)stream;
  const int grid = (n_rows + SP_TPB / 64 - 1) / (SP_TPB / 64);
  const bool n4 = dim % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)out) % 8 == 0;                  // = bliss_embed_norm(out)
#define GO(V, N) k_sage_epilogue<V, N><<<grid, SP_TPB, 0, st>>>((const bf16_t*)a, a_stride, (const bf16_t*)b, b_stride, n_rows, dim, thresh, scale, \
                                                              seed, (unsigned long long*)ctr, (bf16_t*)out, out_stride, (bf16_t*)norm_out)
  if (v4) GO(true, true); else if (n4) GO(false, true); else GO(false, false);
#undef GO
  return (int)hipGetLastError();
}

int bliss_sage_epilogue_bwd(const void* dout, int64_t dout_stride, const void* out, int64_t out_stride, int32_t n_rows, int32_t dim,
                            float p_drop, void* din, int64_t din_stride, void* stream) {
  if (!dout || !out || !din || n_rows < 0 || dim <= 0 || !(p_drop >= 0.f && p_drop < 1.f)) return BLISS_EINVAL;
  if (n_rows == 0) return 0;
  const bool v4 = dim % 4 == 0 && dout_stride % 4 == 0 && out_stride % 4 == 0 && din_stride % 4 == 0 && ((uintptr_t)dout) % 8 == 0 &&
                  ((uintptr_t)out) % 8 == 0 && ((uintptr_t)din) % 8 == 0;
  const float scale = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
  hipStream_t st = (hipStream_t)stream;
  const int grid = (n_rows + SP_TPB / 64 - 1) / (SP_TPB / 64);
  if (v4) k_sage_epilogue_bwd<true><<<grid, SP_TPB, 0, st>>>((const bf16_t*)dout, dout_stride, (const bf16_t*)out, out_stride, n_rows, dim, scale,
                                                            (bf16_t*)din, din_stride);
  else k_sage_epilogue_bwd<false><<<grid, SP_TPB, 0, st>>>((const bf16_t*)dout, dout_stride, (const bf16_t*)out, out_stride, n_rows, dim, scale,
                                                          (bf16_t*)din, din_stride);
  return (int)hipGetLastError();
}

int bliss_gather_rows(const void* feat, int64_t feat_stride, const int32_t* ids, int32_t n_rows, int32_t dim, void* out,
                      int64_t out_stride, void* norm_out, void* stream) {
  if (!feat || !ids || !out || dim <= 0 || feat_stride < dim || out_stride < dim) return BLISS_EINVAL;
  if (n_rows <= 0) return 0;
  const size_t lds = (size_t)(SP_TPB / 64) * ((dim + 7) & ~7) * sizeof(bf16_t);
  if (lds > 48 * 1024) return BLISS_EINVAL;           // (caller gathers and norms separately)
  hipStream_t st = (hipStream_t)stream;
  const int grid = (n_rows + SP_TPB / 64 - 1) / (SP_TPB / 64);
  const uintptr_t al = (uintptr_t)feat | (uintptr_t)out;
  const int norm_vec4 = (dim % 4 == 0) && (out_stride % 4 == 0) && (((uintptr_t)out) % 8 == 0);     // = bliss_embed_norm(out)
  if (dim % 4 == 0 && feat_stride % 4 == 0 && out_stride % 4 == 0 && al % 8 == 0)
    k_gather_rows_norm<4><<<grid, SP_TPB, lds, st>>>((const bf16_t*)feat, feat_stride, ids, n_rows, dim, (bf16_t*)out, out_stride, (bf16_t*)norm_out, norm_vec4);
  else if (dim % 2 == 0 && feat_stride % 2 == 0 && out_stride % 2 == 0 && al % 4 == 0)
    k_gather_rows_norm<2><<<grid, SP_TPB, lds, st>>>((const bf16_t*)feat, feat_stride, ids, n_rows, dim, (bf16_t*)out, out_stride, (bf16_t*)norm_out, norm_vec4);
  else
    k_gather_rows_norm<1><<<grid, SP_TPB, lds, st>>>((const bf16_t*)feat, feat_stride, ids, n_rows, dim, (bf16_t*)out, out_stride, (bf16_t*)norm_out, norm_vec4);
  return (int)hipGetLastError();
}

int bliss_embed_norm(const void* h, int32_t n_rows, int32_t dim, int64_t row_stride, void* out, void* stream) {
  if (!h || !out) return BLISS_EINVAL;
  if (n_rows <= 0) return 0;
  const int vec4 = (dim % 4 == 0) && (row_stride % 4 == 0) && (((uintptr_t)h) % 8 == 0);
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH(BK_EMBED_NORM, st, k_embed_norm<<<(n_rows + 3) / 4, SP_TPB, 0, st>>>((const bf16_t*)h, n_rows, dim, row_stride, (bf16_t*)out, vec4));
  return (int)hipGetLastError();
}

}  // extern "C"
