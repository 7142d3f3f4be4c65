// Self-inclusive normalised-sum message passing for SAGEConv('gcn') with sampled edge weights, gfx950.
//
// Replaces DGL's  graph.update_all(fn.u_mul_e('h', '_edge_weight', 'm'), fn.sum('m', 'neigh'));
// h_neigh = (neigh + h_dst) / (in_degrees + 1)  [DGL-recalled] and its autograd backward with ONE rounding per direction:
//   out[i, :] = bf16( (sum_{e in row i} float(w_e) * float(h[src_e, :])  +  float(h_self[i, :])) * (1.0f / (float)(deg_i + 1)) )
//   gh[j, :]  = bf16( sum_{e : src_e = j} (float(w_e) / (float)(deg_{dst_e} + 1)) * float(g[dst_e, :])
//                     +  (j < live n_dst ? (1.0f / (float)(deg_j + 1)) * float(g[j, :]) : 0) )
// deg_i = the block's in-degree (edges with multiplicity, not a sum of weights).  The messages are summed in fp32 in the
// balanced walk's fixed order (by edge inside a chunk, chunk partials in chunk order); the self term is added LAST, in fp32,
// where a finished row is rounded and stored -- never to the fp32 chunk partials.  A live destination without in-edges gets its
// self row bit for bit; rows at or past the live destination count get +0 without their self row being read.
//
// Both directions keep the balanced chunk decomposition of spmm_walk.cuh (a wave owns spmm_chunk_edges(nnz) consecutive
// entries of the edge list, a lane 4 bf16 columns, the (neighbour, coefficient) pairs fetched coalesced and broadcast by
// v_readlane, 4 row loads in flight) and bring their own walk and fix-up, as spmm_max.hip does: the shared walk's policy has a
// per-edge coefficient and a per-row scale but no self term, and its fix-up clears a row without edges.  The self row of a row
// is read where the row BEGINS in a chunk (its address needs the row id alone), so it travels with the row's first edge loads.
// The backward is a gather through the by-source index: no float atomics, bitwise reproducible.
//
// Partials: slot (chunk ci, head 0 | tail 1) = floats [(ci * 2 + t) * dim, + dim), as for bliss_spmm_fwd.
#include "common.cuh"
#include "spmm_walk.cuh"
#include "bliss_gnn.h"
#include "prof.h"

namespace {

using spmm_walk::bcast_f;
using spmm_walk::bcast_i;
using spmm_walk::f4;
using spmm_walk::load4;
using spmm_walk::spmm_chunk_edges;
using spmm_walk::store4;

#define SS_TPB 256

// One description for the four kernels.  Forward: row_ptr = indptr (rows = destinations), h = the features, hs = h_self.
// Backward: row_ptr = t_indptr (rows = sources), h = hs = gout, indptr = the block's CSR by destination (the degrees).
struct SelfArgs {
  const int* row_ptr; const int* t_edge; const int* src; const int* dst; const int* indptr;
  const bf16_t* w;
  const bf16_t* h; int64_t h_stride;
  const bf16_t* hs; int64_t hs_stride;
  int n_rows;                                               // rows of `out`: n_dst (forward), n_src (backward)
  int n_dst; const int* n_dst_dev;                          // the destination bound and the live count on the device (or NULL)
  const int* nnz_dev; int nnz;
  int dim;
  bf16_t* out; int64_t out_stride;
  float* part;
  int EC;
};

// min(*dev, host) clamped at 0; host alone without a device-side count
__device__ __forceinline__ int live_count(const int* dev, int host) {
  int n = host;
  if (dev) { const int t = *dev; n = t < n ? t : n; }
  return n < 0 ? 0 : n;
}

// 1 / (deg_r + 1) of destination r, deg from the block's indptr below the live edge count
__device__ __forceinline__ float inv_deg1(const int* __restrict__ indptr, int r, int nnz) {
  const int d = min(indptr[r + 1], nnz) - indptr[r];
  return 1.0f / (float)((d > 0 ? d : 0) + 1);
}

template <bool VEC4>
__device__ __forceinline__ f4 row_at(const bf16_t* p, int64_t off) {
  if (VEC4) return load4(p + off);
  return f4{bf2f(p[off]), 0.f, 0.f, 0.f};
}

template <bool VEC4>
__device__ __forceinline__ void put_row(bf16_t* out, int64_t off, f4 a) {
  if (VEC4) store4<false>(out, off, a);
  else out[off] = f2bf(a.x);
}

__device__ __forceinline__ f4 mul4(f4 a, float k) { return f4{a.x * k, a.y * k, a.z * k, a.w * k}; }
__device__ __forceinline__ f4 add4(f4 a, f4 b) { return f4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// ---- the walk, both directions ----------------------------------------------------------------------------------------------
// FWD (BWD = false): row = dst[e], neighbour = src[e], coefficient = w[e]; a finished row: (acc + h_self[row]) * 1/(deg + 1).
// BWD:               row = src[e], neighbour = dst[e], coefficient = w[e] / (deg_dst + 1); a finished row: acc + the self term
//                    inv_row * g[row] if row is a live destination.
template <bool VEC4, bool BWD>
__device__ __forceinline__ void walk(const SelfArgs& p) {
  const int nnz = live_count(p.nnz_dev, p.nnz);
  const int EC = p.EC, dim = p.dim;
  const int ci = blockIdx.x * (SS_TPB / 64) + (threadIdx.x >> 6);
  if ((int64_t)ci * EC >= nnz) return;                      // (rows without edges are written by the fix-up)
  const int live = BWD ? live_count(p.n_dst_dev, p.n_dst) : 0;
  const int lane = lane_id();
  const int c0 = ci * EC, c1 = min(nnz, c0 + EC), cnt = c1 - c0;
  int my_row = -1, my_n = 0;
  float my_c = 0.f;
  if (lane < cnt) {
    const int e = BWD ? p.t_edge[c0 + lane] : c0 + lane;
    const int s = p.src[e], d = p.dst[e];
    my_row = BWD ? s : d;
    my_n = BWD ? d : s;
    my_c = p.w ? bf2f(p.w[e]) : 1.0f;
    if (BWD) {
      const int dg = min(p.indptr[d + 1], nnz) - p.indptr[d];
      my_c = my_c / (float)((dg > 0 ? dg : 0) + 1);
    }
  }
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int col0 = 0; col0 < dim; col0 += 64 * W) {
    const int col = col0 + lane * W;
    const bool act = col < dim;
    // the self term of row r (r has a live edge in this chunk: a live row, in bounds)
    auto self_of = [&](int r) {
      f4 a = zero;
      if (!act) return a;
      if (BWD) {
        if (r < live) a = mul4(row_at<VEC4>(p.hs, r * p.hs_stride + col), inv_deg1(p.indptr, r, nnz));
      } else {
        a = row_at<VEC4>(p.hs, r * p.hs_stride + col);
      }
      return a;
    };
    // finish row r: the self term last, one rounding at the store; or leave an fp32 partial (no self term) for the fix-up
    auto flush = [&](int r, f4 acc, f4 sv) {
      const int rb = p.row_ptr[r], re = min(p.row_ptr[r + 1], nnz);
      const bool starts = rb >= c0, ends = re <= c1;
      if (!act) return;
      if (starts && ends) {
        acc = add4(acc, sv);
        if (!BWD) acc = mul4(acc, 1.0f / (float)(re - rb + 1));
        put_row<VEC4>(p.out, r * p.out_stride + col, acc);
      } else {
        float* q = p.part + ((int64_t)ci * 2 + (starts ? 1 : 0)) * dim + col;
        if (VEC4) *reinterpret_cast<float4*>(q) = make_float4(acc.x, acc.y, acc.z, acc.w);
        else q[0] = acc.x;
      }
    };
    int cur = bcast_i(my_row, 0);
    f4 acc = zero, sv = self_of(cur);
    for (int j = 0; j < cnt;) {
      const int r = bcast_i(my_row, j);
      if (r != cur) { flush(cur, acc, sv); acc = zero; cur = r; sv = self_of(r); }
      const int run = __popcll(__ballot(my_row == r && lane >= j));
      const int end = j + run;
      for (; j + 4 <= end; j += 4) {
        const int n0 = bcast_i(my_n, j), n1 = bcast_i(my_n, j + 1), n2 = bcast_i(my_n, j + 2), n3 = bcast_i(my_n, j + 3);
        const float k0 = bcast_f(my_c, j), k1 = bcast_f(my_c, j + 1), k2 = bcast_f(my_c, j + 2), k3 = bcast_f(my_c, j + 3);
        if (act) {
          if (VEC4) {
            const f4 a0 = load4(p.h + n0 * p.h_stride + col), a1 = load4(p.h + n1 * p.h_stride + col);
            const f4 a2 = load4(p.h + n2 * p.h_stride + col), a3 = load4(p.h + n3 * p.h_stride + col);
            acc.x += k0 * a0.x; acc.y += k0 * a0.y; acc.z += k0 * a0.z; acc.w += k0 * a0.w;
            acc.x += k1 * a1.x; acc.y += k1 * a1.y; acc.z += k1 * a1.z; acc.w += k1 * a1.w;
            acc.x += k2 * a2.x; acc.y += k2 * a2.y; acc.z += k2 * a2.z; acc.w += k2 * a2.w;
            acc.x += k3 * a3.x; acc.y += k3 * a3.y; acc.z += k3 * a3.z; acc.w += k3 * a3.w;
          } else {
            const float a0 = bf2f(p.h[n0 * p.h_stride + col]), a1 = bf2f(p.h[n1 * p.h_stride + col]);
            const float a2 = bf2f(p.h[n2 * p.h_stride + col]), a3 = bf2f(p.h[n3 * p.h_stride + col]);
            acc.x += k0 * a0; acc.x += k1 * a1; acc.x += k2 * a2; acc.x += k3 * a3;
          }
        }
      }
      for (; j < end; ++j) {
        const int n0 = bcast_i(my_n, j);
        const float k0 = bcast_f(my_c, j);
        if (act) {
          if (VEC4) {
            const f4 a0 = load4(p.h + n0 * p.h_stride + col);
            acc.x += k0 * a0.x; acc.y += k0 * a0.y; acc.z += k0 * a0.z; acc.w += k0 * a0.w;
          } else acc.x += k0 * bf2f(p.h[n0 * p.h_stride + col]);
        }
      }
    }
    flush(cur, acc, sv);
  }
}

// ---- the fix-up, both directions: one wave per row -----------------------------------------------------------------------------
// A row cut by chunk boundaries: the tail partial of the chunk it starts in, then the head partials of the following chunks in
// chunk order, then the self term, one rounding.  A row without live edges: FWD its self row, bit for bit (+0 at or past the live
// destination count, the self row unread); BWD the self term alone for a live destination, else +0.
template <bool VEC4, bool BWD>
__device__ __forceinline__ void fix(const SelfArgs& p) {
  const int r = blockIdx.x * (SS_TPB / 64) + (threadIdx.x >> 6);
  if (r >= p.n_rows) return;
  const int nnz = live_count(p.nnz_dev, p.nnz);
  const int live = live_count(p.n_dst_dev, p.n_dst);
  const int lane = lane_id(), dim = p.dim, EC = p.EC;
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  bf16_t* po = p.out + r * p.out_stride;
  if (!BWD && r >= live) {                                  // capacity padding: +0, nothing read
    for (int col = lane * W; col < dim; col += 64 * W) put_row<VEC4>(po, col, zero);
    return;
  }
  const int rb = p.row_ptr[r], re = min(p.row_ptr[r + 1], nnz);
  const bool has_self = !BWD || r < live;
  const bf16_t* ps = p.hs + r * p.hs_stride;                // (formed only; read under has_self)
  if (re <= rb) {
    if (!BWD) {                                             // the self row's own bits: (0 + x) * 1.0f rounds to x, copied instead
      for (int col = lane * W; col < dim; col += 64 * W) {
        if (VEC4) *reinterpret_cast<uint2*>(po + col) = *reinterpret_cast<const uint2*>(ps + col);
        else po[col] = ps[col];
      }
    } else {
      const float inv = has_self ? inv_deg1(p.indptr, r, nnz) : 0.f;
      for (int col = lane * W; col < dim; col += 64 * W)
        put_row<VEC4>(po, col, has_self ? mul4(row_at<VEC4>(ps, col), inv) : zero);
    }
    return;
  }
  const int c = rb / EC, c_end = (re - 1) / EC;
  if (c_end == c) return;                                   // finished by its chunk
  const float inv = BWD ? (has_self ? inv_deg1(p.indptr, r, nnz) : 0.f) : 1.0f / (float)(re - rb + 1);
  for (int col = lane * W; col < dim; col += 64 * W) {
    const f4 sv = has_self ? row_at<VEC4>(ps, col) : zero;  // (issued in front of the partials' loads, used behind them)
    f4 sum = zero;
    if (VEC4) {
      const float4 v = *reinterpret_cast<const float4*>(p.part + ((int64_t)c * 2 + 1) * dim + col);
      sum = f4{v.x, v.y, v.z, v.w};
#pragma unroll 4
      for (int cc = c + 1; cc <= c_end; ++cc) {
        const float4 u = *reinterpret_cast<const float4*>(p.part + ((int64_t)cc * 2) * dim + col);
        sum.x += u.x; sum.y += u.y; sum.z += u.z; sum.w += u.w;
      }
    } else {
      sum.x = p.part[((int64_t)c * 2 + 1) * dim + col];
      for (int cc = c + 1; cc <= c_end; ++cc) sum.x += p.part[((int64_t)cc * 2) * dim + col];
    }
    if (BWD) sum = add4(sum, mul4(sv, inv));
    else sum = mul4(add4(sum, sv), inv);
    put_row<VEC4>(po, col, sum);
  }
}

template <bool VEC4> __global__ void __launch_bounds__(SS_TPB) k_spmm_self(SelfArgs p) { walk<VEC4, false>(p); }
template <bool VEC4> __global__ void __launch_bounds__(SS_TPB) k_spmm_self_fixup(SelfArgs p) { fix<VEC4, false>(p); }
template <bool VEC4> __global__ void __launch_bounds__(SS_TPB) k_spmm_self_bwd(SelfArgs p) { walk<VEC4, true>(p); }
template <bool VEC4> __global__ void __launch_bounds__(SS_TPB) k_spmm_self_bwd_fixup(SelfArgs p) { fix<VEC4, true>(p); }

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p) % a == 0; }

template <bool BWD>
int launch_self(SelfArgs p, hipStream_t st) {
  if (p.n_rows == 0) return 0;
  const int EC = p.EC;
  const bool vec4 = p.dim % 4 == 0 && p.h_stride % 4 == 0 && p.hs_stride % 4 == 0 && p.out_stride % 4 == 0 && al(p.h, 8) && al(p.hs, 8) &&
                    al(p.out, 8) && al(p.part, 16);
  const int nchunks = (p.nnz + EC - 1) / EC;
  const dim3 block(SS_TPB), grid((nchunks + SS_TPB / 64 - 1) / (SS_TPB / 64)), gfix((p.n_rows + SS_TPB / 64 - 1) / (SS_TPB / 64));
  if (nchunks > 0) {
    if (BWD) {
      if (vec4) PROF_LAUNCH(BK_SPMM_SELF_BWD, st, k_spmm_self_bwd<true><<<grid, block, 0, st>>>(p));
      else PROF_LAUNCH(BK_SPMM_SELF_BWD, st, k_spmm_self_bwd<false><<<grid, block, 0, st>>>(p));
    } else {
      if (vec4) PROF_LAUNCH(BK_SPMM_SELF_FWD, st, k_spmm_self<true><<<grid, block, 0, st>>>(p));
      else PROF_LAUNCH(BK_SPMM_SELF_FWD, st, k_spmm_self<false><<<grid, block, 0, st>>>(p));
    }
  }
  if (BWD) {
    if (vec4) PROF_LAUNCH(BK_SPMM_SELF_BWD_FIXUP, st, k_spmm_self_bwd_fixup<true><<<gfix, block, 0, st>>>(p));
    else PROF_LAUNCH(BK_SPMM_SELF_BWD_FIXUP, st, k_spmm_self_bwd_fixup<false><<<gfix, block, 0, st>>>(p));
  } else {
    if (vec4) PROF_LAUNCH(BK_SPMM_SELF_FIXUP, st, k_spmm_self_fixup<true><<<gfix, block, 0, st>>>(p));
    else PROF_LAUNCH(BK_SPMM_SELF_FIXUP, st, k_spmm_self_fixup<false><<<gfix, block, 0, st>>>(p));
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int bliss_spmm_self_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const void* h, int64_t h_stride,
                        const void* h_self, int64_t h_self_stride, int32_t n_dst, const int32_t* n_dst_dev, const int32_t* nnz_dev,
                        int32_t nnz, int32_t dim, void* out, int64_t out_stride, float* partials, void* stream) {
  if (!indptr || !h || !h_self || !out || n_dst < 0 || nnz < 0 || dim <= 0 || (nnz > 0 && (!src || !dst))) return BLISS_EINVAL;
  if (h_stride < dim || h_self_stride < dim || out_stride < dim) return BLISS_EINVAL;
  const int EC = spmm_chunk_edges(nnz);
  if (nnz > EC && !partials) return BLISS_EINVAL;           // partials only when a row can be cut: more than one chunk
  SelfArgs p = {indptr, nullptr, src, dst, indptr, (const bf16_t*)w, (const bf16_t*)h, h_stride, (const bf16_t*)h_self, h_self_stride,
                n_dst, n_dst, n_dst_dev, nnz_dev, nnz, dim, (bf16_t*)out, out_stride, partials, EC};
  return launch_self<false>(p, (hipStream_t)stream);
}

int bliss_spmm_self_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const int32_t* indptr,
                        const void* w, const void* gout, int64_t gout_stride, int32_t n_src, int32_t n_dst, const int32_t* n_dst_dev,
                        const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, float* partials, void* stream) {
  if (!t_indptr || !indptr || !gout || !gh || n_src < 0 || n_dst < 0 || nnz < 0 || dim <= 0 || (nnz > 0 && (!t_edge || !src || !dst)))
    return BLISS_EINVAL;
  if (gout_stride < dim || gh_stride < dim) return BLISS_EINVAL;
  if (n_dst > n_src) return BLISS_EINVAL;                   // the self term lands on the leading source rows
  const int EC = spmm_chunk_edges(nnz);
  if (nnz > EC && !partials) return BLISS_EINVAL;
  SelfArgs p = {t_indptr, t_edge, src, dst, indptr, (const bf16_t*)w, (const bf16_t*)gout, gout_stride, (const bf16_t*)gout, gout_stride,
                n_src, n_dst, n_dst_dev, nnz_dev, nnz, dim, (bf16_t*)gh, gh_stride, partials, EC};
  return launch_self<true>(p, (hipStream_t)stream);
}

}  // extern "C"
