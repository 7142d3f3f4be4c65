// The balanced SpMM traversal of the message-passing kernels, gfx950: the one copy of the row primitives, the chunk walk, the
// chunk-order fix-up and the chunk-length rule.  spmm.hip (SAGEConv) and gcn.hip (GraphConv) wrap the
// walk and the fix-up in their kernels and differ only in a policy object; gcn_infer.hip and gat.hip take the row primitives
// (and gcn_infer.hip the chunk rule, whose fp32 sum order it reproduces per row).
//
// HBM-bound gather: a 64-lane wave owns EC consecutive edges; a lane owns 4 consecutive bf16 features (8-byte loads, 512 B per
// wave-instruction for a 256-wide row); the (neighbour, coefficient) pairs are fetched coalesced and broadcast by lane; 4
// neighbour rows are kept in flight.  fp32 accumulation, one rounding at the store.
//
// Policy contract (a small object passed by value, everything in it wave-uniform or read-only):
//   float coef(float w, int s, int d)    the coefficient of edge s -> d whose weight is w (1.0f without weights): ONE value per
//                                        edge, computed by the lane that fetched the edge
//   float scale(int r, int rb, int re)   the factor row r (edges [rb, re) of row_ptr) is multiplied by at its store; evaluated
//                                        only where a row is stored, never for a partial
#pragma once
#include "common.cuh"

namespace spmm_walk {

struct f4 { float x, y, z, w; };

// broadcast from a lane whose index is wave-uniform: v_readlane (scalar result, no LDS round trip like __shfl's ds_bpermute)
__device__ __forceinline__ int bcast_i(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float bcast_f(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

__device__ __forceinline__ f4 load4(const bf16_t* p) {
  uint2 v = *reinterpret_cast<const uint2*>(p);
  f4 r;
  r.x = __uint_as_float(v.x << 16); r.y = __uint_as_float(v.x & 0xffff0000u);
  r.z = __uint_as_float(v.y << 16); r.w = __uint_as_float(v.y & 0xffff0000u);
  return r;
}

template <bool OUT_F32>
__device__ __forceinline__ void store4(void* out, int64_t off, f4 a) {
  if (OUT_F32) {
    *reinterpret_cast<float4*>((float*)out + off) = make_float4(a.x, a.y, a.z, a.w);
  } else {
    uint2 v;
    v.x = (uint32_t)f2bf(a.x) | ((uint32_t)f2bf(a.y) << 16);
    v.y = (uint32_t)f2bf(a.z) | ((uint32_t)f2bf(a.w) << 16);
    *reinterpret_cast<uint2*>((bf16_t*)out + off) = v;
  }
}

template <bool VEC4, bool OUT_F32>
__device__ __forceinline__ void store_row(void* out, int64_t off, f4 a, float scale) {
  a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
  if (VEC4) store4<OUT_F32>(out, off, a);
  else if (OUT_F32) ((float*)out)[off] = a.x;
  else ((bf16_t*)out)[off] = f2bf(a.x);
}

// A wave walks its chunk edge by edge (a dependent chain of broadcasts and row loads), so the chunk length trades
// parallelism against per-chunk overhead: the sampled blocks of this path hold 2 K - 500 K edges, far too few for
// 64-edge chunks to fill the chip: 64 edges per wave from 200 K edges up, 32 from 50 K, 16 below.
__host__ __device__ inline int spmm_chunk_edges(int nnz) { return nnz >= 200000 ? 64 : (nnz >= 50000 ? 32 : 16); }

// Balanced ("merge-style") traversal: a wave owns EC consecutive entries of the edge list (spmm_chunk_edges), whatever
// rows they belong to, so a 30 000-edge hub row and a 3-edge row cost the same per wave.  Rows that lie
// inside one chunk are finished and stored by that wave; a row cut by chunk boundaries leaves fp32
// partials (one "head" and one "tail" slot per chunk) that fixup() adds IN CHUNK ORDER -- the sum
// order is fixed, so results are bitwise reproducible without float atomics.
// FWD: row = destination (CSR row), neighbour = src[e]
// BWD: row = source (t_edge groups the edges by source), neighbour = dst[e]
// Chunk `ci` of the nnz live edges (the caller has checked ci against the chunk count); nothing at or past nnz is read.
template <bool VEC4, bool OUT_F32, bool BWD, class Policy>
__device__ __forceinline__ void chunk(const Policy pol, int ci, int nnz, int EC, const int* __restrict__ row_ptr,
                                      const int* __restrict__ t_edge, const int* __restrict__ src, const int* __restrict__ dst,
                                      const bf16_t* __restrict__ w, const bf16_t* __restrict__ h, int64_t h_stride, int dim,
                                      void* out, int64_t out_stride, float* __restrict__ part) {
  const int lane = lane_id();
  const int c0 = ci * EC, c1 = min(nnz, c0 + EC), cnt = c1 - c0;
  int my_row = -1, my_n = 0;
  float my_c = 0.f;
  if (lane < cnt) {
    const int e = BWD ? t_edge[c0 + lane] : c0 + lane;
    const int s = src[e], d = dst[e];
    my_row = BWD ? s : d;
    my_n = BWD ? d : s;
    my_c = pol.coef(w ? bf2f(w[e]) : 1.0f, s, d);
  }
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int col0 = 0; col0 < dim; col0 += 64 * W) {
    const int col = col0 + lane * W;
    const bool act = col < dim;
    // finish row r with the accumulated value: store, or leave a partial for the fix-up pass
    auto flush = [&](int r, f4 acc) {
      const int rb = row_ptr[r], re = row_ptr[r + 1];
      const bool starts = rb >= c0, ends = re <= c1;
      if (!act) return;
      if (starts && ends) {
        store_row<VEC4, OUT_F32>(out, r * out_stride + col, acc, pol.scale(r, rb, re));
      } else {
        float* q = part + ((int64_t)ci * 2 + (starts ? 1 : 0)) * dim + col;
        q[0] = acc.x;
        if (VEC4) { q[1] = acc.y; q[2] = acc.z; q[3] = acc.w; }
      }
    };
    if (cnt == 0) continue;                                 // rows without edges are cleared by fixup()
    int cur = bcast_i(my_row, 0);
    f4 acc = zero;
    for (int j = 0; j < cnt;) {
      const int r = bcast_i(my_row, j);
      if (r != cur) { flush(cur, acc); acc = zero; cur = r; }
      const int run = __popcll(__ballot(my_row == r && lane >= j));
      const int end = j + run;
      for (; j + 4 <= end; j += 4) {
        int n0 = bcast_i(my_n, j), n1 = bcast_i(my_n, j + 1), n2 = bcast_i(my_n, j + 2), n3 = bcast_i(my_n, j + 3);
        float k0 = bcast_f(my_c, j), k1 = bcast_f(my_c, j + 1), k2 = bcast_f(my_c, j + 2), k3 = bcast_f(my_c, j + 3);
        if (act) {
          if (VEC4) {
            f4 a0 = load4(h + n0 * h_stride + col), a1 = load4(h + n1 * h_stride + col);
            f4 a2 = load4(h + n2 * h_stride + col), a3 = load4(h + n3 * h_stride + col);
            acc.x += k0 * a0.x; acc.y += k0 * a0.y; acc.z += k0 * a0.z; acc.w += k0 * a0.w;
            acc.x += k1 * a1.x; acc.y += k1 * a1.y; acc.z += k1 * a1.z; acc.w += k1 * a1.w;
            acc.x += k2 * a2.x; acc.y += k2 * a2.y; acc.z += k2 * a2.z; acc.w += k2 * a2.w;
            acc.x += k3 * a3.x; acc.y += k3 * a3.y; acc.z += k3 * a3.z; acc.w += k3 * a3.w;
          } else {
            float a0 = bf2f(h[n0 * h_stride + col]), a1 = bf2f(h[n1 * h_stride + col]);
            float a2 = bf2f(h[n2 * h_stride + col]), a3 = bf2f(h[n3 * h_stride + col]);
            acc.x += k0 * a0; acc.x += k1 * a1; acc.x += k2 * a2; acc.x += k3 * a3;
          }
        }
      }
      for (; j < end; ++j) {
        int n0 = bcast_i(my_n, j);
        float k0 = bcast_f(my_c, j);
        if (act) {
          if (VEC4) {
            f4 a0 = load4(h + n0 * h_stride + col);
            acc.x += k0 * a0.x; acc.y += k0 * a0.y; acc.z += k0 * a0.z; acc.w += k0 * a0.w;
          } else acc.x += k0 * bf2f(h[n0 * h_stride + col]);
        }
      }
    }
    flush(cur, acc);
  }
}

// Row r after the walk, one wave per row.  Rows cut by chunk boundaries: the tail partial of the chunk they start in + the head
// partials of the following chunks, in chunk order; rows without edges (isolated or capacity-padded) are cleared here.
template <bool VEC4, bool OUT_F32, class Policy>
__device__ __forceinline__ void fixup(const Policy pol, int r, const int* __restrict__ row_ptr, int dim, const float* __restrict__ part,
                                      void* out, int64_t out_stride, int EC) {
  const int lane = lane_id();
  const int rb = row_ptr[r], re = row_ptr[r + 1];
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  if (re <= rb) {                                           // no edges (incl. capacity-padded rows): the output row is zero
    for (int col = lane * W; col < dim; col += 64 * W) store_row<VEC4, OUT_F32>(out, r * out_stride + col, zero, 1.0f);
    return;
  }
  const int c = rb / EC, c_end = (re - 1) / EC;
  if (c_end == c) return;                                   // finished by its chunk
  const float scale = pol.scale(r, rb, re);
  for (int col = lane * W; col < dim; col += 64 * W) {
    f4 sum = zero;
    if (VEC4) {
      const float4 v = *reinterpret_cast<const float4*>(part + ((int64_t)c * 2 + 1) * dim + col);
      sum.x = v.x; sum.y = v.y; sum.z = v.z; sum.w = v.w;
#pragma unroll 4
      for (int cc = c + 1; cc <= c_end; ++cc) {
        const float4 u = *reinterpret_cast<const float4*>(part + ((int64_t)cc * 2) * dim + col);
        sum.x += u.x; sum.y += u.y; sum.z += u.z; sum.w += u.w;
      }
    } else {
      sum.x = part[((int64_t)c * 2 + 1) * dim + col];
      for (int cc = c + 1; cc <= c_end; ++cc) sum.x += part[((int64_t)cc * 2) * dim + col];
    }
    store_row<VEC4, OUT_F32>(out, r * out_stride + col, sum, scale);
  }
}

}  // namespace spmm_walk
