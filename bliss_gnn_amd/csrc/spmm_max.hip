// Max-reduce message passing for SAGEConv('pool') with sampled edge weights, gfx950.
//
// Replaces DGL's g-SpMM behind  graph.update_all(fn.u_mul_e('h', '_edge_weight', 'm'), fn.max('m', 'neigh'))  [DGL-recalled]
// and its autograd backward:
//   m_e[c]    = bf16(float(w_e) * float(h[src_e, c]))       (one rounding: the product of two bf16 values is exact in fp32)
//   arg[i, c] = the lowest edge e of row i whose m_e[c] is largest (float compare, the running best moves on strict > only)
//   out[i, c] = m_arg[c];  a row without edges: out = 0, arg = -1
//   gh[j, c]  = bf16( sum_{e : src_e = j and arg[dst_e, c] == e} float(w_e) * float(gout[dst_e, c]) )     (fp32 sum)
// and, for a layer whose maximised rows are act = relu(z), the backward with the ReLU's mask folded in:
//   gz[j, c]  = act[j, c] > 0 ? gh[j, c] : +0       (the mask behind the one rounding, never on the fp32 chunk partials)
//
// Both directions keep the balanced chunk decomposition of spmm_walk.cuh (a wave owns spmm_chunk_edges(nnz) consecutive
// entries of the edge list, a lane 4 bf16 columns, the (neighbour, weight) pairs fetched coalesced and broadcast by
// v_readlane, 4 row loads in flight).  A row inside one chunk is finished by its wave; a row cut by chunk boundaries leaves
// a head or a tail partial that the fix-up kernel combines IN CHUNK ORDER -- (value, arg) pairs under the same strict > in the
// forward, so the lowest edge still wins; fp32 sums in the backward, which is a gather through the by-source index: no float
// atomics, bitwise reproducible.
//
// Partials, 32-bit words: forward  slot (chunk ci, head 0 | tail 1) = words [(ci * 2 + t) * 2 * dim, + 2 * dim): dim fp32 values,
// then dim int32 args (the args are neither written nor read when arg == NULL); backward slot = words [(ci * 2 + t) * dim, + dim).
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

#define SM_TPB 256

struct i4 { int x, y, z, w; };

__device__ __forceinline__ i4 load4i(const int* p) {
  const int4 v = *reinterpret_cast<const int4*>(p);
  return i4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void store4i(int* p, i4 a) { *reinterpret_cast<int4*>(p) = make_int4(a.x, a.y, a.z, a.w); }
__device__ __forceinline__ void store4f(float* p, f4 a) { *reinterpret_cast<float4*>(p) = make_float4(a.x, a.y, a.z, a.w); }
__device__ __forceinline__ f4 load4f(const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return f4{v.x, v.y, v.z, v.w};
}

// the message of one column: one rounding with a weight, the feature itself without
template <bool HAS_W>
__device__ __forceinline__ float msg(float k, float a) { return HAS_W ? rbf(k * a) : a; }

// the serial first-wins rule: the first edge of a row always takes the slot (arg < 0), later ones only on strict >
__device__ __forceinline__ void take(float& best, int& arg, float m, int e) {
  const bool t = arg < 0 || m > best;
  best = t ? m : best;
  arg = t ? e : arg;
}

// ---- forward --------------------------------------------------------------------------------------------------------------
template <bool VEC4, bool HAS_W>
__global__ void __launch_bounds__(SM_TPB) k_spmm_max(const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                    const int* __restrict__ dst, const bf16_t* __restrict__ w,
                                                    const bf16_t* __restrict__ h, int64_t h_stride, const int* __restrict__ nnz_dev,
                                                    int nnz_host, int dim, bf16_t* __restrict__ out, int64_t out_stride,
                                                    int* __restrict__ arg, int64_t arg_stride, float* __restrict__ part, int EC) {
  const int nnz = nnz_dev ? max(0, min(*nnz_dev, nnz_host)) : nnz_host;
  const int ci = blockIdx.x * (SM_TPB / 64) + (threadIdx.x >> 6);
  if ((int64_t)ci * EC >= nnz) return;                      // (rows without edges are cleared by the fix-up)
  const int lane = lane_id();
  const int c0 = ci * EC, c1 = min(nnz, c0 + EC), cnt = c1 - c0;
  int my_row = -1, my_n = 0;
  float my_c = 1.0f;
  if (lane < cnt) {
    const int e = c0 + lane;
    my_row = dst[e];
    my_n = src[e];
    if (HAS_W) my_c = bf2f(w[e]);
  }
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  const i4 none = {-1, -1, -1, -1};
  for (int col0 = 0; col0 < dim; col0 += 64 * W) {
    const int col = col0 + lane * W;
    const bool act = col < dim;
    // finish row r: store it, or leave a (value, arg) partial for the fix-up pass
    auto flush = [&](int r, f4 best, i4 ba) {
      const int rb = row_ptr[r], re = min(row_ptr[r + 1], nnz);
      const bool starts = rb >= c0, ends = re <= c1;
      if (!act) return;
      if (starts && ends) {
        if (VEC4) {
          store4<false>(out, r * out_stride + col, best);
          if (arg) store4i(arg + r * arg_stride + col, ba);
        } else {
          out[r * out_stride + col] = f2bf(best.x);
          if (arg) arg[r * arg_stride + col] = ba.x;
        }
      } else {
        float* q = part + ((int64_t)ci * 2 + (starts ? 1 : 0)) * 2 * dim + col;
        if (VEC4) {
          store4f(q, best);
          if (arg) store4i(reinterpret_cast<int*>(q) + dim, ba);
        } else {
          q[0] = best.x;
          if (arg) reinterpret_cast<int*>(q)[dim] = ba.x;
        }
      }
    };
    int cur = bcast_i(my_row, 0);
    f4 best = zero;
    i4 ba = none;
    for (int j = 0; j < cnt;) {
      const int r = bcast_i(my_row, j);
      if (r != cur) { flush(cur, best, ba); best = zero; ba = none; cur = r; }
      const int run = __popcll(__ballot(my_row == r && lane >= j));
      const int end = j + run;
      for (; j + 4 <= end; j += 4) {
        const int n0 = bcast_i(my_n, j), n1 = bcast_i(my_n, j + 1), n2 = bcast_i(my_n, j + 2), n3 = bcast_i(my_n, j + 3);
        const float k0 = bcast_f(my_c, j), k1 = bcast_f(my_c, j + 1), k2 = bcast_f(my_c, j + 2), k3 = bcast_f(my_c, j + 3);
        const int e = c0 + j;
        if (act) {
          if (VEC4) {
            const f4 a0 = load4(h + n0 * h_stride + col), a1 = load4(h + n1 * h_stride + col);
            const f4 a2 = load4(h + n2 * h_stride + col), a3 = load4(h + n3 * h_stride + col);
            take(best.x, ba.x, msg<HAS_W>(k0, a0.x), e); take(best.y, ba.y, msg<HAS_W>(k0, a0.y), e);
            take(best.z, ba.z, msg<HAS_W>(k0, a0.z), e); take(best.w, ba.w, msg<HAS_W>(k0, a0.w), e);
            take(best.x, ba.x, msg<HAS_W>(k1, a1.x), e + 1); take(best.y, ba.y, msg<HAS_W>(k1, a1.y), e + 1);
            take(best.z, ba.z, msg<HAS_W>(k1, a1.z), e + 1); take(best.w, ba.w, msg<HAS_W>(k1, a1.w), e + 1);
            take(best.x, ba.x, msg<HAS_W>(k2, a2.x), e + 2); take(best.y, ba.y, msg<HAS_W>(k2, a2.y), e + 2);
            take(best.z, ba.z, msg<HAS_W>(k2, a2.z), e + 2); take(best.w, ba.w, msg<HAS_W>(k2, a2.w), e + 2);
            take(best.x, ba.x, msg<HAS_W>(k3, a3.x), e + 3); take(best.y, ba.y, msg<HAS_W>(k3, a3.y), e + 3);
            take(best.z, ba.z, msg<HAS_W>(k3, a3.z), e + 3); take(best.w, ba.w, msg<HAS_W>(k3, a3.w), e + 3);
          } else {
            const float a0 = bf2f(h[n0 * h_stride + col]), a1 = bf2f(h[n1 * h_stride + col]);
            const float a2 = bf2f(h[n2 * h_stride + col]), a3 = bf2f(h[n3 * h_stride + col]);
            take(best.x, ba.x, msg<HAS_W>(k0, a0), e); take(best.x, ba.x, msg<HAS_W>(k1, a1), e + 1);
            take(best.x, ba.x, msg<HAS_W>(k2, a2), e + 2); take(best.x, ba.x, msg<HAS_W>(k3, a3), e + 3);
          }
        }
      }
      for (; j < end; ++j) {
        const int n0 = bcast_i(my_n, j);
        const float k0 = bcast_f(my_c, j);
        const int e = c0 + j;
        if (act) {
          if (VEC4) {
            const f4 a0 = load4(h + n0 * h_stride + col);
            take(best.x, ba.x, msg<HAS_W>(k0, a0.x), e); take(best.y, ba.y, msg<HAS_W>(k0, a0.y), e);
            take(best.z, ba.z, msg<HAS_W>(k0, a0.z), e); take(best.w, ba.w, msg<HAS_W>(k0, a0.w), e);
          } else take(best.x, ba.x, msg<HAS_W>(k0, bf2f(h[n0 * h_stride + col])), e);
        }
      }
    }
    flush(cur, best, ba);
  }
}

// Row r after the walk, one wave per row.  A row cut by chunk boundaries: the tail partial of the chunk it starts in, then the
// head partials of the following chunks in chunk order (= edge order) under the same strict >; a row without live edges is
// cleared: out 0, arg -1.
template <bool VEC4>
__global__ void __launch_bounds__(SM_TPB) k_spmm_max_fixup(const int* __restrict__ row_ptr, int n_rows, const int* __restrict__ nnz_dev,
                                                          int nnz_host, int dim, const float* __restrict__ part,
                                                          bf16_t* __restrict__ out, int64_t out_stride, int* __restrict__ arg,
                                                          int64_t arg_stride, int EC) {
  const int r = blockIdx.x * (SM_TPB / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int nnz = nnz_dev ? max(0, min(*nnz_dev, nnz_host)) : nnz_host;
  const int lane = lane_id();
  const int rb = row_ptr[r], re = min(row_ptr[r + 1], nnz);
  constexpr int W = VEC4 ? 4 : 1;
  if (re <= rb) {
    for (int col = lane * W; col < dim; col += 64 * W) {
      if (VEC4) {
        store4<false>(out, r * out_stride + col, f4{0.f, 0.f, 0.f, 0.f});
        if (arg) store4i(arg + r * arg_stride + col, i4{-1, -1, -1, -1});
      } else {
        out[r * out_stride + col] = 0;
        if (arg) arg[r * arg_stride + col] = -1;
      }
    }
    return;
  }
  const int c = rb / EC, c_end = (re - 1) / EC;
  if (c_end == c) return;                                   // finished by its chunk
  for (int col = lane * W; col < dim; col += 64 * W) {
    const float* q = part + ((int64_t)c * 2 + 1) * 2 * dim + col;
    if (VEC4) {
      f4 best = load4f(q);
      i4 ba = arg ? load4i(reinterpret_cast<const int*>(q) + dim) : i4{0, 0, 0, 0};
      for (int cc = c + 1; cc <= c_end; ++cc) {
        const float* u = part + ((int64_t)cc * 2) * 2 * dim + col;
        const f4 v = load4f(u);
        const i4 va = arg ? load4i(reinterpret_cast<const int*>(u) + dim) : i4{0, 0, 0, 0};
        take(best.x, ba.x, v.x, va.x); take(best.y, ba.y, v.y, va.y);
        take(best.z, ba.z, v.z, va.z); take(best.w, ba.w, v.w, va.w);
      }
      store4<false>(out, r * out_stride + col, best);
      if (arg) store4i(arg + r * arg_stride + col, ba);
    } else {
      float best = q[0];
      int ba = arg ? reinterpret_cast<const int*>(q)[dim] : 0;
      for (int cc = c + 1; cc <= c_end; ++cc) {
        const float* u = part + ((int64_t)cc * 2) * 2 * dim + col;
        take(best, ba, u[0], arg ? reinterpret_cast<const int*>(u)[dim] : 0);
      }
      out[r * out_stride + col] = f2bf(best);
      if (arg) arg[r * arg_stride + col] = ba;
    }
  }
}

// the ReLU's mask on four finished sums: a column whose activation is not above zero (either zero, or negative) sends +0
__device__ __forceinline__ f4 relu_mask4(f4 v, f4 a) {
  return f4{a.x > 0.f ? v.x : 0.f, a.y > 0.f ? v.y : 0.f, a.z > 0.f ? v.z : 0.f, a.w > 0.f ? v.w : 0.f};
}

// ---- backward: a gather through the by-source index ---------------------------------------------------------------------------
// Entry k of the by-source list is edge e = t_edge[k] of source row_ptr-row j; column c of it contributes w_e * gout[dst_e, c]
// iff arg[dst_e, c] == e.  Per edge the wave reads a gout row (2 B per column) and an arg row (4 B per column).
// RELU: a finished source row is stored under the mask act[r] > 0 -- one bf16 row read per source row of the chunk, issued where the
// row BEGINS (its address needs the row id alone), so it travels with the row's first edge loads and the store does not wait for it.
template <bool VEC4, bool HAS_W, bool RELU>
__global__ void __launch_bounds__(SM_TPB) k_spmm_max_bwd(const int* __restrict__ row_ptr, const int* __restrict__ t_edge,
                                                        const int* __restrict__ src, const int* __restrict__ dst,
                                                        const bf16_t* __restrict__ w, const bf16_t* __restrict__ g, int64_t g_stride,
                                                        const int* __restrict__ arg, int64_t arg_stride,
                                                        const bf16_t* __restrict__ actv, int64_t act_stride,
                                                        const int* __restrict__ nnz_dev, int nnz_host, int dim,
                                                        bf16_t* __restrict__ gh, int64_t gh_stride, float* __restrict__ part, int EC) {
  const int nnz = nnz_dev ? max(0, min(*nnz_dev, nnz_host)) : nnz_host;
  const int ci = blockIdx.x * (SM_TPB / 64) + (threadIdx.x >> 6);
  if ((int64_t)ci * EC >= nnz) return;
  const int lane = lane_id();
  const int c0 = ci * EC, c1 = min(nnz, c0 + EC), cnt = c1 - c0;
  int my_row = -1, my_n = 0, my_e = -1;
  float my_c = 1.0f;
  if (lane < cnt) {
    my_e = t_edge[c0 + lane];
    my_row = src[my_e];
    my_n = dst[my_e];
    if (HAS_W) my_c = bf2f(w[my_e]);
  }
  constexpr int W = VEC4 ? 4 : 1;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int col0 = 0; col0 < dim; col0 += 64 * W) {
    const int col = col0 + lane * W;
    const bool act = col < dim;
    // the activations of row r's columns (RELU only; r is a live source of this chunk: in bounds)
    auto act_of = [&](int r) {
      f4 a = zero;
      if (RELU && act) {
        if (VEC4) a = load4(actv + r * act_stride + col);
        else a.x = bf2f(actv[r * act_stride + col]);
      }
      return a;
    };
    auto flush = [&](int r, f4 acc, f4 am) {
      const int rb = row_ptr[r], re = min(row_ptr[r + 1], nnz);
      const bool starts = rb >= c0, ends = re <= c1;
      if (!act) return;
      if (starts && ends) {
        if (RELU) acc = relu_mask4(acc, am);
        if (VEC4) store4<false>(gh, r * gh_stride + col, acc);
        else gh[r * gh_stride + col] = f2bf(acc.x);
      } else {
        float* q = part + ((int64_t)ci * 2 + (starts ? 1 : 0)) * dim + col;
        if (VEC4) store4f(q, acc);
        else q[0] = acc.x;
      }
    };
    // one edge's masked contribution
    auto add4 = [&](f4& acc, float k, int e, f4 a, i4 m) {
      acc.x += m.x == e ? k * a.x : 0.f; acc.y += m.y == e ? k * a.y : 0.f;
      acc.z += m.z == e ? k * a.z : 0.f; acc.w += m.w == e ? k * a.w : 0.f;
    };
    int cur = bcast_i(my_row, 0);
    f4 acc = zero, am = act_of(cur);
    for (int j = 0; j < cnt;) {
      const int r = bcast_i(my_row, j);
      if (r != cur) { flush(cur, acc, am); acc = zero; cur = r; am = act_of(r); }
      const int run = __popcll(__ballot(my_row == r && lane >= j));
      const int end = j + run;
      for (; j + 4 <= end; j += 4) {
        const int n0 = bcast_i(my_n, j), n1 = bcast_i(my_n, j + 1), n2 = bcast_i(my_n, j + 2), n3 = bcast_i(my_n, j + 3);
        const int e0 = bcast_i(my_e, j), e1 = bcast_i(my_e, j + 1), e2 = bcast_i(my_e, j + 2), e3 = bcast_i(my_e, j + 3);
        const float k0 = bcast_f(my_c, j), k1 = bcast_f(my_c, j + 1), k2 = bcast_f(my_c, j + 2), k3 = bcast_f(my_c, j + 3);
        if (act) {
          if (VEC4) {
            const f4 a0 = load4(g + n0 * g_stride + col), a1 = load4(g + n1 * g_stride + col);
            const f4 a2 = load4(g + n2 * g_stride + col), a3 = load4(g + n3 * g_stride + col);
            const i4 m0 = load4i(arg + n0 * arg_stride + col), m1 = load4i(arg + n1 * arg_stride + col);
            const i4 m2 = load4i(arg + n2 * arg_stride + col), m3 = load4i(arg + n3 * arg_stride + col);
            add4(acc, k0, e0, a0, m0); add4(acc, k1, e1, a1, m1); add4(acc, k2, e2, a2, m2); add4(acc, k3, e3, a3, m3);
          } else {
            const float a0 = bf2f(g[n0 * g_stride + col]), a1 = bf2f(g[n1 * g_stride + col]);
            const float a2 = bf2f(g[n2 * g_stride + col]), a3 = bf2f(g[n3 * g_stride + col]);
            const int m0 = arg[n0 * arg_stride + col], m1 = arg[n1 * arg_stride + col];
            const int m2 = arg[n2 * arg_stride + col], m3 = arg[n3 * arg_stride + col];
            acc.x += m0 == e0 ? k0 * a0 : 0.f; acc.x += m1 == e1 ? k1 * a1 : 0.f;
            acc.x += m2 == e2 ? k2 * a2 : 0.f; acc.x += m3 == e3 ? k3 * a3 : 0.f;
          }
        }
      }
      for (; j < end; ++j) {
        const int n0 = bcast_i(my_n, j), e0 = bcast_i(my_e, j);
        const float k0 = bcast_f(my_c, j);
        if (act) {
          if (VEC4) add4(acc, k0, e0, load4(g + n0 * g_stride + col), load4i(arg + n0 * arg_stride + col));
          else acc.x += arg[n0 * arg_stride + col] == e0 ? k0 * bf2f(g[n0 * g_stride + col]) : 0.f;
        }
      }
    }
    flush(cur, acc, am);
  }
}

// Source row r after the backward walk: chunk partials added in chunk order, one rounding; a source that sends nothing (rows
// past the live count included) is cleared -- RELU: without reading its act row; a combined row is stored under act[r] > 0.
template <bool VEC4, bool RELU>
__global__ void __launch_bounds__(SM_TPB) k_spmm_max_bwd_fixup(const int* __restrict__ row_ptr, int n_rows,
                                                              const int* __restrict__ nnz_dev, int nnz_host, int dim,
                                                              const float* __restrict__ part, const bf16_t* __restrict__ actv,
                                                              int64_t act_stride, bf16_t* __restrict__ gh, int64_t gh_stride, int EC) {
  const int r = blockIdx.x * (SM_TPB / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const int nnz = nnz_dev ? max(0, min(*nnz_dev, nnz_host)) : nnz_host;
  const int lane = lane_id();
  const int rb = row_ptr[r], re = min(row_ptr[r + 1], nnz);
  constexpr int W = VEC4 ? 4 : 1;
  if (re <= rb) {
    for (int col = lane * W; col < dim; col += 64 * W) {
      if (VEC4) store4<false>(gh, r * gh_stride + col, f4{0.f, 0.f, 0.f, 0.f});
      else gh[r * gh_stride + col] = 0;
    }
    return;
  }
  const int c = rb / EC, c_end = (re - 1) / EC;
  if (c_end == c) return;
  for (int col = lane * W; col < dim; col += 64 * W) {
    if (VEC4) {
      f4 am = {0.f, 0.f, 0.f, 0.f};
      if (RELU) am = load4(actv + r * act_stride + col);        // (issued in front of the partials' loads, used behind them)
      f4 sum = load4f(part + ((int64_t)c * 2 + 1) * dim + col);
      for (int cc = c + 1; cc <= c_end; ++cc) {
        const f4 u = load4f(part + ((int64_t)cc * 2) * dim + col);
        sum.x += u.x; sum.y += u.y; sum.z += u.z; sum.w += u.w;
      }
      if (RELU) sum = relu_mask4(sum, am);
      store4<false>(gh, r * gh_stride + col, sum);
    } else {
      const float am = RELU ? bf2f(actv[r * act_stride + col]) : 1.f;
      float sum = part[((int64_t)c * 2 + 1) * dim + col];
      for (int cc = c + 1; cc <= c_end; ++cc) sum += part[((int64_t)cc * 2) * dim + col];
      if (RELU) sum = am > 0.f ? sum : 0.f;
      gh[r * gh_stride + col] = f2bf(sum);
    }
  }
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p) % a == 0; }

// Both backward entry points: RELU = false is bliss_spmm_max_bwd (act unused), true bliss_spmm_max_bwd_relu.
template <bool RELU>
int max_bwd_launch(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w, const void* gout,
                   int64_t gout_stride, const int32_t* arg, int64_t arg_stride, const void* act, int64_t act_stride, int32_t n_src,
                   const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, void* partials, void* stream) {
  if (!t_indptr || !gout || !arg || !gh || n_src < 0 || nnz < 0 || dim <= 0 || (nnz > 0 && (!t_edge || !src || !dst))) return BLISS_EINVAL;
  if (gout_stride < dim || arg_stride < dim || gh_stride < dim) return BLISS_EINVAL;
  const int EC = spmm_chunk_edges(nnz);
  if (nnz > EC && !partials) return BLISS_EINVAL;
  if (n_src == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = dim % 4 == 0 && gout_stride % 4 == 0 && arg_stride % 4 == 0 && gh_stride % 4 == 0 && al(gout, 8) && al(arg, 16) &&
                    al(gh, 8) && al(partials, 16) && (!RELU || (act_stride % 4 == 0 && al(act, 8)));
  const int nchunks = (nnz + EC - 1) / EC;
  const dim3 block(SM_TPB), grid((nchunks + SM_TPB / 64 - 1) / (SM_TPB / 64)), gfix((n_src + SM_TPB / 64 - 1) / (SM_TPB / 64));
#define GO(V, HW) PROF_LAUNCH(RELU ? BK_SPMM_MAX_BWD_RELU : BK_SPMM_MAX_BWD, st, k_spmm_max_bwd<V, HW, RELU><<<grid, block, 0, st>>>(t_indptr, t_edge, src, dst, (const bf16_t*)w, (const bf16_t*)gout, gout_stride, arg, arg_stride, (const bf16_t*)act, act_stride, nnz_dev, nnz, dim, (bf16_t*)gh, gh_stride, (float*)partials, EC))
  if (nchunks > 0) {
    if (vec4) { if (w) GO(true, true); else GO(true, false); }
    else      { if (w) GO(false, true); else GO(false, false); }
  }
#undef GO
#define FIX(V) PROF_LAUNCH(RELU ? BK_SPMM_MAX_BWD_RELU_FIXUP : BK_SPMM_MAX_BWD_FIXUP, st, k_spmm_max_bwd_fixup<V, RELU><<<gfix, block, 0, st>>>(t_indptr, n_src, nnz_dev, nnz, dim, (const float*)partials, (const bf16_t*)act, act_stride, (bf16_t*)gh, gh_stride, EC))
  if (vec4) FIX(true); else FIX(false);
#undef FIX
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int64_t bliss_spmm_max_partial_bytes(int32_t nnz_bound, int32_t dim) {
  if (nnz_bound < 0 || dim <= 0) return BLISS_EINVAL;
  const int EC = spmm_chunk_edges(nnz_bound);
  const int64_t nchunks = ((int64_t)nnz_bound + EC - 1) / EC;
  return nchunks * 2 * 2 * (int64_t)dim * 4;                // per chunk a head and a tail slot of dim values + dim args
}

int bliss_spmm_max_fwd(const int32_t* indptr, const int32_t* src, const int32_t* dst, const void* w, const void* h,
                       int64_t h_stride, int32_t n_dst, const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* out,
                       int64_t out_stride, int32_t* arg, int64_t arg_stride, void* partials, void* stream) {
  if (!indptr || !h || !out || n_dst < 0 || nnz < 0 || dim <= 0 || (nnz > 0 && (!src || !dst))) return BLISS_EINVAL;
  if (h_stride < dim || out_stride < dim || (arg && arg_stride < dim)) return BLISS_EINVAL;
  const int EC = spmm_chunk_edges(nnz);
  if (nnz > EC && !partials) return BLISS_EINVAL;           // partials only when a row can be cut: more than one chunk
  if (n_dst == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = dim % 4 == 0 && h_stride % 4 == 0 && out_stride % 4 == 0 && al(h, 8) && al(out, 8) && al(partials, 16) &&
                    (!arg || (arg_stride % 4 == 0 && al(arg, 16)));
  const int nchunks = (nnz + EC - 1) / EC;
  const dim3 block(SM_TPB), grid((nchunks + SM_TPB / 64 - 1) / (SM_TPB / 64)), gfix((n_dst + SM_TPB / 64 - 1) / (SM_TPB / 64));
#define GO(V, HW) PROF_LAUNCH(BK_SPMM_MAX_FWD, st, k_spmm_max<V, HW><<<grid, block, 0, st>>>(indptr, src, dst, (const bf16_t*)w, (const bf16_t*)h, h_stride, nnz_dev, nnz, dim, (bf16_t*)out, out_stride, arg, arg_stride, (float*)partials, EC))
  if (nchunks > 0) {
    if (vec4) { if (w) GO(true, true); else GO(true, false); }
    else      { if (w) GO(false, true); else GO(false, false); }
  }
#undef GO
#define FIX(V) PROF_LAUNCH(BK_SPMM_MAX_FIXUP, st, k_spmm_max_fixup<V><<<gfix, block, 0, st>>>(indptr, n_dst, nnz_dev, nnz, dim, (const float*)partials, (bf16_t*)out, out_stride, arg, arg_stride, EC))
  if (vec4) FIX(true); else FIX(false);
#undef FIX
  return (int)hipGetLastError();
}

int bliss_spmm_max_bwd(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w,
                       const void* gout, int64_t gout_stride, const int32_t* arg, int64_t arg_stride, int32_t n_src,
                       const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh, int64_t gh_stride, void* partials, void* stream) {
  return max_bwd_launch<false>(t_indptr, t_edge, src, dst, w, gout, gout_stride, arg, arg_stride, nullptr, 0, n_src, nnz_dev, nnz, dim, gh,
                               gh_stride, partials, stream);
}

int bliss_spmm_max_bwd_relu(const int32_t* t_indptr, const int32_t* t_edge, const int32_t* src, const int32_t* dst, const void* w,
                            const void* gout, int64_t gout_stride, const int32_t* arg, int64_t arg_stride, const void* act,
                            int64_t act_stride, int32_t n_src, const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* gh,
                            int64_t gh_stride, void* partials, void* stream) {
  if (!act || act_stride < dim) return BLISS_EINVAL;
  return max_bwd_launch<true>(t_indptr, t_edge, src, dst, w, gout, gout_stride, arg, arg_stride, act, act_stride, n_src, nnz_dev, nnz, dim,
                              gh, gh_stride, partials, stream);
}

}  // extern "C"
