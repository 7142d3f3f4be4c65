// The element-wise glue around a GATv2 layer's message passing, bounded by the block's device-side counts.
//
// model.py:101-106 (residual add, activation), :228-232 (flatten(1) of a hidden layer / mean over the heads of the last one) and
// the NEXT layer's feat_drop (:66) are about ten element-wise launches of the tensor library per layer and direction, each over
// all capacity rows of a padded block.  Here they are one launch per direction over the rows r < min(n_rows, *n_rows_dev):
//     x   = rst[r, h, d] (+ res[r, h, d], rounded to bf16: the tensor add)
//     y   = ELU(x), rounded to bf16                        (act = 1; act = 0: y = x)
//     z   = y as [H*D] (flatten)   or   bf16( (sum_h y[h, d]) * (1 / H) )  -- fp32 sum, ONE rounding, as mean(1) does
//     out = keep ? bf16(z * 1/(1-p)) : 0                    (p > 0; the keyed mask of spmm.hip / sage.hip: drop_hash(seed,
//                                                            launch counter, r * width + column) -- no row's mask depends on how
//                                                            many rows the buffer has)
// Rows at or past the live count are written as zeros and nothing of their inputs is read.  The backward applies the mask and
// scale, the transpose of the flatten / head mean, the ELU derivative and hands the same row to the residual branch.
// The ELU derivative is taken where torch's out-of-place elu takes it: from the INPUT x (d = g * exp(x) for x <= 0), which is
// recomputed here as the forward formed it (bf16(rst + res)) -- nothing extra is stored.
// One thread per 8 bf16 (16-byte accesses where rows and pointers allow, element-wise otherwise), a grid-stride loop over
// (row, column group) items, the count read once (a uniform load), no atomics: nothing is reduced across rows.
#include "common.cuh"
#include "bliss_gnn.h"

namespace {

#define GG_TPB 256
#define GG_MAX_WGS 2048

struct Glue {
  const bf16_t* rst; long long rst_stride;
  const bf16_t* res; long long res_stride;
  int n_rows; const int* n_rows_dev;
  int H, D, act, head_mean;
  unsigned drop_thresh; float drop_scale; unsigned seed; unsigned long long* ctr; unsigned* ctr_used;
  bf16_t* out; long long out_stride;
  bf16_t* pre; long long pre_stride;
  const bf16_t* dout; long long dout_stride;
  bf16_t* din; long long din_stride;
  int vec;
};

// 8 consecutive elements from p, `valid` of them inside the row (the others read as 0)
__device__ __forceinline__ void gg_load8(const bf16_t* p, int valid, bool vec, float (&v)[8]) {
  if (vec && valid >= 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = bf2f((bf16_t)(w[j] & 0xffffu)); v[2 * j + 1] = bf2f((bf16_t)(w[j] >> 16)); }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < valid ? bf2f(p[j]) : 0.f;
  }
}
__device__ __forceinline__ void gg_store8(bf16_t* p, int valid, bool vec, const float (&v)[8]) {
  if (vec && valid >= 8) {
    uint4 q;
    q.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16); q.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    q.z = (uint32_t)f2bf(v[4]) | ((uint32_t)f2bf(v[5]) << 16); q.w = (uint32_t)f2bf(v[6]) | ((uint32_t)f2bf(v[7]) << 16);
    *reinterpret_cast<uint4*>(p) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < valid) p[j] = f2bf(v[j]);
  }
}
__device__ __forceinline__ void gg_zero8(bf16_t* p, int valid, bool vec) {
  if (vec && valid >= 8) *reinterpret_cast<uint4*>(p) = make_uint4(0, 0, 0, 0);
  else {
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < valid) p[j] = 0;
  }
}

__device__ __forceinline__ int gg_live(const Glue& p) {
  int n = p.n_rows;
  if (p.n_rows_dev) { const int t = *p.n_rows_dev; n = t < n ? t : n; }
  return n < 0 ? 0 : n;
}

// x = rst (+ res), the add rounded to bf16, for 8 columns of head h
__device__ __forceinline__ void gg_preact(const Glue& p, long long row, int col, int valid, float (&x)[8]) {
  gg_load8(p.rst + row * p.rst_stride + col, valid, p.vec, x);
  if (p.res) {
    float y[8];
    gg_load8(p.res + row * p.res_stride + col, valid, p.vec, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = rbf(x[j] + y[j]);
  }
}

__global__ void __launch_bounds__(GG_TPB) k_gat_glue_fwd(Glue p) {
  const int n = gg_live(p);
  const int H = p.H, D = p.D, HD = H * D;
  const int width = p.head_mean ? D : HD, G = (width + 7) / 8;
  const uint32_t ctr = p.drop_thresh ? (uint32_t)__hip_atomic_load(p.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  if (p.drop_thresh && p.ctr_used && blockIdx.x == 0 && threadIdx.x == 0) *p.ctr_used = ctr;
  const float inv_h = 1.0f / (float)H;
  const long long total = (long long)p.n_rows * G;
  for (long long idx = (long long)blockIdx.x * GG_TPB + threadIdx.x; idx < total; idx += (long long)gridDim.x * GG_TPB) {
    const long long row = idx / G;
    const int c0 = (int)(idx - row * G) * 8, valid = width - c0;
    bf16_t* o = p.out + row * p.out_stride + c0;
    if (row >= n) {                                     // capacity padding: zeros, nothing read
      gg_zero8(o, valid, p.vec);
      if (p.pre) gg_zero8(p.pre + row * p.pre_stride + c0, valid, p.vec);
      continue;
    }
    float z[8];
    if (p.head_mean) {
      // fp32 sum over the heads, four running sums (head h into sum h & 3) combined in order: up to four heads this IS the
      // sequential sum; one rounding after the product with 1 / H
      float acc[4][8];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[a][j] = 0.f;
      for (int h = 0; h < H; ++h) {
        float x[8];
        gg_preact(p, row, h * D + c0, valid, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float y = x[j];
          if (p.act) y = y <= 0.f ? rbf(expm1f(y)) : y;
          const int a = h & 3;
          if (a == 0) acc[0][j] += y; else if (a == 1) acc[1][j] += y; else if (a == 2) acc[2][j] += y; else acc[3][j] += y;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = rbf((((acc[0][j] + acc[1][j]) + acc[2][j]) + acc[3][j]) * inv_h);
    } else {
      gg_preact(p, row, c0, valid, z);
      if (p.act) {
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = z[j] <= 0.f ? rbf(expm1f(z[j])) : z[j];
      }
    }
    if (p.pre) gg_store8(p.pre + row * p.pre_stride + c0, valid, p.vec, z);
    if (p.drop_thresh) {
      const uint32_t base = (uint32_t)(row * width + c0);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = drop_hash(p.seed, ctr, base + j) >= p.drop_thresh ? rbf(z[j] * p.drop_scale) : 0.f;
    }
    gg_store8(o, valid, p.vec, z);
  }
}

__global__ void __launch_bounds__(GG_TPB) k_gat_glue_bwd(Glue p) {
  const int n = gg_live(p);
  const int H = p.H, D = p.D, HD = H * D;
  const int width = p.head_mean ? D : HD, G = (width + 7) / 8;
  const uint32_t ctr = p.drop_thresh ? *p.ctr_used : 0u;
  const float inv_h = 1.0f / (float)H;
  const int copies = p.head_mean ? H : 1;
  const long long total = (long long)p.n_rows * G;
  for (long long idx = (long long)blockIdx.x * GG_TPB + threadIdx.x; idx < total; idx += (long long)gridDim.x * GG_TPB) {
    const long long row = idx / G;
    const int c0 = (int)(idx - row * G) * 8, valid = width - c0;
    if (row >= n) {
      for (int h = 0; h < copies; ++h) gg_zero8(p.din + row * p.din_stride + h * D + c0, valid, p.vec);
      continue;
    }
    float g[8];
    gg_load8(p.dout + row * p.dout_stride + c0, valid, p.vec, g);
    if (p.drop_thresh) {
      const uint32_t base = (uint32_t)(row * width + c0);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = drop_hash(p.seed, ctr, base + j) >= p.drop_thresh ? rbf(g[j] * p.drop_scale) : 0.f;
    }
    if (p.head_mean) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = rbf(g[j] * inv_h);          // the head mean's transpose: the same row to every head
    }
    for (int h = 0; h < copies; ++h) {
      const int col = h * D + c0;
      float d[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = g[j];
      if (p.act) {
        float x[8];
        gg_preact(p, row, col, valid, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = x[j] <= 0.f ? rbf(g[j] * expf(x[j])) : g[j];
      }
      gg_store8(p.din + row * p.din_stride + col, valid, p.vec, d);
    }
  }
}

// the dropout stream's launch counter moves on behind the forward kernel (every workgroup has read it by then)
__global__ void k_gat_glue_bump(unsigned long long* ctr) { if (threadIdx.x == 0) *ctr += 1ull; }

// a_ij[e] = bf16( (sum_h e[e, h]) * (1 / H) ) over the live edges; the tail is left alone
__global__ void __launch_bounds__(GG_TPB) k_gat_head_mean(const bf16_t* __restrict__ e, int H, int n_edges, const int* __restrict__ n_dev,
                                                           bf16_t* __restrict__ out) {
  int n = n_edges;
  if (n_dev) { const int t = *n_dev; n = t < n ? t : n; }
  const float inv_h = 1.0f / (float)H;
  for (long long i = (long long)blockIdx.x * GG_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * GG_TPB) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < H; ++h) {
      const float v = bf2f(e[i * H + h]);
      const int a = h & 3;
      if (a == 0) acc[0] += v; else if (a == 1) acc[1] += v; else if (a == 2) acc[2] += v; else acc[3] += v;
    }
    out[i] = f2bf((((acc[0] + acc[1]) + acc[2]) + acc[3]) * inv_h);
  }
}

inline bool al16(const void* p, long long stride) { return p == nullptr || ((((uintptr_t)p) % 16 == 0) && (stride % 8 == 0)); }

bool gg_fill(const bliss_gat_glue_t* a, Glue* p, bool backward) {
  if (!a || a->n_rows <= 0 || a->heads <= 0 || a->head_dim <= 0 || (a->act != 0 && a->act != 1)) return false;
  if (a->drop_p < 0.f || a->drop_p >= 1.f) return false;
  if ((long long)a->heads * a->head_dim > (1ll << 20) || (long long)a->n_rows * a->heads * a->head_dim >= (1ll << 32)) return false;
  const bool need_x = !backward || a->act != 0;
  if (need_x && !a->rst) return false;
  if (!backward && (!a->out || (a->drop_p > 0.f && !a->drop_ctr))) return false;
  if (backward && (!a->dout || !a->din || (a->drop_p > 0.f && !a->drop_ctr_used))) return false;
  p->rst = (const bf16_t*)a->rst; p->rst_stride = a->rst_stride;
  p->res = need_x ? (const bf16_t*)a->res : nullptr; p->res_stride = a->res_stride;
  if (!need_x) p->rst = nullptr;
  p->n_rows = a->n_rows; p->n_rows_dev = a->n_rows_dev;
  p->H = a->heads; p->D = a->head_dim; p->act = a->act; p->head_mean = a->head_mean ? 1 : 0;
  p->drop_thresh = a->drop_p > 0.f ? (unsigned)((double)a->drop_p * 4294967296.0) : 0u;
  p->drop_scale = a->drop_p > 0.f ? 1.0f / (1.0f - a->drop_p) : 1.0f;
  p->seed = a->drop_seed; p->ctr = (unsigned long long*)a->drop_ctr; p->ctr_used = a->drop_ctr_used;
  p->out = backward ? nullptr : (bf16_t*)a->out; p->out_stride = a->out_stride;
  p->pre = backward ? nullptr : (bf16_t*)a->pre; p->pre_stride = a->pre_stride;
  p->dout = backward ? (const bf16_t*)a->dout : nullptr; p->dout_stride = a->dout_stride;
  p->din = backward ? (bf16_t*)a->din : nullptr; p->din_stride = a->din_stride;
  // 16-byte accesses: every row start and every column group 16-byte aligned (a head's columns start at h * D)
  p->vec = al16(p->rst, p->rst_stride) && al16(p->res, p->res_stride) && al16(p->out, p->out_stride) && al16(p->pre, p->pre_stride) &&
           al16(p->dout, p->dout_stride) && al16(p->din, p->din_stride) && (!p->head_mean || a->head_dim % 8 == 0);
  return true;
}

inline int gg_grid(long long items) {
  long long g = (items + GG_TPB - 1) / GG_TPB;
  return (int)(g < 1 ? 1 : (g > GG_MAX_WGS ? GG_MAX_WGS : g));
}

}  // namespace

extern "C" {

int bliss_gat_glue_fwd(const bliss_gat_glue_t* args, void* stream) {
  Glue p;
  if (!gg_fill(args, &p, false)) return BLISS_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int width = p.head_mean ? p.D : p.H * p.D;
  k_gat_glue_fwd<<<gg_grid((long long)p.n_rows * ((width + 7) / 8)), GG_TPB, 0, st>>>(p);
  if (p.drop_thresh) k_gat_glue_bump<<<1, 64, 0, st>>>(p.ctr);
  return (int)hipGetLastError();
}

int bliss_gat_glue_bwd(const bliss_gat_glue_t* args, void* stream) {
  Glue p;
  if (!gg_fill(args, &p, true)) return BLISS_EINVAL;
  const int width = p.head_mean ? p.D : p.H * p.D;
  k_gat_glue_bwd<<<gg_grid((long long)p.n_rows * ((width + 7) / 8)), GG_TPB, 0, (hipStream_t)stream>>>(p);
  return (int)hipGetLastError();
}

int bliss_gat_head_mean(const void* e, int32_t heads, int32_t n_edges, const int32_t* n_edges_dev, void* out, void* stream) {
  if (!e || !out || heads <= 0 || n_edges < 0) return BLISS_EINVAL;
  if (n_edges == 0) return 0;
  k_gat_head_mean<<<gg_grid(n_edges), GG_TPB, 0, (hipStream_t)stream>>>((const bf16_t*)e, heads, n_edges, n_edges_dev, (bf16_t*)out);
  return (int)hipGetLastError();
}

}  // extern "C"
