// The dense transforms of a SAGE layer on the matrix cores, fused with what surrounds them.
//
// model.py:321-333 -> dglnn.SAGEConv('mean') [DGL-recalled, SURVEY.md m2-m5]:  rst = fc_self(h_dst) + fc_neigh o mean_w(h)
// with fc_neigh BEFORE the aggregation iff in > out, then relu + dropout, and model.py:318-320 takes the row norms of
// every layer's input.  The reference (and round 1 here) runs each Linear as a library GEMM with its own launch, plus a
// gather kernel in front and an element-wise epilogue behind; at these sizes (a few thousand rows) every launch costs
// more than its arithmetic.  k_tile_gemm is ONE launch for
//     out[r, :] = epilogue( A1[r, :] . W1^T  (+ A2[r, :] . W2^T)  + bias )
// where the rows of A1 may be gathered through an index (blocks[0].srcdata['features'] = features[input_nodes],
// train_lightning.py:138 -- the gather IS the A-operand load), the epilogue is bf16 rounding, optional ReLU, optional
// dropout, and the kernel also leaves the row norms of its INPUT rows (embed_norm of this layer) and of its OUTPUT rows
// (embed_norm of the next layer).  Two argument sets can share a launch (blockIdx.y): fc_neigh over all source rows and
// fc_self over the destination rows of a W-first layer.
//
// Shape of the work: a workgroup (8 waves) owns 32 rows and all N <= 256 output columns.  The 32 input rows are staged
// ONCE in LDS (32 x K bf16 <= 66 KB for K <= 1024, 39 KB for the 602-wide features: four workgroups per CU overlap each
// other's latency chains), which is also where the input norms are taken in exactly k_embed_norm's order (same bits as the
// unfused path).  Wave w computes columns 32 w .. 32 w + 31 as one 32 x 32 tile of v_mfma_f32_32x32x16_bf16: A fragments are 16-byte LDS reads (row = lane & 31, k = 8 (lane >> 5) ..+7), B fragments
// 16-byte global (L2) reads of W[n][k..k+7] -- nn.Linear keeps W as [out, in], i.e. K-contiguous, exactly the B layout
// the instruction wants, so no operand is ever transposed.  fp32 accumulation over all of K (and both products), one
// rounding to bf16 at the store.  A row's result depends on nothing but that row: capacity-padded and exact-size blocks
// give identical bits.
#include "common.cuh"
#include "bliss_gnn.h"
#include <cstdlib>

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#define TG_TPB 512
#define TG_M 32
#define TG_WAVES (TG_TPB / 64)
#define TG_NB (256 / 32 / TG_WAVES)          // 32-column blocks per wave: 8 waves x 1 block cover the 256 columns

struct TileGemm {
  const bf16_t* a1; long long a1_stride; const int* ids;
  const bf16_t* w1; long long w1_stride; int k1;
  const bf16_t* a2; long long a2_stride; const bf16_t* w2; long long w2_stride; int k2;
  const bf16_t* bias;
  int m_bound; const int* m_dev; int n;
  bf16_t* out; long long out_stride;
  bf16_t* a_copy; long long copy_stride;
  bf16_t* in_norm; bf16_t* out_norm;
  int relu; unsigned drop_thresh; float drop_scale; unsigned seed; unsigned long long* ctr;
};

__device__ __forceinline__ int k_pad16(int k) { return (k + 15) & ~15; }
// LDS row stride (elements): K rounded to 16, plus 8: the stride is then 4 (mod 8) dwords, so the 16-byte fragment reads
// of 8 consecutive rows fall into 8 different 4-bank groups (and a 64-row tile of 602-wide rows stays below 80 KB: two
// workgroups per CU)
__device__ __host__ __forceinline__ int lds_stride(int k) {
  return ((k + 15) & ~15) + 8;
}

// sum of squares of one LDS row in k_embed_norm's order (spmm.hip): vec4 = the 4-columns-per-lane walk, else 1 per lane
__device__ __forceinline__ float row_sumsq(const bf16_t* sh, int dim, int vec4, int lane) {
  float s = 0.f;
  if (vec4) {
    for (int c = lane * 4; c < dim; c += 256) {
      const float a = bf2f(sh[c]), b = bf2f(sh[c + 1]), cc = bf2f(sh[c + 2]), d = bf2f(sh[c + 3]);
      s += a * a; s += b * b; s += cc * cc; s += d * d;
    }
  } else {
    for (int c = lane; c < dim; c += 64) { const float a = bf2f(sh[c]); s += a * a; }
  }
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  return s;
}

// bf16 norms of this wave's rows of an LDS tile, each in k_embed_norm's summation order (row_sumsq), the rows side by side:
// independent accumulators, so the LDS reads and the butterfly shuffles of the 8 rows overlap instead of queueing.
// rows_sumsq_add: the per-lane partial sums over `dim` staged columns (vec4: the 4-columns-per-lane walk); rows_norm_store: the
// butterfly and the store.  A lane's columns are lane * 4 + 256 j (or lane + 64 j), so partial sums carried over column
// panels whose width is a multiple of 256 add up in exactly the order of one walk over the whole row (k_tile_gemm_wide).
#define TG_RPW (TG_M / TG_WAVES)
__device__ __forceinline__ void rows_sumsq_add(float s[TG_RPW], const bf16_t* tile, int stride, int dim, bool vec4, int wave, int lane) {
  if (vec4) {
    for (int c = lane * 4; c < dim; c += 256)
#pragma unroll
      for (int q = 0; q < TG_RPW; ++q) {
        const bf16_t* sh = tile + (size_t)(q * TG_WAVES + wave) * stride + c;
        const float a = bf2f(sh[0]), b = bf2f(sh[1]), cc = bf2f(sh[2]), d = bf2f(sh[3]);
        s[q] += a * a; s[q] += b * b; s[q] += cc * cc; s[q] += d * d;
      }
  } else {
    for (int c = lane; c < dim; c += 64)
#pragma unroll
      for (int q = 0; q < TG_RPW; ++q) { const float a = bf2f(tile[(size_t)(q * TG_WAVES + wave) * stride + c]); s[q] += a * a; }
  }
}
__device__ __forceinline__ void rows_norm_store(float s[TG_RPW], int row0, int M, int m_bound, bf16_t* __restrict__ out, int wave, int lane) {
  for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
    for (int q = 0; q < TG_RPW; ++q) s[q] += __shfl_xor(s[q], d);
#pragma unroll
  for (int q = 0; q < TG_RPW; ++q) {
    const int r = row0 + q * TG_WAVES + wave;
    if (lane == 0 && r < m_bound) out[r] = r < M ? f2bf(sqrtf(s[q])) : (bf16_t)0;
  }
}
// (the narrow kernel's walk in one piece, kept as it was written so that k_tile_gemm compiles to the code it always had)
__device__ __forceinline__ void rows_norm(const bf16_t* tile, int stride, int dim, int row0, int M, int m_bound, bf16_t* __restrict__ out,
                                          int wave, int lane) {
  constexpr int RPW = TG_M / TG_WAVES;
  float s[RPW];
#pragma unroll
  for (int q = 0; q < RPW; ++q) s[q] = 0.f;
  if (dim % 4 == 0) {
    for (int c = lane * 4; c < dim; c += 256)
#pragma unroll
      for (int q = 0; q < RPW; ++q) {
        const bf16_t* sh = tile + (size_t)(q * TG_WAVES + wave) * stride + c;
        const float a = bf2f(sh[0]), b = bf2f(sh[1]), cc = bf2f(sh[2]), d = bf2f(sh[3]);
        s[q] += a * a; s[q] += b * b; s[q] += cc * cc; s[q] += d * d;
      }
  } else {
    for (int c = lane; c < dim; c += 64)
#pragma unroll
      for (int q = 0; q < RPW; ++q) { const float a = bf2f(tile[(size_t)(q * TG_WAVES + wave) * stride + c]); s[q] += a * a; }
  }
  for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
    for (int q = 0; q < RPW; ++q) s[q] += __shfl_xor(s[q], d);
#pragma unroll
  for (int q = 0; q < RPW; ++q) {
    const int r = row0 + q * TG_WAVES + wave;
    if (lane == 0 && r < m_bound) out[r] = r < M ? f2bf(sqrtf(s[q])) : (bf16_t)0;
  }
}

// Stage the TG_M rows of one operand in LDS.  Wave w takes rows w, w + 8, ... (4 of them), a lane the dwords lane,
// lane + 64, ... of its row (8 at the largest K; beyond the row they repeat its last dword).  Even path: the 32 loads of a
// lane are independent and leave as one batch before the first LDS store (see the opaque step below for what makes that
// hold in the compiled code) -- the gather is latency-bound (a random 1.2 KB row per id), not bandwidth-bound, so one round
// trip per operand instead of one per load is what counts.  The odd path (odd K, stride or base) loads under its masks, one
// wait per load.  row_id[lr] = the source row of tile row lr or -1 (beyond the true row count: zeros).  Optional copy-out of
// the staged rows.
__device__ __forceinline__ void stage_rows(const bf16_t* __restrict__ a, long long a_stride, const int* row_id, int k,
                                           int row0, int m_bound, bf16_t* tile, int stride, bf16_t* __restrict__ copy, long long copy_stride,
                                           int wave, int lane) {
  const int kp = k_pad16(k);
  const bool even = (k % 2 == 0) && (a_stride % 2 == 0) && (((uintptr_t)a) % 4 == 0);
  const bool copy32 = copy && (copy_stride % 2 == 0) && (((uintptr_t)copy) % 4 == 0);
  if (even) {
    const int dw = k / 2;
    constexpr int MAXC = (1024 / 2 + 63) / 64;          // dwords per lane and row at the largest K
    constexpr int RPW = TG_M / TG_WAVES, HALF = RPW;      // rows per wave, all in flight together (LDS, not registers, bounds the occupancy)
#pragma unroll
    for (int hb = 0; hb < 1; ++hb) {
      uint32_t v[HALF][MAXC];
      int ids[HALF];
#pragma unroll
      for (int q = 0; q < HALF; ++q) {
        const int id = row_id[(hb * HALF + q) * TG_WAVES + wave];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a + (long long)(id < 0 ? 0 : id) * a_stride);
        ids[q] = id;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
          // raw loads from clamped (always valid) addresses; the mask comes in a loop of its own below
          const int c = lane + 64 * j;
          v[q][j] = src[c < dw ? c : dw - 1];
        }
      }
      // Every loaded register is made opaque here, after the last load has been issued.  Written as one expression
      // (load, then select on the mask), the select became a branch, the load sank under it and every load was waited
      // for alone: 32 dependent round trips per operand.  A load cannot sink below a statement that reads its result,
      // so all HALF * MAXC loads leave back to back and the uses below wait for them in order, with counted waits.
#pragma unroll
      for (int q = 0; q < HALF; ++q)
#pragma unroll
        for (int j = 0; j < MAXC; ++j) asm volatile("" : "+v"(v[q][j]));
#pragma unroll
      for (int q = 0; q < HALF; ++q)
#pragma unroll
        for (int j = 0; j < MAXC; ++j) v[q][j] = (ids[q] >= 0 && lane + 64 * j < dw) ? v[q][j] : 0u;
#pragma unroll
      for (int q = 0; q < HALF; ++q) {
        const int lr = (hb * HALF + q) * TG_WAVES + wave, r = row0 + lr;
        uint32_t* sh = reinterpret_cast<uint32_t*>(tile + (size_t)lr * stride);
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
          const int c = lane + 64 * j;
          if (c < kp / 2) sh[c] = v[q][j];               // (c >= dw: the zero padding up to the 16-multiple)
          if (copy && r < m_bound && c < dw) {
            if (copy32) reinterpret_cast<uint32_t*>(copy + (long long)r * copy_stride)[c] = v[q][j];
            else { bf16_t* cp = copy + (long long)r * copy_stride + 2 * c; cp[0] = (bf16_t)(v[q][j] & 0xffffu); cp[1] = (bf16_t)(v[q][j] >> 16); }
          }
        }
      }
    }
  } else {
    for (int rd = 0; rd < TG_M / TG_WAVES; ++rd) {
      const int lr = rd * TG_WAVES + wave, r = row0 + lr, id = row_id[lr];
      const bf16_t* src = a + (long long)(id < 0 ? 0 : id) * a_stride;
      bf16_t* sh = tile + (size_t)lr * stride;
      for (int c = lane; c < kp; c += 64) {
        const bf16_t x = (id >= 0 && c < k) ? src[c] : (bf16_t)0;
        sh[c] = x;
        if (copy && r < m_bound && c < k) copy[(long long)r * copy_stride + c] = x;
      }
    }
  }
}

// W through LDS in slabs of 64 k: an MFMA B fragment is 16 bytes of ONE row of W per lane, so loading fragments straight
// from global memory touches 32 different cache lines per wave instruction and uses a quarter of each (measured: the
// texture path, not the matrix core, bounded the first version of this kernel at ~45 us per launch).  Staged through LDS,
// 8 consecutive threads read one row's 128 contiguous bytes; the next slab is in flight (registers) while the current one
// is multiplied.
#define TG_SLAB 64
#define TG_WSTRIDE (TG_SLAB + 8)
#define TG_WROWS 256
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct WRegs { uint4 v[TG_WROWS * TG_SLAB / 8 / TG_TPB]; };      // 4 x 16 bytes per thread

// full slab (all 64 k inside K, rows 4-byte aligned): no branch, no mask -- rows beyond N are CLAMPED to a real row (their
// columns are computed from it and never stored), so every lane issues its four 16-byte loads unconditionally.  That alone
// lets the compiler count them only where the loads outstanding are the same on every path into the use: w_first_slabs and
// mma_product are written for that.
__device__ __forceinline__ void w_slab_load_full(WRegs& g, const bf16_t* __restrict__ w, long long w_stride, int N, int slab, int tid) {
  const int part = tid & 7, k = slab * TG_SLAB + 8 * part;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(g.v) / sizeof(g.v[0])); ++i) {
    int n = i * (TG_TPB / 8) + (tid >> 3);
    n = n < N ? n : N - 1;
    const u32x4_a4 q = *reinterpret_cast<const u32x4_a4*>(w + (long long)n * w_stride + k);
    g.v[i] = make_uint4(q[0], q[1], q[2], q[3]);
  }
}
// the last, partial slab where the full path's predicate holds and K is even (rows are whole dwords): every lane loads its
// 4 x 4 dwords unconditionally, from element indices clamped into [0, K - 2] of its (clamped) row, and what lies at or
// past K is zeroed afterwards.  One batch of 16 loads: the opaque step between the loads and the masks keeps the compiler
// from sinking a load under its mask (as in stage_rows).
__device__ __forceinline__ void w_slab_load_tail_even(WRegs& g, const bf16_t* __restrict__ w, long long w_stride, int N, int K, int slab, int tid) {
  constexpr int NV = (int)(sizeof(g.v) / sizeof(g.v[0]));
  const int part = tid & 7, k = slab * TG_SLAB + 8 * part;
  uint32_t x[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    int n = i * (TG_TPB / 8) + (tid >> 3);
    n = n < N ? n : N - 1;
    const bf16_t* p = w + (long long)n * w_stride;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int e = k + 2 * d;
      x[i][d] = *reinterpret_cast<const uint32_t*>(p + (e < K ? e : K - 2));
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int d = 0; d < 4; ++d) asm volatile("" : "+v"(x[i][d]));
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int d = 0; d < 4; ++d) x[i][d] = k + 2 * d < K ? x[i][d] : 0u;
    g.v[i] = make_uint4(x[i][0], x[i][1], x[i][2], x[i][3]);
  }
}
// the partial last slab of an odd K, or any slab of an oddly aligned W: element-wise under masks, one wait per load
__device__ __forceinline__ void w_slab_load_tail(WRegs& g, const bf16_t* __restrict__ w, long long w_stride, int N, int K, int slab, int tid) {
  const int part = tid & 7, k = slab * TG_SLAB + 8 * part;
  for (int i = 0; i < (int)(sizeof(g.v) / sizeof(g.v[0])); ++i) {
    int n = i * (TG_TPB / 8) + (tid >> 3);
    n = n < N ? n : N - 1;
    const bf16_t* p = w + (long long)n * w_stride + k;
    union { uint4 u; bf16_t e[8]; } t;
    t.u = make_uint4(0, 0, 0, 0);
    for (int j = 0; j < 8; ++j) if (k + j < K) t.e[j] = p[j];
    g.v[i] = t.u;
  }
}
// how many leading slabs of this W take the branch-free path
__device__ __forceinline__ int w_full_slabs(const bf16_t* w, long long w_stride, int K) {
  return ((w_stride % 2 == 0) && (((uintptr_t)w) % 4 == 0)) ? K / TG_SLAB : 0;
}
// The first two slabs of a product: requested by the caller before mma_product so that they arrive behind other work.  Both
// sets are requested on one path, ga before gb (a W of a single full slab asks for slab 0 twice): mma_product's counted
// waits rest on gb's loads being the younger ones on EVERY path that reaches them.
__device__ __forceinline__ void w_first_slabs(WRegs& ga, WRegs& gb, const bf16_t* __restrict__ w, long long w_stride, int N, int K, int tid) {
  const int nf = w_full_slabs(w, w_stride, K);
  if (nf > 0) {
    w_slab_load_full(ga, w, w_stride, N, 0, tid);
    w_slab_load_full(gb, w, w_stride, N, nf > 1 ? 1 : 0, tid);
  }
}
__device__ __forceinline__ void w_slab_store(const WRegs& g, bf16_t* wl, int tid) {
  const int part = tid & 7;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(g.v) / sizeof(g.v[0])); ++i) {
    const int n = i * (TG_TPB / 8) + (tid >> 3);
    *reinterpret_cast<uint4*>(wl + (size_t)n * TG_WSTRIDE + 8 * part) = g.v[i];
  }
}

// acc += A_tile[32 x K] . W[N x K]^T for this wave's 64 columns (n0 ..); all four waves take part in the slab traffic
__device__ __forceinline__ void mma_product(WRegs& ga, WRegs& gb, const bf16_t* tile, int stride, int k, const bf16_t* __restrict__ w,
                                            long long w_stride, int n0, int N, bf16_t* wl, int tid, int lane, f32x16_t acc[TG_NB]) {
  const int kp = k_pad16(k), r = lane & 31, h = lane >> 5;
  const int nslab = (kp + TG_SLAB - 1) / TG_SLAB;
  // full: all four 16-steps of the slab lie inside K (a literal at every call, so the test folds away and the four steps'
  // LDS reads are issued together instead of one read, one wait, one MFMA at a time)
  auto multiply = [&](int sl, bool full) {
    if (n0 < N) {
#pragma unroll
      for (int st = 0; st < TG_SLAB / 16; ++st) {
        const int ks = sl * TG_SLAB + 16 * st;
        if (full || ks < kp) {
          const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(tile + (size_t)r * stride + ks + 8 * h);
#pragma unroll
          for (int nb = 0; nb < TG_NB; ++nb) {
            const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(wl + (size_t)(n0 + 32 * nb + r) * TG_WSTRIDE + 16 * st + 8 * h);
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[nb], 0, 0, 0);
          }
        }
      }
    }
  };
  // Two register sets (ga: even slabs, gb: odd), two slabs in flight beside the one being multiplied; the caller has
  // requested slabs 0 and 1.  Only full slabs run through this pipeline.  The wait before a set's LDS store must count
  // that set's loads and leave the other set's younger ones outstanding, and the compiler can only count what is the
  // same on every path into the store: with the prefetches under `if (sl + 2 < nfull)` it was not, and each store waited
  // for everything.  So the steady loop refills both sets on every trip, without a condition, and the last one to three
  // slabs, which refill less, are written out after it.
  const int nfull = w_full_slabs(w, w_stride, k);
  auto step = [&](WRegs& g, int sl, int next) {           // next < 0: nothing left to request for this set
    __syncthreads();                                      // the previous slab has been consumed
    w_slab_store(g, wl, tid);
    if (next >= 0) w_slab_load_full(g, w, w_stride, N, next, tid);
    __syncthreads();
    multiply(sl, true);
  };
  int sl = 0;
  for (; sl + 3 < nfull; sl += 2) {
    step(ga, sl, sl + 2);
    step(gb, sl + 1, sl + 3);
  }
  const int left = nfull - sl;
  if (left == 3) {
    step(ga, sl, sl + 2);
    step(gb, sl + 1, -1);
    step(ga, sl + 2, -1);
  } else if (left == 2) {
    step(ga, sl, -1);
    step(gb, sl + 1, -1);
  } else if (left == 1) {
    step(ga, sl, -1);
  }
  // the partial last slab (K not a multiple of 64) or an oddly aligned W: one slab at a time
  const bool dword_tail = nfull * TG_SLAB < kp && (k % 2 == 0) && (w_stride % 2 == 0) && (((uintptr_t)w) % 4 == 0);
  if (dword_tail) {
    WRegs t;
    w_slab_load_tail_even(t, w, w_stride, N, k, nfull, tid);
    __syncthreads();
    w_slab_store(t, wl, tid);
    __syncthreads();
    multiply(nfull, false);
  } else {
    for (int s = nfull; s < nslab; ++s) {
      WRegs t;
      w_slab_load_tail(t, w, w_stride, N, k, s, tid);
      __syncthreads();
      w_slab_store(t, wl, tid);
      __syncthreads();
      multiply(s, false);
    }
  }
}

// WIDE (k_tile_gemm_wide): K is walked in panels of TG_PANEL columns, ONE operand panel in LDS at a time (66 KB at any K); the
// accumulators and the norm's partial sums stay in registers across the panels and across both products.  The k order is the
// narrow kernel's (ascending 16-steps, operand 1 first), a panel boundary is a slab boundary, and one panel IS the narrow walk:
// at K <= TG_PANEL both kernels give the same bits.
#define TG_PANEL 1024
template <bool WIDE>
__device__ __forceinline__ void tile_gemm_body(const TileGemm& p, bf16_t* lds, int* row_id, int dbg) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int M = p.m_bound;
  if (p.m_dev) { const int t = *p.m_dev; M = t < M ? t : M; }
  const int row0 = blockIdx.x * TG_M;
  const uint32_t ctr = p.drop_thresh ? (uint32_t)__hip_atomic_load(p.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  const int N = p.n;
  if (row0 >= p.m_bound) return;                             // (workgroup-uniform: the other argument set has more tiles)
  if (row0 >= M) {
    // a tile of capacity padding: nothing to compute, but what later passes read of these rows must be finite (zero)
    for (int lr = wave; lr < TG_M; lr += TG_WAVES) {
      const int r = row0 + lr;
      if (r >= p.m_bound) break;
      for (int c = lane; c < N; c += 64) p.out[(long long)r * p.out_stride + c] = 0;
      if (p.a_copy) for (int c = lane; c < p.k1; c += 64) p.a_copy[(long long)r * p.copy_stride + c] = 0;
      if (lane == 0) { if (p.in_norm) p.in_norm[r] = 0; if (p.out_norm) p.out_norm[r] = 0; }
    }
    return;
  }
  const int n0 = wave * 32 * TG_NB;
  float bias_v[TG_NB];
#pragma unroll
  for (int nb = 0; nb < TG_NB; ++nb) bias_v[nb] = 0.f;
#pragma unroll
  for (int nb = 0; nb < TG_NB; ++nb) { const int col = n0 + 32 * nb + (lane & 31); if (p.bias && col < N) bias_v[nb] = bf2f(p.bias[col]); }
  WRegs ga, gb;
  f32x16_t acc[TG_NB];
  if constexpr (WIDE) {
    const int kmax = p.k1 > p.k2 ? p.k1 : p.k2;
    bf16_t* wl = lds + (size_t)TG_M * lds_stride(kmax < TG_PANEL ? kmax : TG_PANEL);     // the W slab behind the one staged panel
    if (tid < TG_M) {
      const int r = row0 + tid;
      row_id[tid] = r < M ? (p.ids ? p.ids[r] : r) : -1;
      row_id[TG_M + tid] = r < M ? r : -1;
    }
#pragma unroll
    for (int m = 0; m < TG_NB; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    float ss[TG_RPW];
#pragma unroll
    for (int q = 0; q < TG_RPW; ++q) ss[q] = 0.f;
    const bool vec4 = p.k1 % 4 == 0;                        // (on the full row length, as k_embed_norm chooses)
    for (int op = 0; op < (p.k2 ? 2 : 1); ++op) {
      const bf16_t* a = op ? p.a2 : p.a1;
      const bf16_t* w = op ? p.w2 : p.w1;
      const long long a_stride = op ? p.a2_stride : p.a1_stride, w_stride = op ? p.w2_stride : p.w1_stride;
      const int K = op ? p.k2 : p.k1;
      for (int c0 = 0; c0 < K; c0 += TG_PANEL) {
        // every fast-path predicate below is taken on the panel's own base pointer and width
        const int pw = K - c0 < TG_PANEL ? K - c0 : TG_PANEL, st = lds_stride(pw);
        w_first_slabs(ga, gb, w + c0, w_stride, N, pw, tid);
        __syncthreads();                                    // every wave has multiplied the previous panel (first panel: row_id is set)
        stage_rows(a + c0, a_stride, row_id + op * TG_M, pw, row0, p.m_bound, lds, st, (op == 0 && p.a_copy) ? p.a_copy + c0 : nullptr,
                   p.copy_stride, wave, lane);
        __syncthreads();
        if (op == 0 && p.in_norm) rows_sumsq_add(ss, lds, st, pw, vec4, wave, lane);
        mma_product(ga, gb, lds, st, pw, w + c0, w_stride, n0, N, wl, tid, lane, acc);
      }
      if (op == 0 && p.in_norm) rows_norm_store(ss, row0, M, p.m_bound, p.in_norm, wave, lane);   // model.py:318-320 of THIS layer
    }
  } else {
    const int s1 = lds_stride(p.k1), s2 = p.k2 ? lds_stride(p.k2) : 0;
    bf16_t* t1 = lds;
    bf16_t* t2 = lds + (size_t)TG_M * s1;
    bf16_t* wl = lds + (size_t)TG_M * (s1 + s2);              // the W slab behind the staged rows
    // the first two W slabs depend on nothing: requested now, they arrive while the rows are gathered
    {
      w_first_slabs(ga, gb, p.w1, p.w1_stride, N, p.k1, tid);
    }
    if (tid < TG_M) {
      const int r = row0 + tid;
      row_id[tid] = r < M ? (p.ids ? p.ids[r] : r) : -1;
      row_id[TG_M + tid] = r < M ? r : -1;
    }
    __syncthreads();
    if (!(dbg & 1)) stage_rows(p.a1, p.a1_stride, row_id, p.k1, row0, p.m_bound, t1, s1, p.a_copy, p.copy_stride, wave, lane);
    if (p.k2) stage_rows(p.a2, p.a2_stride, row_id + TG_M, p.k2, row0, p.m_bound, t2, s2, nullptr, 0, wave, lane);
    __syncthreads();
    if (p.in_norm && !(dbg & 4)) rows_norm(t1, s1, p.k1, row0, M, p.m_bound, p.in_norm, wave, lane);   // model.py:318-320 of THIS layer
#pragma unroll
    for (int m = 0; m < TG_NB; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    if (!(dbg & 2)) mma_product(ga, gb, t1, s1, p.k1, p.w1, p.w1_stride, n0, N, wl, tid, lane, acc);
    if (p.k2) {
      w_first_slabs(ga, gb, p.w2, p.w2_stride, N, p.k2, tid);
      mma_product(ga, gb, t2, s2, p.k2, p.w2, p.w2_stride, n0, N, wl, tid, lane, acc);
    }
  }
  __syncthreads();                                          // every wave is done reading the staged rows: reuse the LDS for the output tile
  const int so = ((N + 63) & ~63) + 8;
  bf16_t* ot = lds;
  if (n0 < N) {
#pragma unroll
    for (int m = 0; m < TG_NB; ++m) {                        // (m = the wave's column blocks)
      const int col = n0 + 32 * m + (lane & 31);
      const float bv = bias_v[m];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int lr = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        float t = rbf(acc[m][i] + bv);                       // fp32 accumulator + bias, ONE rounding to bf16
        if (p.relu) t = t > 0.f ? t : 0.f;
        if (p.drop_thresh) {
          const bool keep = drop_hash(p.seed, ctr, (uint32_t)((row0 + lr) * N + col)) >= p.drop_thresh;
          t = keep ? rbf(t * p.drop_scale) : 0.f;
        }
        ot[(size_t)lr * so + col] = (row0 + lr < M && col < N) ? f2bf(t) : (bf16_t)0;
      }
    }
  }
  __syncthreads();
  const bool pair_ok = (N % 2 == 0) && (p.out_stride % 2 == 0) && (((uintptr_t)p.out) % 4 == 0);
  for (int lr = wave; lr < TG_M; lr += TG_WAVES) {
    const int r = row0 + lr;
    if (r >= p.m_bound) break;
    const bf16_t* sh = ot + (size_t)lr * so;
    bf16_t* o = p.out + (long long)r * p.out_stride;
    if (pair_ok) for (int c = lane * 2; c < N; c += 128) *reinterpret_cast<uint32_t*>(o + c) = *reinterpret_cast<const uint32_t*>(sh + c);
    else for (int c = lane; c < N; c += 64) o[c] = sh[c];
  }
  if (p.out_norm) rows_norm(ot, so, N, row0, M, p.m_bound, p.out_norm, wave, lane);
}

// dropout stream: the last workgroup of the launch bumps the device-resident launch counter (everybody has read it)
__device__ __forceinline__ void bump_drop_counter(const TileGemm& p0, const TileGemm& p1, int n_sets) {
  unsigned long long* ctr = p0.drop_thresh ? p0.ctr : (n_sets > 1 && p1.drop_thresh ? p1.ctr : nullptr);
  if (ctr) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
      if (atomicAdd(ctr + 1, 1ull) == total - 1) {
        __hip_atomic_store(ctr + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(ctr, 1ull);
      }
    }
  }
}

// (waves_per_eu(4): two workgroups per CU is what the 330-workgroup input layer needs to run in one round, so the register
// allocator is held to the 128 VGPRs of that occupancy step instead of drifting one past it; it does so without scratch)
__global__ void __launch_bounds__(TG_TPB) __attribute__((amdgpu_waves_per_eu(4))) k_tile_gemm(TileGemm p0, TileGemm p1, int n_sets, int dbg) {
  extern __shared__ __attribute__((aligned(16))) bf16_t tg_lds[];
  __shared__ int row_id[2 * TG_M];
  if (dbg & 8) return;
  tile_gemm_body<false>(blockIdx.y == 0 ? p0 : p1, tg_lds, row_id, dbg);
  bump_drop_counter(p0, p1, n_sets);
}

// (the wide body reads its arguments inside the panel loops: a set chosen field by field stays in scalar registers, where a
// reference chosen by blockIdx.y put both sets into scratch memory)
__device__ __forceinline__ TileGemm pick_set(const TileGemm& a, const TileGemm& b, bool first) {
  TileGemm p;
#define TG_PICK(f) p.f = first ? a.f : b.f
  TG_PICK(a1); TG_PICK(a1_stride); TG_PICK(ids); TG_PICK(w1); TG_PICK(w1_stride); TG_PICK(k1);
  TG_PICK(a2); TG_PICK(a2_stride); TG_PICK(w2); TG_PICK(w2_stride); TG_PICK(k2); TG_PICK(bias);
  TG_PICK(m_bound); TG_PICK(m_dev); TG_PICK(n); TG_PICK(out); TG_PICK(out_stride); TG_PICK(a_copy); TG_PICK(copy_stride);
  TG_PICK(in_norm); TG_PICK(out_norm); TG_PICK(relu); TG_PICK(drop_thresh); TG_PICK(drop_scale); TG_PICK(seed); TG_PICK(ctr);
#undef TG_PICK
  return p;
}

__global__ void __launch_bounds__(TG_TPB) k_tile_gemm_wide(TileGemm p0, TileGemm p1, int n_sets) {
  extern __shared__ __attribute__((aligned(16))) bf16_t tg_lds[];
  __shared__ int row_id[2 * TG_M];
  tile_gemm_body<true>(pick_set(p0, p1, blockIdx.y == 0), tg_lds, row_id, 0);
  bump_drop_counter(p0, p1, n_sets);
}

bool convert(const bliss_tile_gemm_t* a, TileGemm* p, size_t* lds_bytes, int* tiles, bool wide) {
  const int k_max = wide ? BLISS_WIDE_MAX_K : 1024;
  if (!a->a1 || !a->w1 || !a->out || a->k1 <= 0 || a->k1 > k_max || a->n <= 0 || a->n > 256 || a->m_bound <= 0) return false;
  if (a->k2 < 0 || a->k2 > k_max || (a->k2 > 0 && (!a->a2 || !a->w2))) return false;
  if (a->drop_p < 0.f || a->drop_p >= 1.f || (a->drop_p > 0.f && !a->drop_ctr)) return false;
  p->a1 = (const bf16_t*)a->a1; p->a1_stride = a->a1_stride; p->ids = a->ids;
  p->w1 = (const bf16_t*)a->w1; p->w1_stride = a->w1_stride; p->k1 = a->k1;
  p->a2 = (const bf16_t*)a->a2; p->a2_stride = a->a2_stride; p->w2 = (const bf16_t*)a->w2; p->w2_stride = a->w2_stride; p->k2 = a->k2;
  p->bias = (const bf16_t*)a->bias; p->m_bound = a->m_bound; p->m_dev = a->m_dev; p->n = a->n;
  p->out = (bf16_t*)a->out; p->out_stride = a->out_stride; p->a_copy = (bf16_t*)a->a_copy; p->copy_stride = a->copy_stride;
  p->in_norm = (bf16_t*)a->in_norm; p->out_norm = (bf16_t*)a->out_norm; p->relu = a->relu;
  p->drop_thresh = a->drop_p > 0.f ? (unsigned)((double)a->drop_p * 4294967296.0) : 0u;
  p->drop_scale = a->drop_p > 0.f ? 1.0f / (1.0f - a->drop_p) : 1.0f;
  p->seed = a->drop_seed; p->ctr = (unsigned long long*)a->drop_ctr;
  const int k_wide = a->k1 > a->k2 ? a->k1 : a->k2;       // wide: one panel of the wider operand at a time
  const size_t rows = wide ? (size_t)lds_stride(k_wide < TG_PANEL ? k_wide : TG_PANEL) : (size_t)lds_stride(a->k1) + (a->k2 ? lds_stride(a->k2) : 0);
  const size_t stage = ((size_t)TG_M * rows + (size_t)TG_WROWS * TG_WSTRIDE) * sizeof(bf16_t);
  const size_t outt = (size_t)TG_M * (((a->n + 63) & ~63) + 8) * sizeof(bf16_t);
  *lds_bytes = stage > outt ? stage : outt;
  *tiles = (a->m_bound + TG_M - 1) / TG_M;
  return true;
}

template <typename Kernel, typename... Dbg>
int tile_gemm_launch(Kernel kernel, size_t* lds_set, bool wide, const bliss_tile_gemm_t* first, const bliss_tile_gemm_t* second, void* stream, Dbg... dbg) {
  if (!first) return BLISS_EINVAL;
  TileGemm p0, p1;
  size_t l0 = 0, l1 = 0;
  int t0 = 0, t1 = 0;
  if (!convert(first, &p0, &l0, &t0, wide)) return BLISS_EINVAL;
  p1 = p0;
  if (second && !convert(second, &p1, &l1, &t1, wide)) return BLISS_EINVAL;
  const size_t lds = l0 > l1 ? l0 : l1;
  if (lds > 160 * 1024) return BLISS_EINVAL;
  if (lds > *lds_set) {
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return BLISS_EINVAL;
    *lds_set = lds;
  }
  const dim3 grid(t0 > t1 ? t0 : t1, second ? 2 : 1);
  kernel<<<grid, TG_TPB, lds, (hipStream_t)stream>>>(p0, p1, second ? 2 : 1, dbg...);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int bliss_tile_gemm(const bliss_tile_gemm_t* first, const bliss_tile_gemm_t* second, void* stream) {
  static size_t lds_set = 0;
  static const int dbg = []() { const char* e = getenv("BLISS_TG_DEBUG"); return e ? atoi(e) : 0; }();
  return tile_gemm_launch(k_tile_gemm, &lds_set, false, first, second, stream, dbg);
}

// The same walk with K in panels (tile_gemm_body<true>): k1, k2 <= BLISS_WIDE_MAX_K, one panel in LDS at any K.
extern "C" int bliss_tile_gemm_wide(const bliss_tile_gemm_t* first, const bliss_tile_gemm_t* second, void* stream) {
  static size_t lds_set = 0;
  return tile_gemm_launch(k_tile_gemm_wide, &lds_set, true, first, second, stream);
}
