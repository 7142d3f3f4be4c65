// Recurrent neighbour aggregation for SAGEConv('lstm'), gfx950: an LSTM cell run over every destination's
// in-edges in the block's row order, forward and backward, and the by-source reduction of the gate gradients.
//
// [DGL-recalled] dglnn.SAGEConv(in, out, 'lstm') hands each destination's mailbox to nn.LSTM(D, D, batch_first=True) and keeps the
// last hidden state.  The input projection is factored out of the recurrence: W_ih (w_e h[s]) = w_e (W_ih h[s]), so the caller
// computes P = bf16(h @ W_ih^T) [n_src, 4 D] once per SOURCE row and the kernels take P.  For destination d with live in-edges
// e_0 .. e_{L-1} (ascending position in indptr), gate order i, f, g, o (column k D + u of P, row k D + u of W_hh):
//   pre_k[u] = ((float(w_e) * float(P[src_e, k D + u])) + (float(b_ih[k D + u]) + float(b_hh[k D + u]))) + sum_j bf16(h_{t-1})[j] W_hh[k D + u, j]
//   i, f, o  = 1 / (1 + exp(-pre))      g = tanh(pre_g)         fp32
//   c_t      = f c_{t-1} + i g          h_t = o tanh(c_t)       fp32; h_t is rounded to bf16 where it becomes the next operand
//   neigh[d] = bf16(h_{L-1});  a destination without live in-edges, and every row at or past the live destination count, gets +0
// The last term runs on v_mfma_f32_32x32x16_bf16 with fp32 accumulation from +0 in ascending j (16 per instruction), and is added
// LAST.  c and the gates never leave fp32.  Never contracted (-ffp-contract=off); no float atomics: two runs give the same bits.
//
// Launch shape.  A workgroup (8 waves) owns LS_T = 32 consecutive destination rows and walks t = 0 .. (the tile's largest degree)
// - 1; a row whose degree is at or below t is frozen (its h and c stay, nothing is read or written for it): no sort by degree, no
// host read.  Wave v owns hidden units 32 v .. 32 v + 31 -- D <= 256 is eight waves -- and keeps FOUR accumulator tiles, one per
// gate: the B operand of gate k is rows k D + 32 v .. of W_hh, K-contiguous as nn.LSTM stores them, so the four gates of hidden
// unit u arrive in the same lane (column = lane & 31, the tile's 32 destination rows in the 16 registers x 2 lane halves) and the
// cell update needs no exchange.  The tile's h lives in LDS as the bf16 A operand ([32][Dk + 8], 16-byte fragment reads); W_hh
// (8 D^2 bytes, 512 KB at D = 256) does not fit LDS and is streamed from L2 every step, 16-byte loads, two k-steps at a time so
// that eight fragment loads leave together.  The per-edge loads of a step (src, w, four P values per row) are issued in front
// of the products and used behind them.  D is padded to the granule (units to 32, K to 16) with zero fragments: a padded hidden
// unit stays exactly 0 and is never stored.  Two barriers per step (operand read / operand replaced).
//
// Training also saves, per live edge: the four gate activations and c_t in fp32 and bf16(h_{t-1}) (+0 at a row's first edge):
// 16 D + 4 D + 2 D = 22 D bytes per edge.  hprev[live, nnz) is written as +0 (a dense product reads it); the fp32 state past the
// live count is left unwritten and is never read.
//
// Backward (k_lstm_agg_bwd): the same tiles, t descending, d h and d c carried in fp32 in the accumulator layout.  Per step
//   dh = carry + (t == L - 1 ? float(gout[d]) : 0);  tc = tanh(c_t);  dc = dc + (dh * o) * (1 - tc * tc)
//   dG_i = bf16((dc * g) * (i * (1 - i)))   dG_f = bf16((dc * c_{t-1}) * (f * (1 - f)))
//   dG_g = bf16((dc * i) * (1 - g * g))     dG_o = bf16((dh * tc) * (o * (1 - o)))        dc <- dc * f
// dG[e] (bf16 [nnz, 4 D]) is stored and also laid into LDS as the A operand of  carry = dG_t . W_hh  (K = 4 D, the B operand
// read from W_hh^T [D, 4 D], K-contiguous).  dG[live, nnz) is written as +0.
// k_lstm_edge_reduce: dP[s] = bf16(sum over the out-edges e of s, ascending in the by-source index, float(w_e) * float(dG[e])),
// one wave per source row, fp32 from +0.
#include "common.cuh"
#include "bliss_gnn.h"
#include "prof.h"

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#define LS_T 32                                             // destination rows of a tile (bliss_lstm_tile_rows)
#define LS_TPB 512                                          // 8 waves x 32 hidden units
#define LS_MAX_D 256
#define LS_HS (LS_MAX_D + 8)                                // the forward's LDS row stride at the largest D (elements)

struct LstmFwd {
  const int* indptr; const int* src; const bf16_t* w; const bf16_t* p; int64_t p_stride;
  const bf16_t* whh; int64_t whh_stride; const bf16_t* b_ih; const bf16_t* b_hh;
  int n_dst; const int* n_dst_dev; const int* nnz_dev; int nnz; int dim;
  bf16_t* out; int64_t out_stride; float* gates; float* cell; bf16_t* hprev;
};

struct LstmBwd {
  const int* indptr; const bf16_t* gout; int64_t gout_stride; const bf16_t* wt; int64_t wt_stride;
  const float* gates; const float* cell;
  int n_dst; const int* n_dst_dev; const int* nnz_dev; int nnz; int dim;
  bf16_t* dgate;
};

struct LstmRed {
  const int* t_indptr; const int* t_edge; const bf16_t* w; const bf16_t* dgate; int n_src; const int* nnz_dev; int nnz; int dim;
  bf16_t* dp; int64_t dp_stride;
};

__device__ __forceinline__ int live_count(const int* dev, int host) {
  int n = host;
  if (dev) { const int t = *dev; n = t < n ? t : n; }
  return n < 0 ? 0 : n;
}

// 8 consecutive elements row[k0 .. k0 + 7] as an MFMA fragment; zero where !row_ok or at and past column K.  VEC: one 16-byte
// load, unconditional (a fragment that does not exist re-reads `safe`, the matrix's first row, and is discarded).
template <bool VEC>
__device__ __forceinline__ bf16x8_t load_frag(const bf16_t* row, int k0, int K, bool row_ok, const bf16_t* safe) {
  union { uint4 u; bf16_t e[8]; bf16x8_t v; } t;
  if (VEC) {
    const bool ok = row_ok && k0 < K;
    const uint4 v = *reinterpret_cast<const uint4*>(ok ? row + k0 : safe);
    t.u = ok ? v : make_uint4(0, 0, 0, 0);
  } else {
    t.u = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) if (row_ok && k0 + j < K) t.e[j] = row[k0 + j];
  }
  return t.v;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }

// the tile's rows: first live edge and live degree of each into LDS, the largest degree returned (workgroup-uniform)
__device__ __forceinline__ int tile_rows(const int* __restrict__ indptr, int row0, int live_dst, int live, int* s_beg, int* s_deg) {
  if (threadIdx.x < LS_T) {
    const int r = row0 + (int)threadIdx.x;
    int b = 0, d = 0;
    if (r < live_dst) {
      b = min(indptr[r], live);
      d = min(indptr[(int64_t)r + 1], live) - b;
      d = d > 0 ? d : 0;
    }
    s_beg[threadIdx.x] = b; s_deg[threadIdx.x] = d;
  }
  __syncthreads();
  int md = 0;
#pragma unroll
  for (int i = 0; i < LS_T; ++i) md = max(md, s_deg[i]);
  return md;
}

template <bool VEC>
__global__ void __launch_bounds__(LS_TPB) k_lstm_agg_fwd(LstmFwd p) {
  __shared__ __attribute__((aligned(16))) bf16_t s_h[LS_T * LS_HS];
  __shared__ int s_beg[LS_T], s_deg[LS_T];
  const int D = p.dim, Dk = (D + 15) & ~15, HS = Dk + 8, KS = Dk >> 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int u = wave * 32 + r;
  const bool u_ok = u < D;
  const int live = live_count(p.nnz_dev, p.nnz), live_dst = live_count(p.n_dst_dev, p.n_dst);
  const int row0 = blockIdx.x * LS_T;
  if (p.hprev) {                                            // +0 for the edges past the live count
    const int64_t n = (int64_t)(p.nnz - live) * D, base = (int64_t)live * D;
    for (int64_t i = (int64_t)blockIdx.x * LS_TPB + tid; i < n; i += (int64_t)gridDim.x * LS_TPB) p.hprev[base + i] = 0;
  }
  if (row0 >= p.n_dst) return;                              // (the one workgroup of a block without rows)
  for (int i = tid; i < LS_T * HS; i += LS_TPB) s_h[i] = 0;
  const int maxdeg = tile_rows(p.indptr, row0, live_dst, live, s_beg, s_deg);     // (its barrier covers the clear of s_h)

  float bsum[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float bi = (p.b_ih && u_ok) ? bf2f(p.b_ih[g * D + u]) : 0.f, bh = (p.b_hh && u_ok) ? bf2f(p.b_hh[g * D + u]) : 0.f;
    bsum[g] = bi + bh;
  }
  float c[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) c[q] = 0.f;

  for (int t = 0; t < maxdeg; ++t) {
    // this step's edge operands, issued in front of the products
    float wv[16];
    uint32_t pv[2][16];                                     // P of gates (i, f) and (g, o), packed pairs
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
      wv[q] = 1.0f;
      pv[0][q] = pv[1][q] = 0u;
      if (u_ok && t < s_deg[row]) {
        const int64_t e = (int64_t)s_beg[row] + t;
        const int s = p.src[e];
        if (p.w) wv[q] = bf2f(p.w[e]);
        const bf16_t* pr = p.p + (int64_t)s * p.p_stride + u;
        pv[0][q] = (uint32_t)pr[0] | ((uint32_t)pr[D] << 16);
        pv[1][q] = (uint32_t)pr[2 * D] | ((uint32_t)pr[3 * D] << 16);
      }
    }
    // bf16(h_{t-1}) . W_hh^T for this wave's 32 units, the four gates side by side
    f32x16_t acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[g][q] = 0.f;
    if (wave * 32 < D && t > 0) {                           // (h_{-1} = 0: the first step's product is +0)
      // two k-steps at a time: their eight fragment loads leave together, in front of the eight products
      auto frags = [&](int ks, bf16x8_t& a, bf16x8_t (&b)[4]) {
        const int k0 = 16 * ks + 8 * hh;
        a = *reinterpret_cast<const bf16x8_t*>(s_h + r * HS + k0);
#pragma unroll
        for (int g = 0; g < 4; ++g) b[g] = load_frag<VEC>(p.whh + (int64_t)(g * D + u) * p.whh_stride, k0, D, u_ok, p.whh);
      };
      int ks = 0;
      for (; ks + 1 < KS; ks += 2) {
        bf16x8_t a0, a1, b0[4], b1[4];
        frags(ks, a0, b0);
        frags(ks + 1, a1, b1);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0[g], acc[g], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[g], acc[g], 0, 0, 0);
      }
      if (ks < KS) {
        bf16x8_t a0, b0[4];
        frags(ks, a0, b0);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0[g], acc[g], 0, 0, 0);
      }
    }
    // the cell update, in the accumulator layout: register q of lane half hh is row (q & 3) + 8 (q >> 2) + 4 hh, column u
    bf16_t hn[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
      hn[q] = 0;
      if (u_ok && t < s_deg[row]) {
        const int64_t e = (int64_t)s_beg[row] + t;
        const float gi = sigmoid_f(((wv[q] * __uint_as_float(pv[0][q] << 16)) + bsum[0]) + acc[0][q]);
        const float gf = sigmoid_f(((wv[q] * __uint_as_float(pv[0][q] & 0xffff0000u)) + bsum[1]) + acc[1][q]);
        const float gg = tanhf(((wv[q] * __uint_as_float(pv[1][q] << 16)) + bsum[2]) + acc[2][q]);
        const float go = sigmoid_f(((wv[q] * __uint_as_float(pv[1][q] & 0xffff0000u)) + bsum[3]) + acc[3][q]);
        const float cn = gf * c[q] + gi * gg;
        c[q] = cn;
        hn[q] = f2bf(go * tanhf(cn));
        if (p.hprev) {
          float* gs = p.gates + e * 4 * D + u;
          gs[0] = gi; gs[D] = gf; gs[2 * D] = gg; gs[3 * D] = go;
          p.cell[e * D + u] = cn;
          p.hprev[e * D + u] = s_h[row * HS + u];
        }
      }
    }
    __syncthreads();                                        // every wave has read the operand h_{t-1}
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
      if (u_ok && t < s_deg[row]) s_h[row * HS + u] = hn[q];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
    const int gr = row0 + row;
    if (u_ok && gr < p.n_dst) p.out[(int64_t)gr * p.out_stride + u] = s_h[row * HS + u];
  }
}

template <bool VEC>
__global__ void __launch_bounds__(LS_TPB) k_lstm_agg_bwd(LstmBwd p) {
  extern __shared__ __attribute__((aligned(16))) bf16_t s_g[];                 // dG of the step: [LS_T][4 Dk + 8]
  __shared__ int s_beg[LS_T], s_deg[LS_T];
  const int D = p.dim, Dk = (D + 15) & ~15, GS = 4 * Dk + 8, KS = Dk >> 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int u = wave * 32 + r;
  const bool u_ok = u < D;
  const int live = live_count(p.nnz_dev, p.nnz), live_dst = live_count(p.n_dst_dev, p.n_dst);
  const int row0 = blockIdx.x * LS_T;
  {                                                         // +0 for the edges past the live count
    const int64_t n = (int64_t)(p.nnz - live) * 4 * D, base = (int64_t)live * 4 * D;
    for (int64_t i = (int64_t)blockIdx.x * LS_TPB + tid; i < n; i += (int64_t)gridDim.x * LS_TPB) p.dgate[base + i] = 0;
  }
  if (row0 >= p.n_dst) return;
  for (int i = tid; i < LS_T * GS; i += LS_TPB) s_g[i] = 0;
  const int maxdeg = tile_rows(p.indptr, row0, live_dst, live, s_beg, s_deg);

  float dhc[16], dc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) { dhc[q] = 0.f; dc[q] = 0.f; }

  for (int t = maxdeg - 1; t >= 0; --t) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
      const int dg = s_deg[row];
      bf16_t o4[4] = {0, 0, 0, 0};
      if (u_ok && t < dg) {
        const int64_t e = (int64_t)s_beg[row] + t;
        const float* gs = p.gates + e * 4 * D + u;
        const float gi = gs[0], gf = gs[D], gg = gs[2 * D], go = gs[3 * D];
        const float ct = p.cell[e * D + u];
        const float cp = t > 0 ? p.cell[(e - 1) * D + u] : 0.f;
        float dh = dhc[q];
        if (t == dg - 1) dh = dh + bf2f(p.gout[(int64_t)(row0 + row) * p.gout_stride + u]);
        const float tc = tanhf(ct);
        const float dct = dc[q] + (dh * go) * (1.0f - tc * tc);
        o4[0] = f2bf((dct * gg) * (gi * (1.0f - gi)));
        o4[1] = f2bf((dct * cp) * (gf * (1.0f - gf)));
        o4[2] = f2bf((dct * gi) * (1.0f - gg * gg));
        o4[3] = f2bf((dh * tc) * (go * (1.0f - go)));
        dc[q] = dct * gf;
        bf16_t* ge = p.dgate + e * 4 * D + u;
        ge[0] = o4[0]; ge[D] = o4[1]; ge[2 * D] = o4[2]; ge[3 * D] = o4[3];
      }
      if (u < Dk) {
#pragma unroll
        for (int g = 0; g < 4; ++g) s_g[row * GS + g * Dk + u] = o4[g];
      }
    }
    __syncthreads();
    // carry = dG_t . W_hh for this wave's 32 units: K = the 4 Dk padded gate columns, B from W_hh^T [D, 4 D]
    f32x16_t acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    if (wave * 32 < D && t > 0) {                           // (the carry out of step 0 is not used: h_{-1} is a constant)
      // the 4 Dk / 16 k-steps in ascending order, four at a time: their fragment loads leave together
      auto frag = [&](int kk, bf16x8_t& a, bf16x8_t& b) {
        const int g = kk / KS, k0 = 16 * (kk - g * KS) + 8 * hh;
        a = *reinterpret_cast<const bf16x8_t*>(s_g + r * GS + g * Dk + k0);
        b = load_frag<VEC>(p.wt + (int64_t)u * p.wt_stride + g * D, k0, D, u_ok, p.wt);
      };
      int kk = 0;
      for (; kk + 3 < 4 * KS; kk += 4) {
        bf16x8_t a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) frag(kk + j, a[j], b[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[j], b[j], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) dhc[q] = acc[q];
    __syncthreads();                                        // the operand has been read: the next step may replace it
  }
}

// dP[s, :] over 4 D columns: a wave per source row, a lane one column of each 64-column group, four groups at a time
__global__ void __launch_bounds__(256) k_lstm_edge_reduce(LstmRed p) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= p.n_src) return;
  const int live = live_count(p.nnz_dev, p.nnz), lane = lane_id(), W = 4 * p.dim;
  const int kb = p.t_indptr[s], ke = min(p.t_indptr[(int64_t)s + 1], live);
  for (int c0 = 0; c0 < W; c0 += 256) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = kb; k < ke; ++k) {
      const int e = p.t_edge[k];
      const float we = p.w ? bf2f(p.w[e]) : 1.0f;
      const bf16_t* ge = p.dgate + (int64_t)e * W;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = c0 + 64 * j + lane;
        if (col < W) acc[j] += we * bf2f(ge[col]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + 64 * j + lane;
      if (col < W) p.dp[(int64_t)s * p.dp_stride + col] = f2bf(acc[j]);
    }
  }
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p) % a == 0; }

}  // namespace

extern "C" {

int bliss_lstm_tile_rows(void) { return LS_T; }

int bliss_lstm_agg_fwd(const int32_t* indptr, const int32_t* src, const void* w, const void* p, int64_t p_stride, const void* w_hh,
                       int64_t w_hh_stride, const void* b_ih, const void* b_hh, int32_t n_dst, const int32_t* n_dst_dev,
                       const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* out, int64_t out_stride, float* gates, float* cell,
                       void* hprev, void* stream) {
  if (!indptr || !w_hh || !out || n_dst < 0 || nnz < 0 || dim < 1 || dim > LS_MAX_D || (nnz > 0 && (!src || !p))) return BLISS_EINVAL;
  if (p_stride < 4 * (int64_t)dim || w_hh_stride < dim || out_stride < dim) return BLISS_EINVAL;
  const int saved = (gates != nullptr) + (cell != nullptr) + (hprev != nullptr);
  if (saved != 0 && saved != 3) return BLISS_EINVAL;        // the backward's state: all three or none
  const int tiles = (n_dst + LS_T - 1) / LS_T, grid = tiles > 0 ? tiles : (nnz > 0 && hprev ? 1 : 0);
  if (grid == 0) return 0;
  LstmFwd a = {indptr, src, (const bf16_t*)w, (const bf16_t*)p, p_stride, (const bf16_t*)w_hh, w_hh_stride, (const bf16_t*)b_ih,
               (const bf16_t*)b_hh, n_dst, n_dst_dev, nnz_dev, nnz, dim, (bf16_t*)out, out_stride, gates, cell, (bf16_t*)hprev};
  hipStream_t st = (hipStream_t)stream;
  if (dim % 8 == 0 && w_hh_stride % 8 == 0 && al(w_hh, 16)) PROF_LAUNCH(BK_LSTM_AGG_FWD, st, k_lstm_agg_fwd<true><<<grid, LS_TPB, 0, st>>>(a));
  else PROF_LAUNCH(BK_LSTM_AGG_FWD, st, k_lstm_agg_fwd<false><<<grid, LS_TPB, 0, st>>>(a));
  return (int)hipGetLastError();
}

int bliss_lstm_agg_bwd(const int32_t* indptr, const void* gout, int64_t gout_stride, const void* w_hh_t, int64_t w_hh_t_stride,
                       const float* gates, const float* cell, int32_t n_dst, const int32_t* n_dst_dev, const int32_t* nnz_dev,
                       int32_t nnz, int32_t dim, void* dgate, void* stream) {
  if (!indptr || !gout || !w_hh_t || n_dst < 0 || nnz < 0 || dim < 1 || dim > LS_MAX_D || (nnz > 0 && (!gates || !cell || !dgate)))
    return BLISS_EINVAL;
  if (gout_stride < dim || w_hh_t_stride < 4 * (int64_t)dim) return BLISS_EINVAL;
  const int tiles = (n_dst + LS_T - 1) / LS_T, grid = tiles > 0 ? tiles : (nnz > 0 ? 1 : 0);
  if (grid == 0 || nnz == 0) return 0;                      // no edge: no gate gradient to write
  LstmBwd a = {indptr, (const bf16_t*)gout, gout_stride, (const bf16_t*)w_hh_t, w_hh_t_stride, gates, cell, n_dst, n_dst_dev, nnz_dev,
               nnz, dim, (bf16_t*)dgate};
  const int Dk = (dim + 15) & ~15;
  const size_t lds = (size_t)LS_T * (4 * Dk + 8) * sizeof(bf16_t);
  const bool vec = dim % 8 == 0 && w_hh_t_stride % 8 == 0 && al(w_hh_t, 16);
  static size_t lds_set[2] = {0, 0};
  if (lds > lds_set[vec]) {
    const void* fn = vec ? (const void*)k_lstm_agg_bwd<true> : (const void*)k_lstm_agg_bwd<false>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return BLISS_EINVAL;
    lds_set[vec] = lds;
  }
  hipStream_t st = (hipStream_t)stream;
  if (vec) PROF_LAUNCH(BK_LSTM_AGG_BWD, st, k_lstm_agg_bwd<true><<<grid, LS_TPB, lds, st>>>(a));
  else PROF_LAUNCH(BK_LSTM_AGG_BWD, st, k_lstm_agg_bwd<false><<<grid, LS_TPB, lds, st>>>(a));
  return (int)hipGetLastError();
}

int bliss_lstm_edge_reduce(const int32_t* t_indptr, const int32_t* t_edge, const void* w, const void* dgate, int32_t n_src,
                           const int32_t* nnz_dev, int32_t nnz, int32_t dim, void* dp, int64_t dp_stride, void* stream) {
  if (!t_indptr || !dp || n_src < 0 || nnz < 0 || dim < 1 || dim > LS_MAX_D || (nnz > 0 && (!t_edge || !dgate))) return BLISS_EINVAL;
  if (dp_stride < 4 * (int64_t)dim) return BLISS_EINVAL;
  if (n_src == 0) return 0;
  LstmRed a = {t_indptr, t_edge, (const bf16_t*)w, (const bf16_t*)dgate, n_src, nnz_dev, nnz, dim, (bf16_t*)dp, dp_stride};
  hipStream_t st = (hipStream_t)stream;
  PROF_LAUNCH(BK_LSTM_EDGE_REDUCE, st, k_lstm_edge_reduce<<<(n_src + 3) / 4, 256, 0, st>>>(a));
  return (int)hipGetLastError();
}

}  // extern "C"
