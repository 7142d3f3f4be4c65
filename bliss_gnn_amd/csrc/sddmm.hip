// Per-edge dot product of two gathered rows (an SDDMM on the block's edge list), gfx950: the gradient of
// the aggregation ops w.r.t. their per-edge weights, and fn.u_dot_v.
//
// For live edge e with s = src[e], d = dst[e]:
//   dot_e  = sum_c float(a[d, c]) * float(b[s, c])                 (BLISS_SDDMM_MAX: only the columns c with arg[d, c] == e)
//   out[e] = round(dot_e * coef_e)                                  ONE rounding, to bf16, or none with out_fp32
//   coef_e = 1                               BLISS_SDDMM_SUM, BLISS_SDDMM_MAX
//            1.0f / (float)max(deg_d, 1)     BLISS_SDDMM_MEAN       deg_d = indptr[d + 1] - indptr[d]
//            1.0f / (float)(deg_d + 1)       BLISS_SDDMM_SELF
// The live edge count is nnz_dev ? min(*nnz_dev, nnz) : nnz; entries [live, nnz) are written as +0 and nothing (no endpoint,
// no row, no degree, no arg entry) is read for an edge at or past it.
//
// Sum order (fixed, the same in all three load forms, so the bits do not depend on an operand's alignment):
//   * the columns are cut into groups of 8 consecutive ones; group g belongs to lane g % 16 of the edge's 16-lane row;
//   * a lane starts from +0 and adds its products one by one in ascending column order (group g, then g + 16, ...); a column
//     masked out in MAX mode adds +0;
//   * the 16 lane sums p_0 .. p_15 are added as a balanced binary tree of neighbours, four DPP row_shr steps (1, 2, 4, 8):
//       (((p15 + p14) + (p13 + p12)) + ((p11 + p10) + (p9 + p8))) + (((p7 + p6) + (p5 + p4)) + ((p3 + p2) + (p1 + p0)))
//   * the total is multiplied by coef_e (fp32) and rounded once.
// Products and sums are fp32, never contracted (-ffp-contract=off).  No float atomics: two runs give the same bits.
//
// Launch shape: 256-thread workgroups; a wave owns spmm_chunk_edges(nnz) consecutive edges, whose (src, dst) pairs and
// coefficients its lanes fetch once, coalesced.  It then works on FOUR edges at a time, one per 16-lane row: a lane loads 8
// consecutive bf16 columns of the a row and of the b row with one 16-byte load each, so one step covers 128 columns of four
// edges (8 row pieces) and a 256-wide row takes two steps.  The loads of four steps -- two quads of a 256-wide row, four
// quads up to 128 columns -- are issued together, before the first of them is multiplied and reduced: 32 row pieces in flight
// per wave, at least 16 of them belonging to the quads behind the one being reduced.  The per-edge
// reduction stays inside the row on the DPP path: no LDS, no ds_bpermute.  Consecutive edges of one destination re-read its a row
// from L1 / L2.  Where the 16-byte form does not apply (a base or row stride that is not 16-byte aligned, dim % 8 != 0) the 8
// columns come from two 8-byte loads, else from 8 scalar loads: a column-sliced view works.  No load sits behind a branch: a lane
// without an edge or past the last column reads a clamped address of a live edge's row and discards the value.
#include "common.cuh"
#include "spmm_walk.cuh"
#include "bliss_gnn.h"
#include "prof.h"

namespace {

using spmm_walk::bcast_f;
using spmm_walk::bcast_i;
using spmm_walk::spmm_chunk_edges;

#define SD_TPB 256
#define SD_COLS 128                                         // columns of one step: 16 lanes x 8
#define SD_BATCH 4                                          // steps whose loads are issued together

struct SdArgs {
  const int* src; const int* dst; const int* indptr; const int* nnz_dev; int nnz;
  const bf16_t* a; int64_t a_stride;
  const bf16_t* b; int64_t b_stride;
  const int* arg; int64_t arg_stride;
  int dim, mode;
  void* out; int out_fp32;
  int EC;
};

// the operands of one step of one lane: 8 columns of the a row and of the b row as packed bf16 pairs, (MAX) their winners
template <bool MAX>
struct Item {
  uint32_t a[4], b[4];
  int m[8];                                                 // (unused, and so not allocated, outside MAX mode)
};

// 8 columns of row `p` from column `col` into packed pairs.  The addresses are clamped, never guarded: a column at or past dim
// re-reads one of the row's first columns (dim >= 1) and the caller discards it, so no load sits behind a branch and a
// batch's loads stay in flight together.
template <int FORM>
__device__ __forceinline__ void load8(const bf16_t* p, int col, int dim, uint32_t (&r)[4]) {
  if (FORM == 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(p + (col < dim ? col : 0));
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  } else if (FORM == 4) {
    const int ca = col < dim ? col : 0, cb = col + 4 < dim ? col + 4 : 0;
    const uint2 v = *reinterpret_cast<const uint2*>(p + ca), u = *reinterpret_cast<const uint2*>(p + cb);
    r[0] = v.x; r[1] = v.y; r[2] = u.x; r[3] = u.y;
  } else {
    uint32_t x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = p[col + k < dim ? col + k : 0];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = x[2 * k] | (x[2 * k + 1] << 16);
  }
}
template <int FORM>
__device__ __forceinline__ void load8_arg(const int* p, int col, int dim, int (&m)[8]) {
  if (FORM == 8) {
    const int c = col < dim ? col : 0;
    const int4 u = *reinterpret_cast<const int4*>(p + c), v = *reinterpret_cast<const int4*>(p + c + 4);
    m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = u.w; m[4] = v.x; m[5] = v.y; m[6] = v.z; m[7] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = p[col + k < dim ? col + k : 0];
  }
}

// the value of the wave-uniform entries v[j0 .. j0 + 3] (one per 16-lane row) in each row's lanes
__device__ __forceinline__ int row_pick_i(int v, int j0, int row) {
  const int x0 = bcast_i(v, j0), x1 = bcast_i(v, j0 + 1), x2 = bcast_i(v, j0 + 2), x3 = bcast_i(v, j0 + 3);
  int x = x0;
  x = row == 1 ? x1 : x;
  x = row == 2 ? x2 : x;
  x = row == 3 ? x3 : x;
  return x;
}
__device__ __forceinline__ float row_pick_f(float v, int j0, int row) { return __int_as_float(row_pick_i(__float_as_int(v), j0, row)); }

template <int CTRL>
__device__ __forceinline__ float row_shr_f(float v) { return __int_as_float(dpp_mov0<CTRL, 0xf>(__float_as_int(v))); }

template <int FORM, bool MAX>
__global__ void __launch_bounds__(SD_TPB) k_sddmm_dot(SdArgs p) {
  const int EC = p.EC, dim = p.dim;
  const int ci = blockIdx.x * (SD_TPB / 64) + (threadIdx.x >> 6);
  if ((int64_t)ci * EC >= p.nnz) return;
  int live = p.nnz;
  if (p.nnz_dev) { const int t = *p.nnz_dev; live = t < live ? t : live; }
  if (live < 0) live = 0;
  const int lane = lane_id(), row = lane >> 4, l16 = lane & 15;
  const int c0 = ci * EC;
  float* out32 = (float*)p.out;
  bf16_t* out16 = (bf16_t*)p.out;
  {                                                         // the +0 tail [live, nnz) of this wave's run
    const int64_t e = (int64_t)c0 + lane;
    if (lane < EC && e < p.nnz && e >= live) {
      if (p.out_fp32) out32[e] = 0.f; else out16[e] = 0;
    }
  }
  const int cnt = __builtin_amdgcn_readfirstlane(min(live, c0 + EC) - c0);       // live edges of the run (wave-uniform)
  if (cnt <= 0) return;
  // the run's endpoints and coefficients once, coalesced; lanes past the run repeat its last edge (a live one: whatever a
  // clamped address below reads belongs to a live edge)
  const int64_t me = (int64_t)c0 + min(lane, cnt - 1);
  const int my_s = p.src[me], my_d = p.dst[me];
  float my_c = 1.0f;
  if (p.mode == BLISS_SDDMM_MEAN || p.mode == BLISS_SDDMM_SELF) {
    const int deg = p.indptr[(int64_t)my_d + 1] - p.indptr[my_d];
    my_c = p.mode == BLISS_SDDMM_MEAN ? 1.0f / (float)max(deg, 1) : 1.0f / (float)(max(deg, 0) + 1);
  }
  const int P = (dim + SD_COLS - 1) / SD_COLS;              // steps per quad
  const int Q = (cnt + 3) >> 2;                             // quads of the run

  // step (q, pass): quad q = edges c0 + 4q .. 4q + 3 (one per row), columns [pass * 128, + 128).  A step past the run's last
  // one re-reads the last quad (wave-uniform clamp, the result unused): the loads are unconditional.
  auto fetch = [&](int q, int pass, Item<MAX>& it) {
    const int qq = q < Q ? q : Q - 1;
    const int col = pass * SD_COLS + l16 * 8;
    const int s = row_pick_i(my_s, 4 * qq, row), d = row_pick_i(my_d, 4 * qq, row);
    load8<FORM>(p.a + (int64_t)d * p.a_stride, col, dim, it.a);
    load8<FORM>(p.b + (int64_t)s * p.b_stride, col, dim, it.b);
    if (MAX) load8_arg<FORM>(p.arg + (int64_t)d * p.arg_stride, col, dim, it.m);
  };
  auto advance = [&](int& q, int& pass) { if (++pass == P) { pass = 0; ++q; } };

  float acc = 0.f;
  // multiply and add step (q, pass) of `it`; behind a quad's last step: reduce its four rows and store
  auto compute = [&](int q, int pass, const Item<MAX>& it) {
    const int j = 4 * q + row, col = pass * SD_COLS + l16 * 8;
    const int e = c0 + j;
    const bool valid = j < cnt;
    if (pass == 0) acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t ua = it.a[k >> 1], ub = it.b[k >> 1];
      const float x = (k & 1) ? __uint_as_float(ua & 0xffff0000u) : __uint_as_float(ua << 16);
      const float y = (k & 1) ? __uint_as_float(ub & 0xffff0000u) : __uint_as_float(ub << 16);
      bool ok = valid && col + k < dim;
      if (MAX) ok = ok && it.m[MAX ? k : 0] == e;
      acc += ok ? x * y : 0.f;
    }
    if (pass == P - 1) {                                    // wave-uniform: every lane takes part in the row reduction
      float v = acc;
      v += row_shr_f<0x111>(v); v += row_shr_f<0x112>(v); v += row_shr_f<0x114>(v); v += row_shr_f<0x118>(v);
      v = v * row_pick_f(my_c, 4 * q, row);
      if (l16 == 15 && valid) {
        if (p.out_fp32) out32[(int64_t)e] = v; else out16[(int64_t)e] = f2bf(v);
      }
    }
  };

  // SD_BATCH steps at a time: all their loads leave together, then the steps are consumed oldest first, each behind a wait for
  // its own loads alone.  (Nothing is carried in registers from one batch to the next: a carried operand would be copied
  // while its load is pending, and the copy waits.)
  int fq = 0, fp = 0, q = 0, pass = 0;
  while (q < Q) {
    Item<MAX> it[SD_BATCH];
#pragma unroll
    for (int u = 0; u < SD_BATCH; ++u) { fetch(fq, fp, it[u]); advance(fq, fp); }
#pragma unroll
    for (int u = 0; u < SD_BATCH; ++u) {
      if (q < Q) { compute(q, pass, it[u]); advance(q, pass); }
    }
  }
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p) % a == 0; }

}  // namespace

extern "C" {

int bliss_sddmm_dot(const int32_t* src, const int32_t* dst, const int32_t* indptr, const int32_t* nnz_dev, int32_t nnz, const void* a,
                    int64_t a_stride, const void* b, int64_t b_stride, const int32_t* arg, int64_t arg_stride, int32_t dim, int32_t mode,
                    void* out, int32_t out_fp32, void* stream) {
  if (nnz < 0 || dim <= 0) return BLISS_EINVAL;
  if (mode != BLISS_SDDMM_SUM && mode != BLISS_SDDMM_MEAN && mode != BLISS_SDDMM_SELF && mode != BLISS_SDDMM_MAX) return BLISS_EINVAL;
  if (a_stride < dim || b_stride < dim) return BLISS_EINVAL;
  if ((mode == BLISS_SDDMM_MEAN || mode == BLISS_SDDMM_SELF) && !indptr) return BLISS_EINVAL;
  if (mode == BLISS_SDDMM_MAX && (!arg || arg_stride < dim)) return BLISS_EINVAL;
  if (nnz > 0 && (!src || !dst || !a || !b || !out)) return BLISS_EINVAL;
  if (nnz == 0) return 0;
  const bool is_max = mode == BLISS_SDDMM_MAX;
  const int EC = spmm_chunk_edges(nnz);
  SdArgs p = {src, dst, indptr, nnz_dev, nnz, (const bf16_t*)a, a_stride, (const bf16_t*)b, b_stride, is_max ? arg : nullptr,
              is_max ? arg_stride : 0, dim, mode, out, out_fp32 ? 1 : 0, EC};
  const bool v8 = dim % 8 == 0 && a_stride % 8 == 0 && b_stride % 8 == 0 && al(a, 16) && al(b, 16) &&
                  (!is_max || (arg_stride % 4 == 0 && al(arg, 16)));
  const bool v4 = dim % 4 == 0 && a_stride % 4 == 0 && b_stride % 4 == 0 && al(a, 8) && al(b, 8);
  const int nchunks = (nnz + EC - 1) / EC;
  const dim3 block(SD_TPB), grid((nchunks + SD_TPB / 64 - 1) / (SD_TPB / 64));
  hipStream_t st = (hipStream_t)stream;
  if (is_max) {
    if (v8) PROF_LAUNCH(BK_SDDMM_DOT, st, k_sddmm_dot<8, true><<<grid, block, 0, st>>>(p));
    else if (v4) PROF_LAUNCH(BK_SDDMM_DOT, st, k_sddmm_dot<4, true><<<grid, block, 0, st>>>(p));
    else PROF_LAUNCH(BK_SDDMM_DOT, st, k_sddmm_dot<1, true><<<grid, block, 0, st>>>(p));
  } else {
    if (v8) PROF_LAUNCH(BK_SDDMM_DOT, st, k_sddmm_dot<8, false><<<grid, block, 0, st>>>(p));
    else if (v4) PROF_LAUNCH(BK_SDDMM_DOT, st, k_sddmm_dot<4, false><<<grid, block, 0, st>>>(p));
    else PROF_LAUNCH(BK_SDDMM_DOT, st, k_sddmm_dot<1, false><<<grid, block, 0, st>>>(p));
  }
  return (int)hipGetLastError();
}

}  // extern "C"
