// Micro-F1 (torchmetrics Multiclass / MultilabelF1Score(average='micro'), train_lightning.py:68-70, updated per batch at :143
// and :179-203) as counts kept on the device: one launch per batch adds {tp, fp, fn, n} to four int64 words.  Nothing is read
// back, so the update sits inside a replayed train or validation step; the caller reads the four words once, when it wants
// the number.  The rule (normative; restated in include/bliss_gnn.h, DESIGN.md section 14 and tests/metrics_ref.py):
//
//   single-label  prediction = FIRST index of the row's largest logit; NaN is larger than everything and the first NaN wins
//                 (torch.argmax); +0 == -0; a row of -inf predicts 0.  Correct: tp += 1; wrong: fp += 1, fn += 1; n += 1 per
//                 counted row.  A label outside [0, n_cls) -- or an id outside a given table / prediction -- sets bit 2 of *err
//                 and the row is in none of the four counts.
//   multi-label   per (row, class) pair: hit = x > 0 (the exact statement of sigmoid(x) > 0.5), y = target > 0.5; NaN and +-0
//                 are no hit on either side; n += n_cls per counted row.
//
// The adds are 64-bit integer atomics, at most one per workgroup and counter: integer adds commute, so the four words do not
// depend on the launch's scheduling.  The kernels keep no state besides `counts` and `err`: there is no word to leave zero.
#include "common.cuh"
#include "bliss_gnn.h"

namespace {

#define F1_TPB 256
#define F1_ROWS_PER_WG (F1_TPB / 64)

// The tail of both kernels: per-thread counters -> wave totals (DPP) -> workgroup totals (LDS) -> one atomic per counter that
// is not zero.  Every thread of the workgroup calls it.
__device__ __forceinline__ void f1_commit(long long tp, long long fp, long long fn, long long n, long long* counts) {
  __shared__ long long part[F1_TPB / 64][4];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  tp = wave_total_i64(tp); fp = wave_total_i64(fp); fn = wave_total_i64(fn); n = wave_total_i64(n);
  if (lane == 0) { part[wave][0] = tp; part[wave][1] = fp; part[wave][2] = fn; part[wave][3] = n; }
  __syncthreads();
  if (threadIdx.x < 4) {
    long long t = 0;
    for (int w = 0; w < F1_TPB / 64; ++w) t += part[w][threadIdx.x];
    if (t) atomicAdd((unsigned long long*)counts + threadIdx.x, (unsigned long long)t);
  }
}

__device__ __forceinline__ int f1_valid_rows(int n_rows, const int* __restrict__ n_rows_dev) {
  if (!n_rows_dev) return n_rows;
  const int v = *n_rows_dev;
  return v < n_rows ? (v < 0 ? 0 : v) : n_rows;
}

// A logit as an unsigned key whose order is torch.argmax's: NaN (any payload, either sign) above +inf, -0 equal to +0.
__device__ __forceinline__ uint32_t f1_key(bf16_t b) {
  uint32_t u = ((uint32_t)b) << 16;
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One wave per row, lanes striding the classes (the shape of k_cross_entropy).  (key, index) pairs travel as one 64-bit word,
// key in the high half and ~index in the low half: the maximum of these words is the largest key at its LOWEST index.  Every
// real element's word is > 0 (the smallest key, -inf's, is 0x007fffff), so 0 stands for "no element".
__global__ void __launch_bounds__(F1_TPB) k_f1_multiclass(const bf16_t* __restrict__ logits, long long stride, int n_pred_rows,
                                                          const int* __restrict__ row_ids, const long long* __restrict__ labels,
                                                          const int* __restrict__ label_ids, int n_table, int n_rows,
                                                          const int* __restrict__ n_rows_dev, int n_cls, long long* counts, int* err) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int n_valid = f1_valid_rows(n_rows, n_rows_dev);
  long long tp = 0, wrong = 0;                              // (lane 0 of each wave counts its rows)
  for (int r = blockIdx.x * F1_ROWS_PER_WG + wave; r < n_valid; r += gridDim.x * F1_ROWS_PER_WG) {   // (wave-uniform)
    const long long pr = row_ids ? (long long)row_ids[r] : (long long)r;
    const long long li = label_ids ? (long long)label_ids[r] : (long long)r;
    bool ok = (n_pred_rows <= 0 || (pr >= 0 && pr < n_pred_rows)) && (!label_ids || n_table <= 0 || (li >= 0 && li < n_table));
    long long y = 0;
    if (ok) {
      y = labels[li];
      ok = y >= 0 && y < n_cls;
    }
    if (!ok) {
      if (lane == 0) atomicOr(err, BLISS_ERR_CAP_CAND);
      continue;
    }
    const bf16_t* x = logits + pr * stride;
    unsigned long long best = 0;
    for (int c = lane; c < n_cls; c += 64) {
      const unsigned long long w = ((unsigned long long)f1_key(x[c]) << 32) | (uint32_t)~(uint32_t)c;
      best = w > best ? w : best;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, d), hi = (uint32_t)__shfl_xor((int)(best >> 32), d);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      best = o > best ? o : best;
    }
    if (lane == 0) {
      const int pred = (int)~(uint32_t)best;
      if (pred == (int)y) tp += 1; else wrong += 1;
    }
  }
  f1_commit(tp, wrong, wrong, tp + wrong, counts);
}

// Element-wise over the (row, class) pairs of the counted rows; per-thread counters, then f1_commit.
__global__ void __launch_bounds__(F1_TPB) k_f1_multilabel(const bf16_t* __restrict__ logits, long long stride, int n_pred_rows,
                                                          const int* __restrict__ row_ids, const float* __restrict__ targets,
                                                          const int* __restrict__ label_ids, int n_table, int n_rows,
                                                          const int* __restrict__ n_rows_dev, int n_cls, long long* counts, int* err) {
  const int n_valid = f1_valid_rows(n_rows, n_rows_dev);
  const long long total = (long long)n_valid * n_cls;
  long long tp = 0, fp = 0, fn = 0, n = 0;
  for (long long i = (long long)blockIdx.x * F1_TPB + threadIdx.x; i < total; i += (long long)gridDim.x * F1_TPB) {
    const int r = (int)(i / n_cls), c = (int)(i - (long long)r * n_cls);
    const long long pr = row_ids ? (long long)row_ids[r] : (long long)r;
    const long long li = label_ids ? (long long)label_ids[r] : (long long)r;
    const bool ok = (n_pred_rows <= 0 || (pr >= 0 && pr < n_pred_rows)) && (!label_ids || n_table <= 0 || (li >= 0 && li < n_table));
    if (!ok) {
      if (c == 0) atomicOr(err, BLISS_ERR_CAP_CAND);
      continue;
    }
    const bool hit = bf2f(logits[pr * stride + c]) > 0.f;                    // (false for NaN and for +-0)
    const bool y = targets[li * n_cls + c] > 0.5f;
    tp += hit && y; fp += hit && !y; fn += !hit && y; n += 1;
  }
  f1_commit(tp, fp, fn, n, counts);
}

int f1_grid(long long work_items, long long per_wg) {
  long long g = (work_items + per_wg - 1) / per_wg;
  return (int)(g > BLISS_F1_MAX_WORKGROUPS ? BLISS_F1_MAX_WORKGROUPS : g);
}

bool f1_args_ok(const void* logits, int64_t stride, int32_t n_pred_rows, const void* labels, const void* label_table, int32_t n_table,
                const int32_t* label_ids, int32_t n_rows, int32_t n_cls, const int64_t* counts, const int32_t* err) {
  if (!logits || !counts || !err || n_cls <= 0 || n_rows < 0 || n_pred_rows < 0 || n_table < 0 || stride < n_cls) return false;
  const bool direct = labels != nullptr, table = label_table != nullptr && label_ids != nullptr;
  if (direct == table) return false;                        // exactly one of the two label forms
  if (direct && (label_table || label_ids)) return false;
  return true;
}

}  // namespace

extern "C" int bliss_f1_multiclass(const void* logits, int64_t stride, int32_t n_pred_rows, const int32_t* row_ids, const int64_t* labels,
                                   const int64_t* label_table, int32_t n_table, const int32_t* label_ids, int32_t n_rows,
                                   const int32_t* n_rows_dev, int32_t n_cls, int64_t* counts, int32_t* err, void* stream) {
  if (!f1_args_ok(logits, stride, n_pred_rows, labels, label_table, n_table, label_ids, n_rows, n_cls, counts, err)) return BLISS_EINVAL;
  if (n_rows == 0) return 0;
  k_f1_multiclass<<<f1_grid(n_rows, F1_ROWS_PER_WG), F1_TPB, 0, (hipStream_t)stream>>>(
      (const bf16_t*)logits, stride, n_pred_rows, row_ids, (const long long*)(labels ? labels : label_table), label_ids, n_table, n_rows,
      n_rows_dev, n_cls, (long long*)counts, err);
  return (int)hipGetLastError();
}

extern "C" int bliss_f1_multilabel(const void* logits, int64_t stride, int32_t n_pred_rows, const int32_t* row_ids, const float* labels,
                                   const float* label_table, int32_t n_table, const int32_t* label_ids, int32_t n_rows,
                                   const int32_t* n_rows_dev, int32_t n_cls, int64_t* counts, int32_t* err, void* stream) {
  if (!f1_args_ok(logits, stride, n_pred_rows, labels, label_table, n_table, label_ids, n_rows, n_cls, counts, err)) return BLISS_EINVAL;
  if (n_rows == 0) return 0;
  k_f1_multilabel<<<f1_grid((long long)n_rows * n_cls, F1_TPB), F1_TPB, 0, (hipStream_t)stream>>>(
      (const bf16_t*)logits, stride, n_pred_rows, row_ids, labels ? labels : label_table, label_ids, n_table, n_rows, n_rows_dev, n_cls,
      (long long*)counts, err);
  return (int)hipGetLastError();
}
