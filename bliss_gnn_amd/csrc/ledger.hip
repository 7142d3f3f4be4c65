// Step ledger: one launch of one small workgroup at the end of a train step folds the finished step into a device-resident
// record -- the epoch's loss sum, the reference's num_nodes/i / num_edges/i averages (train_lightning.py:76-136), high-water
// marks of the sampled sizes, the OR of the sampler's error words and an early warning before a capacity overflows.  A loop of
// replayed steps then needs no host read per step.  The rule and the record's layout are normative in
// include/bliss_gnn.h and restated by tests/ledger_ref.py.
//
// Plain C++, fixed-order arithmetic: lane n < L owns layer n's words, lane 0 the scalar words; no lane reads what another lane
// writes in the same launch, so there is no barrier, no atomic and no flag.  The fp64 products and sums stay apart
// (-ffp-contract=off): with w = 0.99 they are the bits TrainStep._ema keeps in Python floats.
#include "common.cuh"
#include "bliss_gnn.h"

namespace {

struct LedgerHead {                       // the first 80 bytes of the record
  unsigned long long steps_epoch, steps_total;
  double loss_last, loss_sum;
  unsigned long long nonfinite;
  double cum_out;
  long long first_bad_step, first_near_step;
  int err, near, n_layers, reserved;
};
static_assert(sizeof(LedgerHead) == 80, "ledger header layout");

struct LedgerCaps { int k[BLISS_LEDGER_MAX_LAYERS], b[BLISS_LEDGER_MAX_LAYERS]; };

__global__ void __launch_bounds__(64) k_step_ledger(const void* __restrict__ loss, int loss_dtype, const int* __restrict__ counts,
                                                    int L, LedgerCaps caps, double w, double regrow_at, char* __restrict__ ledger) {
  LedgerHead* h = (LedgerHead*)ledger;
  double* cum_nodes = (double*)(ledger + sizeof(LedgerHead));
  double* cum_edges = cum_nodes + L;
  int* hw_k = (int*)(cum_edges + L);
  int* hw_b = hw_k + L;
  int* hw_e = hw_b + L;
  const int n = threadIdx.x;
  if (n < L) {                                               // layer n's words (LayerCounts: S E C K B err ...)
    const int* c = counts + 10 * n;
    const int E = c[1], K = c[3], B = c[4];
    const double pn = cum_nodes[n] * w;
    cum_nodes[n] = pn + (double)K;
    const double pe = cum_edges[n] * w;
    cum_edges[n] = pe + (double)B;
    if (K > hw_k[n]) hw_k[n] = K;
    if (B > hw_b[n]) hw_b[n] = B;
    if (E > hw_e[n]) hw_e[n] = E;
  }
  if (n == 0) {
    double x;
    if (loss_dtype == BLISS_LEDGER_LOSS_BF16) x = (double)bf2f(*(const bf16_t*)loss);
    else x = (double)*(const float*)loss;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    const bool finite = ((bits >> 52) & 0x7ffull) != 0x7ffull;
    int e = 0, near = 0;
    for (int l = 0; l < L; ++l) {
      const int* c = counts + 10 * l;
      e |= c[5];
      const double lim_k = regrow_at * (double)caps.k[l], lim_b = regrow_at * (double)caps.b[l];
      if ((double)c[3] > lim_k || (double)c[4] > lim_b) near = 1;
    }
    const long long at = (long long)h->steps_total;
    h->loss_last = x;
    h->loss_sum = h->loss_sum + x;
    if (!finite) h->nonfinite += 1;
    const double po = h->cum_out * w;
    h->cum_out = po + (double)counts[0];
    if (e) {
      if (h->first_bad_step < 0) h->first_bad_step = at;
      h->err |= e;
    }
    if (near) {
      if (h->first_near_step < 0) h->first_near_step = at;
      h->near = 1;
    }
    h->steps_epoch += 1;
    h->steps_total += 1;
  }
}

__global__ void __launch_bounds__(64) k_ledger_mode(int mode, char* __restrict__ ledger) {
  LedgerHead* h = (LedgerHead*)ledger;
  if (threadIdx.x != 0) return;
  if (mode == BLISS_LEDGER_RESET_EPOCH) {
    h->steps_epoch = 0;
    h->loss_sum = 0.0;
    h->nonfinite = 0;
  } else {                                                   // BLISS_LEDGER_REARM
    h->near = 0;
    h->first_near_step = -1;
  }
}

// The running mean / variance of the input layer's size (train_lightning.py:437-441, BatchSizeCallback.push) as a device record:
// lane 0 of one wave folds x = K of `layer`'s counts record.  Four separate fp64 operations per fold (-ffp-contract=off), the
// bits of the same statements in Python floats (tests/batch_stats_ref.py).
struct BatchStats {
  unsigned long long n;
  double m, s;
  unsigned long long reserved;
};
static_assert(sizeof(BatchStats) == BLISS_BATCH_STATS_BYTES, "batch statistics layout");

__global__ void __launch_bounds__(64) k_batch_stats(int mode, const int* __restrict__ counts, int layer, BatchStats* __restrict__ rec) {
  if (threadIdx.x != 0) return;
  if (mode == BLISS_BATCH_STATS_CLEAR) {
    rec->n = 0;
    rec->m = 0.0;
    rec->s = 0.0;
    rec->reserved = 0;
    return;
  }
  const double x = (double)counts[10 * layer + 3];           // LayerCounts: S E C K ...
  const unsigned long long n = rec->n + 1;
  const double m_old = rec->m;
  const double d_old = x - m_old;
  const double q = d_old / (double)n;
  const double m_new = m_old + q;
  const double d_new = x - m_new;
  const double prod = d_old * d_new;
  rec->n = n;
  rec->m = m_new;
  rec->s = rec->s + prod;
}

bool layers_ok(int n_layers) { return n_layers >= 1 && n_layers <= BLISS_LEDGER_MAX_LAYERS; }

}  // namespace

extern "C" int bliss_step_ledger_bytes(int n_layers) {
  if (!layers_ok(n_layers)) return BLISS_EINVAL;
  return (int)sizeof(LedgerHead) + 16 * n_layers + 8 * ((12 * n_layers + 7) / 8);
}

extern "C" int bliss_step_ledger(int mode, const void* loss, int loss_dtype, const int32_t* counts, int n_layers, const int32_t* caps,
                                 double w, double regrow_at, void* ledger, void* stream) {
  if (!ledger || !layers_ok(n_layers)) return BLISS_EINVAL;
  if (mode == BLISS_LEDGER_RESET_EPOCH || mode == BLISS_LEDGER_REARM) {
    k_ledger_mode<<<1, 64, 0, (hipStream_t)stream>>>(mode, (char*)ledger);
    return (int)hipGetLastError();
  }
  if (mode != BLISS_LEDGER_STEP || !loss || !counts || !caps) return BLISS_EINVAL;
  if (loss_dtype != BLISS_LEDGER_LOSS_BF16 && loss_dtype != BLISS_LEDGER_LOSS_F32) return BLISS_EINVAL;
  LedgerCaps c;
  for (int n = 0; n < BLISS_LEDGER_MAX_LAYERS; ++n) {
    c.k[n] = n < n_layers ? caps[3 * n] : 0;
    c.b[n] = n < n_layers ? caps[3 * n + 1] : 0;
  }
  k_step_ledger<<<1, 64, 0, (hipStream_t)stream>>>(loss, loss_dtype, (const int*)counts, n_layers, c, w, regrow_at, (char*)ledger);
  return (int)hipGetLastError();
}

extern "C" int bliss_batch_stats(int mode, const int32_t* counts, int layer, void* record, void* stream) {
  if (!record || (mode != BLISS_BATCH_STATS_PUSH && mode != BLISS_BATCH_STATS_CLEAR)) return BLISS_EINVAL;
  if (mode == BLISS_BATCH_STATS_PUSH && (!counts || layer < 0 || layer >= BLISS_LEDGER_MAX_LAYERS)) return BLISS_EINVAL;
  k_batch_stats<<<1, 64, 0, (hipStream_t)stream>>>(mode, (const int*)counts, layer, (BatchStats*)record);
  return (int)hipGetLastError();
}
