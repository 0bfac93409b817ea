// Validation kernels of the VL-BERT pre-training heads (gfx950; HBM-bound row reductions): the FORWARD-ONLY twins of loss.hip.
//   * vlb_ce_eval:      F.cross_entropy(ignore_index=-1)'s value + the top-1 hit of every labelled row -- MLMAccuracy / MLMAccuracyWVC /
//                       MLMAccuracyAUX and, with V = 2, RelationshipAccuracy (common/metrics/pretrain_metrics.py:20-71)
//   * vlb_soft_ce_eval: soft_cross_entropy (common/utils/misc.py:124-151) + argmax(logits) == argmax(target) over the valid rows
//                       -- MVRCAccuracy (pretrain_metrics.py:74-85)
// One 256-thread block per row, ONE pass over the row: an online (max, sum-exp, argmax) triple per thread, merged across the block with
// the tie rule of torch.argmax (equal values -> the LOWEST column) inside the combine step.  The logits are only read: 2 V bytes per
// labelled row (61 044 B at V = 30522), nothing per unlabelled row -- the fused forward+backward kernels of loss.hip read the row
// twice and write it once.  Columns >= V of a row are padding and never enter the max, the sum or the argmax.
// No host synchronisation, no allocation: where the mean's denominator is not known up front (one-group hard labels, soft labels)
// the rows add their raw sums into a slot of a small device-resident table and the LAST block to retire (ticket counter) divides,
// publishes and clears the slot; the host hands every launch the next slot of the ring, so launches in flight on different streams
// do not share one.
#include <atomic>

#include "arg_reduce.h"

__device__ __forceinline__ float block_sum4(float v, float* sh) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// Raw sums of one launch whose denominator is only known when its last row is done.  Zero at load; the last block clears its slot.
struct EvalSlot {
  float loss;
  unsigned hits, n, ticket;
};
#define VLB_EVAL_SLOTS 256
__device__ EvalSlot g_eval_slots[VLB_EVAL_SLOTS];
static std::atomic<unsigned> g_next_slot{0};

// thread 0 of every block: add this row's share, take a ticket; the last ticket publishes mean loss / hits / count and clears the slot
__device__ __forceinline__ void slot_finish(EvalSlot* sl, bool counted, float row_loss, int hit, float* loss_out, vlb_u64* acc) {
  if (counted) {
    atomicAdd(&sl->loss, row_loss);
    if (hit) atomicAdd(&sl->hits, 1u);
    atomicAdd(&sl->n, 1u);
  }
  __threadfence();
  if (atomicAdd(&sl->ticket, 1u) != gridDim.x - 1) return;
  __threadfence();
  const unsigned n = atomicExch(&sl->n, 0u), hits = atomicExch(&sl->hits, 0u);
  const float loss = atomicExch(&sl->loss, 0.f);
  atomicExch(&sl->ticket, 0u);
  if (n == 0) return;   // nothing counted: loss and counters stay untouched
  atomicAdd(loss_out, loss / (float)n);
  if (hits) atomicAdd(acc, (vlb_u64)hits);
  atomicAdd(acc + 1, (vlb_u64)n);
}

// One block per row.  logits: 16-bit [rows, ld], columns >= V are padding (never read into the reduction).
// count1 != nullptr: compacted rows, [0, *count0) = group 0, the labelled rows behind them = group 1, each with its own mean / counters.
// count1 == nullptr: one group, rows with label outside [0, V) are skipped wherever they stand; denominator through the slot.
__global__ __launch_bounds__(256) void ce_eval_kernel(const bf16_t* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                                      const float* __restrict__ count0, const float* __restrict__ count1,
                                                      float* __restrict__ loss_out0, float* __restrict__ loss_out1,
                                                      vlb_u64* __restrict__ acc0, vlb_u64* __restrict__ acc1, int32_t* __restrict__ pred,
                                                      int slot) {
  __shared__ float sh[12];
  const int row = blockIdx.x;
  const float* n_valid = count0;
  float* loss_out = loss_out0;
  vlb_u64* acc = acc0;
  if (count1 && (float)row >= *count0) {
    n_valid = count1;
    loss_out = loss_out1;
    acc = acc1;
  }
  const bf16_t* x = logits + (long)row * ld;
  const long label = labels[row];
  const bool labelled = label >= 0 && label < V;   // block-uniform
  float m = -INFINITY, s = 0.f, row_loss = 0.f;
  int idx = INT_MAX;
  if (labelled) {
    // a thread's columns ascend (8 at c, then c + 2048, ...): `>` alone keeps its lowest column among equals
    for (int c = threadIdx.x * 8; c < V; c += 2048) {
      const uint4 w = *(const uint4*)(x + c);      // c + 8 <= ld: ld % 8 == 0 and ld >= V
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
      float v[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = (c + 2 * k < V) ? bflo(ww[k]) : -INFINITY;
        v[2 * k + 1] = (c + 2 * k + 1 < V) ? bfhi(ww[k]) : -INFINITY;
      }
      float cm = v[0];
      int ci = c;
#pragma unroll
      for (int k = 1; k < 8; ++k)
        if (v[k] > cm) { cm = v[k]; ci = c + k; }
      if (cm == -INFINITY) continue;               // (a chunk of -inf logits adds nothing)
      const float mn = fmaxf(m, cm);
      float cs = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) cs += __expf(v[k] - mn);   // exp(-inf) = 0 for the padding
      s = s * __expf(m - mn) + cs;
      if (cm > m) idx = ci;
      m = mn;
    }
    block_arg_reduce(m, s, idx, sh);
    row_loss = m + __logf(s) - bf2f(x[label]);
  }
  if (threadIdx.x != 0) return;
  const int hit = labelled && idx == (int)label;
  if (pred) pred[row] = labelled ? idx : -1;
  if (count1) {
    if (!labelled) return;
    atomicAdd(loss_out, row_loss / fmaxf(*n_valid, 1.f));
    if (hit) atomicAdd(acc, (vlb_u64)1);
    atomicAdd(acc + 1, (vlb_u64)1);
    return;
  }
  slot_finish(&g_eval_slots[slot], labelled, row_loss, hit, loss_out, acc);
}

// One block per row.  logits 16-bit [rows, ld], target fp32 [rows, ldt].  valid iff |sum(t) - 1| < 0.1;
//   loss_row = lse * sum(t) - sum(t * x) (the arithmetic of soft_ce_fwd_bwd_kernel);  hit = argmax(x) == argmax(t)
__global__ __launch_bounds__(256) void soft_ce_eval_kernel(const bf16_t* __restrict__ logits, long ld, int C, const float* __restrict__ target,
                                                           long ldt, float* __restrict__ loss_out, vlb_u64* __restrict__ acc, int slot) {
  __shared__ float sh[28];
  const int row = blockIdx.x;
  const bf16_t* x = logits + (long)row * ld;
  const float* t = target + (long)row * ldt;
  float m = -INFINITY, s = 0.f, tm = -INFINITY, ts = 0.f, dot = 0.f;
  int xi = INT_MAX, ti = INT_MAX;
  for (int c = threadIdx.x; c < C; c += 256) {     // ascending columns per thread: `>` keeps the lowest among equals
    const float v = bf2f(x[c]), tv = t[c];
    arg_merge(m, s, xi, v, 1.f, c);
    if (tv > tm) { tm = tv; ti = c; }
    ts += tv;
    dot += tv * v;
  }
  ts = block_sum4(ts, sh + 20);
  const bool valid = fabsf(ts - 1.f) < 0.1f;       // block-uniform
  float row_loss = 0.f;
  if (valid) {
    block_arg_reduce(m, s, xi, sh);
    block_argmax(tm, ti, sh + 12);
    dot = block_sum4(dot, sh + 24);
    row_loss = (m + __logf(s)) * ts - dot;
  }
  if (threadIdx.x != 0) return;
  slot_finish(&g_eval_slots[slot], valid, row_loss, valid && xi == ti, loss_out, acc);
}

extern "C" int vlb_ce_eval(const void* logits, long ld, int rows, int V, const int64_t* labels, const float* count0, const float* count1,
                           float* loss_out0, float* loss_out1, int64_t* acc0, int64_t* acc1, int32_t* pred, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && labels && loss_out0 && acc0 && V > 0, "vlb_ce_eval: null argument");
  VLB_CHECK_ARG(!count1 || (count0 && loss_out1 && acc1), "vlb_ce_eval: the two-group form needs count0, loss_out1 and acc1");
  VLB_CHECK_ARG(ld >= V && (ld % 8) == 0 && ((uintptr_t)logits % 16) == 0,
                "vlb_ce_eval: ld=%ld must be >= V=%d and a multiple of 8, logits 16-byte aligned", ld, V);
  const int slot = (int)(g_next_slot.fetch_add(1u) % VLB_EVAL_SLOTS);
  hipLaunchKernelGGL(ce_eval_kernel, dim3(rows), dim3(256), 0, stream, (const bf16_t*)logits, ld, V, labels, count0, count1, loss_out0,
                     loss_out1, (vlb_u64*)acc0, (vlb_u64*)acc1, pred, slot);
  VLB_CHECK_LAUNCH("vlb_ce_eval");
  return VLB_OK;
}

extern "C" int vlb_soft_ce_eval(const void* logits, long ld, int rows, int C, const float* target, long ldt, float* loss_out, int64_t* acc,
                                hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && target && loss_out && acc && C > 0, "vlb_soft_ce_eval: null argument");
  VLB_CHECK_ARG(ld >= C && ldt >= C, "vlb_soft_ce_eval: bad leading dimensions");
  const int slot = (int)(g_next_slot.fetch_add(1u) % VLB_EVAL_SLOTS);
  hipLaunchKernelGGL(soft_ce_eval_kernel, dim3(rows), dim3(256), 0, stream, (const bf16_t*)logits, ld, C, target, ldt, loss_out,
                     (vlb_u64*)acc, slot);
  VLB_CHECK_LAUNCH("vlb_soft_ce_eval");
  return VLB_OK;
}
