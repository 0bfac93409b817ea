// Evaluation kernels of the fine-tuning heads (gfx950; small HBM-bound row reductions over the fp32 `label_logits` of the VQA / VCR /
// RefCOCO+ mirrors): the device side of common/metrics/{vqa,vcr,refcoco}_metrics.py and of the test-set writers.
//   * vlb_argmax_eval:     argmax per row with torch.argmax's rules (equal maxima -> the LOWEST column; NaN is the largest value and the
//                          FIRST NaN wins; a row of -inf gives column 0), optionally the fp32 softmax of the row, and per mode
//                            0 predict                 (test time)
//                            1 hard labels             vcr_metrics.Accuracy      sum int64 += hits, count += rows with label != -1
//                            2 gather label[r, pred]   vqa_metrics.SoftAccuracy  sum DOUBLE += scores in row order, count += rows
//                            3 gather > 0.5            refcoco_metrics.RefAccuracy  sum int64 += hits, count += rows
//   * vlb_binary_cls_eval: ClsAccuracy / ClsPosAccuracy / ClsPosFraction of refcoco_metrics.py in one pass over [rows, N]
//   * vlb_joint_hits:      JointAccuracy of vcr_metrics.py from the two nets' predictions
// Layout of vlb_argmax_eval: C <= VLB_ARGMAX_WAVE_MAX_C (256) -> ONE WAVE PER ROW, four rows per 256-thread block (a lane reads columns
// lane, lane + 64, ...); C > 256 -> ONE 256-THREAD BLOCK PER ROW (a thread reads columns t, t + 256, ...).  A thread's columns ascend
// and the merge keeps the lower column among equals, so the result does not depend on the layout.  Columns >= C of a row (ld > C) are
// never read.  Softmax (probs != NULL): two more passes over the row, which sits in the cache (the VCR writer's rows are 4 wide).
// Mode 2's double must not depend on block scheduling: the rows write their scores to score[] and a SECOND SINGLE-BLOCK LAUNCH
// (sum_scores_kernel) adds them to the accumulator in ascending row order in fp64 -- the simpler of the two ways (no ticket, no
// device-resident slot table as in metrics.hip): the result is bit-equal to `for r: s += float(score[r])` continued from the
// accumulator's value.  No host synchronisation, no allocation; every output is accumulated (+=), integer counters with one
// 64-bit atomic per row (modes 1, 3) or per wave and counter (the other two kernels).
#include <limits.h>

#include "vlb_common.h"

typedef unsigned long long vlb_u64;

#define VLB_ARGMAX_WAVE_MAX_C 256

// does (v2, i2) beat (v, i) under torch.argmax's order?  NaN above everything, the lowest column among equals / among NaNs
__device__ __forceinline__ bool arg_better(float v2, int i2, float v, int i) {
  if (v != v) return v2 != v2 && i2 < i;
  return v2 != v2 || v2 > v || (v2 == v && i2 < i);
}

__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (arg_better(v2, i2, v, i)) { v = v2; i = i2; }
  }
}

// 256 threads: argmax of the block, broadcast (the block_argmax of metrics.hip with the NaN rule).  sh: 8 floats
__device__ __forceinline__ void block_argmax_nan(float& v, int& i, float* sh) {
  wave_argmax(v, i);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
    sh[wave * 2] = v;
    sh[wave * 2 + 1] = __int_as_float(i);
  }
  __syncthreads();
  v = sh[0];
  i = __float_as_int(sh[1]);
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float v2 = sh[w * 2];
    const int i2 = __float_as_int(sh[w * 2 + 1]);
    if (arg_better(v2, i2, v, i)) { v = v2; i = i2; }
  }
}

// BLOCK = true: one 256-thread block per row; false: one wave per row, 4 rows per block.
template <bool BLOCK>
__global__ __launch_bounds__(256) void argmax_eval_kernel(const float* __restrict__ logits, long ld, int rows, int C, int mode,
                                                          const void* __restrict__ label, long ldl, int32_t* __restrict__ pred,
                                                          float* __restrict__ score, float* __restrict__ probs, long ldp,
                                                          vlb_u64* __restrict__ sum, vlb_u64* __restrict__ count) {
  __shared__ float sh[12];
  const int lane = threadIdx.x & 63;
  const int row = BLOCK ? (int)blockIdx.x : (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (!BLOCK && row >= rows) return;                 // (wave-uniform; no block-wide barrier on this path)
  const int t = BLOCK ? (int)threadIdx.x : lane, step = BLOCK ? 256 : 64;
  const float* x = logits + (long)row * ld;
  float v = -INFINITY;
  int idx = INT_MAX;
  for (int c = t; c < C; c += step) {
    const float xv = x[c];
    if (arg_better(xv, c, v, idx)) { v = xv; idx = c; }
  }
  if (BLOCK) block_argmax_nan(v, idx, sh); else wave_argmax(v, idx);
  if (probs) {                                       // F.softmax(logits.float(), 1): exp(x - max) / sum; a NaN or all -inf row gives NaN
    float s = 0.f;
    for (int c = t; c < C; c += step) s += __expf(x[c] - v);
    s = wave_sum(s);
    if (BLOCK) {
      __syncthreads();
      if (lane == 0) sh[8 + (threadIdx.x >> 6)] = s;
      __syncthreads();
      s = sh[8] + sh[9] + sh[10] + sh[11];
    }
    const float inv = 1.0f / s;
    float* p = probs + (long)row * ldp;
    for (int c = t; c < C; c += step) p[c] = __expf(x[c] - v) * inv;
  }
  if (t != 0) return;
  if (pred) pred[row] = idx;
  if (mode == 0) return;
  if (mode == 1) {
    const long lab = ((const int64_t*)label)[row];
    const bool hit = lab == (long)idx;               // (an out-of-range label never equals a column: a miss)
    if (score) score[row] = hit ? 1.f : 0.f;
    if (hit) atomicAdd(sum, (vlb_u64)1);
    if (lab != -1) atomicAdd(count, (vlb_u64)1);
    return;
  }
  const float g = ((const float*)label)[(long)row * ldl + idx];
  if (mode == 2) {
    score[row] = g;                                  // added up in row order by sum_scores_kernel
    return;
  }
  const bool hit = g > 0.5f;
  if (score) score[row] = hit ? 1.f : 0.f;
  if (hit) atomicAdd(sum, (vlb_u64)1);
  if (row == 0) atomicAdd(count, (vlb_u64)rows);
}

// ONE block: *sum (double) += score[0] + score[1] + ... in this order; *count += rows
__global__ __launch_bounds__(256) void sum_scores_kernel(const float* __restrict__ score, int rows, double* __restrict__ sum,
                                                         int64_t* __restrict__ count) {
  __shared__ float sh[256];
  double s = threadIdx.x == 0 ? *sum : 0.0;
  for (int base = 0; base < rows; base += 256) {
    const int n = min(256, rows - base);
    if ((int)threadIdx.x < n) sh[threadIdx.x] = score[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 0; k < n; ++k) s += (double)sh[k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *sum = s;
    *count += (int64_t)rows;
  }
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lab = (long)label (truncation toward zero: -0.5 -> 0 is VALID, -1 is not), pred = logit > 0 (0 and NaN -> 0)
__global__ __launch_bounds__(256) void binary_cls_eval_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ label,
                                                              long ldl, int rows, int N, vlb_u64* __restrict__ acc) {
  int c[4] = {0, 0, 0, 0};
  const long total = (long)rows * N;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / N, col = e - r * N;
    const long lab = (long)label[r * ldl + col];
    const long p = logits[r * ld + col] > 0.f ? 1 : 0;
    if (lab >= 0) {
      c[0] += p == lab;
      c[1] += 1;
    }
    if (lab == 1) {
      c[2] += p == 1;
      c[3] += 1;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int w = wave_sum_int(c[k]);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(acc + k, (vlb_u64)w);
  }
}

__global__ __launch_bounds__(256) void joint_hits_kernel(const int32_t* __restrict__ pred_a, const int64_t* __restrict__ label_a,
                                                         const int32_t* __restrict__ pred_r, const int64_t* __restrict__ label_r, int rows,
                                                         vlb_u64* __restrict__ acc) {
  int hits = 0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256)
    hits += ((long)pred_a[r] == label_a[r]) && ((long)pred_r[r] == label_r[r]);
  hits = wave_sum_int(hits);
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(acc, (vlb_u64)hits);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(acc + 1, (vlb_u64)rows);
}

extern "C" int vlb_argmax_eval(const float* logits, long ld, int rows, int C, int mode, const void* label, long ldl, int32_t* pred,
                               float* score, float* probs, long ldp, void* sum, int64_t* count, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && C > 0 && ld >= C, "vlb_argmax_eval: logits=%p, C=%d, ld=%ld (need ld >= C > 0)", (const void*)logits, C, ld);
  VLB_CHECK_ARG(mode >= 0 && mode <= 3, "vlb_argmax_eval: mode %d (0 predict, 1 hard, 2 gather, 3 gather > 0.5)", mode);
  VLB_CHECK_ARG(mode == 0 || (label && sum && count), "vlb_argmax_eval: mode %d needs label, sum and count", mode);
  VLB_CHECK_ARG(mode < 2 || ldl >= C, "vlb_argmax_eval: ldl=%ld must be >= C=%d", ldl, C);
  VLB_CHECK_ARG(mode != 2 || score, "vlb_argmax_eval: mode 2 needs score[rows] (the scratch of the ordered sum)");
  VLB_CHECK_ARG(!probs || ldp >= C, "vlb_argmax_eval: ldp=%ld must be >= C=%d", ldp, C);
  if (C > VLB_ARGMAX_WAVE_MAX_C)
    hipLaunchKernelGGL(argmax_eval_kernel<true>, dim3(rows), dim3(256), 0, stream, logits, ld, rows, C, mode, label, ldl, pred, score, probs,
                       ldp, (vlb_u64*)sum, (vlb_u64*)count);
  else
    hipLaunchKernelGGL(argmax_eval_kernel<false>, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, logits, ld, rows, C, mode, label, ldl, pred,
                       score, probs, ldp, (vlb_u64*)sum, (vlb_u64*)count);
  VLB_CHECK_LAUNCH("vlb_argmax_eval");
  if (mode == 2) {
    hipLaunchKernelGGL(sum_scores_kernel, dim3(1), dim3(256), 0, stream, (const float*)score, rows, (double*)sum, count);
    VLB_CHECK_LAUNCH("vlb_argmax_eval (ordered sum)");
  }
  return VLB_OK;
}

extern "C" int vlb_binary_cls_eval(const float* logits, long ld, const float* label, long ldl, int rows, int N, int64_t* acc,
                                   hipStream_t stream) {
  if (rows <= 0 || N <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && label && acc, "vlb_binary_cls_eval: null argument");
  VLB_CHECK_ARG(ld >= N && ldl >= N, "vlb_binary_cls_eval: ld=%ld and ldl=%ld must be >= N=%d", ld, ldl, N);
  const long total = (long)rows * N;
  const int blocks = (int)(total < 256L * 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(binary_cls_eval_kernel, dim3(blocks), dim3(256), 0, stream, logits, ld, label, ldl, rows, N, (vlb_u64*)acc);
  VLB_CHECK_LAUNCH("vlb_binary_cls_eval");
  return VLB_OK;
}

extern "C" int vlb_joint_hits(const int32_t* pred_a, const int64_t* label_a, const int32_t* pred_r, const int64_t* label_r, int rows,
                              int64_t* acc, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(pred_a && label_a && pred_r && label_r && acc, "vlb_joint_hits: null argument");
  const int blocks = rows < 256 * 256 ? (rows + 255) / 256 : 256;
  hipLaunchKernelGGL(joint_hits_kernel, dim3(blocks), dim3(256), 0, stream, pred_a, label_a, pred_r, label_r, rows, (vlb_u64*)acc);
  VLB_CHECK_LAUNCH("vlb_joint_hits");
  return VLB_OK;
}
