// Loss kernels of the VL-BERT pre-training heads (gfx950; HBM-bound row reductions).
//   * MLM: F.cross_entropy(logits[B*T, V], labels, ignore_index=-1), mean over labelled rows
//          (pretrain/modules/resnet_vlbert_for_pretraining.py:176-178)
//   * MVRC: soft_cross_entropy (common/utils/misc.py:124-151): rows are valid iff
//          |sum(target) - 1| < 0.1; loss = mean_valid( -sum_c log_softmax(x)_c * t_c )
// Forward and backward are fused: one pass computes the row's log-sum-exp (online max/sum), the
// second writes d(loss)/d(logits) IN PLACE over the bf16 logits (scaled by 1/n_valid * gscale).
// A copy of the logits is only kept when the caller asks for one (API parity / metrics).
// n_valid is produced on the device by the count kernels -> no host synchronisation
// (the reference does `.item()` at misc.py:140).
#include <type_traits>

#include "arg_reduce.h"

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;  // both empty
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// Block-wide (256 threads) reduction of an online-softmax (max, sum) pair, result broadcast, with the roundings written out.
// online_merge's s * e + s2 * e2 holds two products and the build contracts one of them into the add (-ffp-contract=fast); WHICH one
// is the compiler's choice per inlined copy.  When this reduction was a loop over online_merge, the compiler chose differently
// inside an ACC kernel than inside the plain one (the ACC forms' last butterfly step but one), which moved the last bit of a row's
// sum-exp and with it single 16-bit gradients.  What the plain kernels -- hard and soft labels, static and dynamic scale, both
// builds -- were compiled to is the contract: the thread's own product s * e rounded in every step except the last butterfly step
// (o == 1), where the partner's is.  This function states exactly that with __fmul_rn / fmaf, so that every kernel of this file
// computes those bits whatever surrounds the reduction (tests/test_loss_bits_gpu.py holds them to a recording of that build).
template <bool OWN>
__device__ __forceinline__ void online_merge_as_plain(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;  // both empty
  const float e = __expf(m - mn), e2 = __expf(m2 - mn);
  s = OWN ? fmaf(s2, e2, __fmul_rn(s, e)) : fmaf(s, e, __fmul_rn(s2, e2));
  m = mn;
}

__device__ __forceinline__ void block_online_reduce_as_plain(float& m, float& s, float* sh) {
#pragma unroll
  for (int o = 32; o > 1; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge_as_plain<true>(m, s, m2, s2);
  }
  {
    const float m2 = __shfl_xor(m, 1, 64), s2 = __shfl_xor(s, 1, 64);
    online_merge_as_plain<false>(m, s, m2, s2);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
    sh[wave * 2] = m;
    sh[wave * 2 + 1] = s;
  }
  __syncthreads();
  m = sh[0];
  s = sh[1];
#pragma unroll
  for (int w = 1; w < 4; ++w) online_merge_as_plain<true>(m, s, sh[w * 2], sh[w * 2 + 1]);
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// counts[0] = #rows with label >= 0
__global__ void count_labels_kernel(const int64_t* __restrict__ labels, int n, float* __restrict__ counts) {
  int c = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) c += (labels[i] >= 0);
  float f = wave_sum((float)c);
  if ((threadIdx.x & 63) == 0 && f != 0.f) atomicAdd(counts, f);
}

// the same count for the ACC form of the one-group loss, which also adds the rows the accuracy counts -- label in [0, V), the rows
// vlb_ce_eval counts -- to acc[1].  (counts[0] keeps every label >= 0: it is the divisor of the mean, as above.)
__global__ void count_labels_acc_kernel(const int64_t* __restrict__ labels, int n, int V, float* __restrict__ counts, vlb_u64* __restrict__ acc) {
  int c = 0, k = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int64_t l = labels[i];
    c += (l >= 0);
    k += (l >= 0 && l < V);
  }
  float f = wave_sum((float)c);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
  if ((threadIdx.x & 63) == 0) {
    if (f != 0.f) atomicAdd(counts, f);
    if (k) atomicAdd(acc + 1, (vlb_u64)k);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The two row kernels (hard labels, soft labels), one block per row, each in a plain and a row-weighted form.  The forms differ in
// where a row's scale, loss slot and counters come from -- the NORM argument, one of the two structs below -- and in nothing else.
//   select(row, k): false = the row belongs to no sample (skipped like an unlabelled row); otherwise picks the row's loss slot and
//                   counters and loads k, its divisor or its weight
//   mean(v, k):     the row's share of v.  The arithmetic is the form's own and stays so: v / nv here, v * wr there
//   count_up_front(row) / PER_ROW: who adds the counted rows to acc[1] (ACC forms)
// ------------------------------------------------------------------------------------------------------------------
// Batch mean: 1 / max(*n_valid, 1).  Two-group form (compacted MLM rows of the multitask wrapper): rows [0, *n_valid) belong to group
// 0 (mean over n_valid -> loss_out), the rows behind them to group 1 (mean over *n_valid2 -> loss_out2); n_valid2 == nullptr: one
// group.  The counted rows are known before the launch: with up_front thread 0 of block 0 adds *n_valid / *n_valid2 to acc[1] /
// acc2[1], before any early return (its own row may be unlabelled); without, a count kernel has added them (count_labels_acc_kernel).
struct MeanNorm {
  static constexpr bool PER_ROW = false;
  const float* n_valid;
  float* loss_out;
  vlb_u64* acc;
  const float* n_valid2;
  float* loss_out2;
  vlb_u64* acc2;
  bool up_front;
  __device__ __forceinline__ void count_up_front(int row) const {
    if (up_front && row == 0 && threadIdx.x == 0) {
      const vlb_u64 n0 = (vlb_u64)*n_valid;
      if (n0) atomicAdd(acc + 1, n0);
      if (n_valid2) {
        const vlb_u64 n1 = (vlb_u64)*n_valid2;
        if (n1) atomicAdd(acc2 + 1, n1);
      }
    }
  }
  __device__ __forceinline__ bool select(int row, float& nv) {
    if (n_valid2 && (float)row >= *n_valid) {
      n_valid = n_valid2;
      loss_out = loss_out2;
      acc = acc2;
    }
    nv = fmaxf(*n_valid, 1.f);
    return true;
  }
  static __device__ __forceinline__ float mean(float v, float nv) { return v / nv; }
};

// Per-sample weights (vlb_sample_norm_weights, below): w[s(r)] for 1 / n_valid, s(r) = pos(r) / T with pos the row itself or, on the
// compacted MLM rows, sel_pos[r] (-1 behind the labelled rows).  Samples s < B_split add to loss_out / acc, the others to loss_out2 /
// acc2.  A counted row adds its own 1 to acc[1] (integer atomics: no dependence on arrival order); the weights do not enter.
struct RowWeightNorm {
  static constexpr bool PER_ROW = true;
  const int32_t* sel_pos;
  int B, T, B_split;
  const float* w;
  float* loss_out;
  vlb_u64* acc;
  float* loss_out2;
  vlb_u64* acc2;
  __device__ __forceinline__ void count_up_front(int) const {}
  __device__ __forceinline__ bool select(int row, float& wr) {
    const int pos = sel_pos ? sel_pos[row] : row;
    const int smp = pos >= 0 ? pos / T : B;
    if (smp >= B) return false;
    if (smp >= B_split) {
      loss_out = loss_out2;
      acc = acc2;
    }
    wr = w[smp];
    return true;
  }
  static __device__ __forceinline__ float mean(float v, float wr) { return v * wr; }
};

// ---- the row code of the hard-label kernel: 8 columns per thread and step, 16-byte accesses ----
__device__ __forceinline__ void hard_copy_row(const bf16_t* __restrict__ x, bf16_t* __restrict__ cp, int V) {
  for (int c = threadIdx.x * 8; c < V; c += 2048) {
    if (c + 8 <= V) *(uint4*)(cp + c) = *(const uint4*)(x + c);
    else for (int k = c; k < V; ++k) cp[k] = x[k];
  }
}

__device__ __forceinline__ void hard_zero_row(bf16_t* __restrict__ x, int ldv) {
  for (int c = threadIdx.x * 8; c < ldv; c += 2048) *(uint4*)(x + c) = make_uint4(0, 0, 0, 0);
}

// online_merge(m, s, v, 1.f) for the scan below, its early return (both empty: nothing changes) as a select: inside a function the
// compiler kept that return as a second branch per element, which cost the wide rows 2 %
__device__ __forceinline__ void online_add(float& m, float& s, float v) {
  const float mn = fmaxf(m, v);
  const float sn = s * __expf(m - mn) + __expf(v - mn);
  s = (mn == -INFINITY) ? s : sn;
  m = mn;
}

// the thread's online (m, s) over its columns of [0, V) and (ACC) idx, the column of m: a thread's columns ascend, so `>` alone keeps
// its lowest column among equals
template <bool ACC>
__device__ __forceinline__ void hard_scan_row(const bf16_t* __restrict__ x, int V, float& m, float& s, int& idx) {
  m = -INFINITY, s = 0.f, idx = INT_MAX;
  for (int c = threadIdx.x * 8; c < V; c += 2048) {
    const uint4 w = *(const uint4*)(x + c);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = bflo(ww[k]), b = bfhi(ww[k]);
      if (c + 2 * k < V) {
        if (ACC && a > m) idx = c + 2 * k;
        online_add(m, s, a);
      }
      if (c + 2 * k + 1 < V) {
        if (ACC && b > m) idx = c + 2 * k + 1;
        online_add(m, s, b);
      }
    }
  }
}

// x <- (softmax(x) - onehot(label)) * sc over [0, V), zero over the padding [V, ldv)
__device__ __forceinline__ void hard_grad_row(bf16_t* __restrict__ x, int ldv, int V, long label, float lse, float sc) {
  for (int c = threadIdx.x * 8; c < ldv; c += 2048) {
    const uint4 w = *(const uint4*)(x + c);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c0 = c + 2 * k, c1 = c0 + 1;
      float g0 = (c0 < V) ? __expf(bflo(ww[k]) - lse) : 0.f;
      float g1 = (c1 < V) ? __expf(bfhi(ww[k]) - lse) : 0.f;
      if (c0 == label) g0 -= 1.f;
      if (c1 == label) g1 -= 1.f;
      o[k] = pack2bf(g0 * sc, g1 * sc);
    }
    *(uint4*)(x + c) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// logits: bf16 [rows, ld] (columns >= V are padding and are zeroed).
// out: loss slot += mean(row_loss);  logits <- dlogits * mean(gscale).  A row whose label is outside [0, V) (ignore_index) or that
// NORM does not select adds no loss and gets a zero gradient row.
// BWD = false is the forward-only twin of eval_step(): the logits are only read.
// DS (dynamic loss scale): the gradient scale is gscale * *dscale, a device value formed once per block and used exactly where gscale
// is -- the same bits as a launch given the product from the host, and no second pass over the logits.  The static instantiation
// never reads the trailing argument.
// ACC (training-time metrics): the per-thread online (m, s) pair also carries the column of m, merged with the tie rule of arg_reduce.h,
// and a row whose argmax is its label adds 1 to acc[0] of its group -- an integer atomic, so the counters do not depend on arrival
// order.  The columns meet in block_argmax (arg_reduce.h) before (m, s) become the row's.
template <class NORM, bool BWD, bool DS, bool ACC>
__global__ __launch_bounds__(256) void ce_row_kernel(bf16_t* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels, NORM norm,
                                                     float gscale, bf16_t* __restrict__ logits_copy, long ldcopy,
                                                     const float* __restrict__ dscale) {
  if (DS) gscale = __fmul_rn(gscale, *dscale);
  __shared__ float sh[16];
  const int row = blockIdx.x;
  if (ACC) norm.count_up_front(row);
  bf16_t* x = logits + (long)row * ld;
  const long label = labels[row];
  const int ldv = (int)ld;
  if (BWD && logits_copy) hard_copy_row(x, logits_copy + (long)row * ldcopy, V);
  float k;
  if (label < 0 || label >= V || !norm.select(row, k)) {
    if (BWD) hard_zero_row(x, ldv);
    return;
  }
  float m, s;
  int idx;
  hard_scan_row<ACC>(x, V, m, s, idx);
  if (ACC) {
    float mv = m;
    block_argmax(mv, idx, sh + 8);
  }
  block_online_reduce_as_plain(m, s, sh);
  const float lse = m + __logf(s);
  if (threadIdx.x == 0) {
    atomicAdd(norm.loss_out, NORM::mean(lse - bf2f(x[label]), k));
    if (ACC) {
      if (idx == (int)label) atomicAdd(norm.acc, (vlb_u64)1);
      if (NORM::PER_ROW) atomicAdd(norm.acc + 1, (vlb_u64)1);
    }
  }
  if (!BWD) return;
  const float sc = NORM::mean(gscale, k);
  __syncthreads();  // x[label] read above before anyone overwrites it
  hard_grad_row(x, ldv, V, label, lse, sc);
}

// The runtime (dscale != nullptr, acc != nullptr) of an entry point as the <DS, ACC> of its launch:
//   with_ds_acc(dscale, acc, [&](auto DS, auto ACC) { hipLaunchKernelGGL((kernel<..., DS(), ACC()>), ...); });
template <class F>
static void with_ds_acc(const void* dscale, const void* acc, F&& launch) {
  if (dscale) {
    if (acc) launch(std::true_type(), std::true_type());
    else launch(std::true_type(), std::false_type());
  } else {
    if (acc) launch(std::false_type(), std::true_type());
    else launch(std::false_type(), std::false_type());
  }
}

// ------------------------------------------------------------------------------------------------------------------
// MLM head compaction.  ~85 % of the text positions carry no label (ignore_index -1): their logits rows are never read by
// the loss and their d(logits) rows are exactly zero, so transform -> LayerNorm -> decoder (modeling.py:439-472) and the whole
// backward of the head only need the LABELLED rows.  This kernel builds the (stable, ascending) list of labelled positions:
//   sel_pos[k]  = position i in [0, n) of the k-th labelled row (-1 beyond the count)
//   sel_src[k]  = src_rows[i]: its row in the packed encoder output (-1 -> zero row)
//   labels_c[k] = its label (-1 beyond the count)
//   counts[0] = labelled rows among positions [0, n_split) (image-caption samples), counts[1] = among [n_split, n) (text-only
//   auxiliary samples of the multitask wrapper); *overflow |= (count > cap): the rows that did not fit are NOT trained on, so the
//   host treats the flag as an error (engine.loss_values) -- capacity is a contract with the data pipeline (masking probability).
// One 1024-thread block walks the positions in tiles of 16384: wave w owns the 16 consecutive 64-position chunks 16 w .. 16 w + 15 of
// the tile, reads each with one coalesced load (all 16 in flight) and keeps the labels in registers -- they are read once.  A ballot
// per chunk gives the labelled positions as a bit mask; the slot of a position is (rows of the tiles before) + (rows of the waves
// below, from 16 wave totals in LDS) + (rows of the wave's chunks before, a running popcount) + (set bits below the lane).
// ------------------------------------------------------------------------------------------------------------------
#define MLM_TILE_CHUNKS 16      // chunks per wave and tile
__global__ __launch_bounds__(1024) void mlm_compact_kernel(const int64_t* __restrict__ labels, const int32_t* __restrict__ src_rows, int n,
                                                           int n_split, int V, int cap, int32_t* __restrict__ sel_pos,
                                                           int32_t* __restrict__ sel_src, int64_t* __restrict__ labels_c,
                                                           float* __restrict__ count0, float* __restrict__ count1,
                                                           int32_t* __restrict__ overflow) {
  __shared__ int wsum[16], wsum0[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int total = 0, n0 = 0;      // labelled positions so far: all, and those in front of n_split
  for (int tile0 = 0; tile0 < n; tile0 += 1024 * MLM_TILE_CHUNKS) {
    const int first = tile0 + wave * MLM_TILE_CHUNKS * 64;      // the wave's first position (may lie beyond n)
    int lab[MLM_TILE_CHUNKS];                                    // a kept label is in [0, V): 32 bits hold it
    unsigned long long bal[MLM_TILE_CHUNKS];
    int wtot = 0, wtot0 = 0;
#pragma unroll
    for (int i = 0; i < MLM_TILE_CHUNKS; ++i) {
      const int idx = first + i * 64 + lane;
      const int64_t l = (idx < n) ? labels[idx] : (int64_t)-1;
      lab[i] = (int)l;
      bal[i] = __ballot(l >= 0 && l < V);
    }
#pragma unroll
    for (int i = 0; i < MLM_TILE_CHUNKS; ++i) {
      const int d = n_split - (first + i * 64);                  // positions of the chunk in front of the split
      const unsigned long long front = d <= 0 ? 0ull : (d >= 64 ? ~0ull : (1ull << d) - 1ull);
      wtot += __popcll(bal[i]);
      wtot0 += __popcll(bal[i] & front);
    }
    __syncthreads();      // (the previous tile's totals have been read)
    if (lane == 0) {
      wsum[wave] = wtot;
      wsum0[wave] = wtot0;
    }
    __syncthreads();
    int k = total;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w < wave) k += wsum[w];
      total += wsum[w];
      n0 += wsum0[w];
    }
#pragma unroll
    for (int i = 0; i < MLM_TILE_CHUNKS; ++i) {
      if ((bal[i] >> lane) & 1ull) {
        const int kk = k + __popcll(bal[i] & below), idx = first + i * 64 + lane;
        if (kk < cap) {
          sel_pos[kk] = idx;
          sel_src[kk] = src_rows[idx];
          labels_c[kk] = (int64_t)lab[i];
        }
      }
      k += __popcll(bal[i]);
    }
  }
  for (int q = total + tid; q < cap; q += 1024) {   // padding behind the labelled rows
    sel_pos[q] = -1;
    sel_src[q] = -1;
    labels_c[q] = -1;
  }
  if (tid == 0) {
    const int kept = min(total, cap);
    n0 = min(n0, kept);
    *count0 = (float)n0;
    *count1 = (float)(kept - n0);
    if (total > cap) *overflow = 1;
  }
}

extern "C" int vlb_mlm_compact(const int64_t* labels, const int32_t* src_rows, int n, int n_split, int V, int cap, int32_t* sel_pos,
                               int32_t* sel_src, int64_t* labels_c, float* count0, float* count1, int32_t* overflow, hipStream_t stream) {
  VLB_CHECK_ARG(labels && src_rows && sel_pos && sel_src && labels_c && count0 && count1 && overflow, "vlb_mlm_compact: null argument");
  VLB_CHECK_ARG(n > 0 && cap > 0 && n_split >= 0 && n_split <= n, "vlb_mlm_compact: bad sizes");
  hipLaunchKernelGGL(mlm_compact_kernel, dim3(1), dim3(1024), 0, stream, labels, src_rows, n, n_split, V, cap, sel_pos, sel_src, labels_c,
                     count0, count1, overflow);
  VLB_CHECK_LAUNCH("vlb_mlm_compact");
  return VLB_OK;
}

// CE forward + backward on COMPACTED rows: counts are given (vlb_mlm_compact wrote them), two groups with their own means.
// dscale (nullable): gscale * *dscale from a device scalar -- the dynamic loss scale of an fp16 run.  acc0 / acc1 (both or neither):
// [hits, counted rows] of the two groups added to an int64[2] each.
extern "C" int vlb_ce_fwd_bwd_compact(void* logits, long ld, int rows, int V, const int64_t* labels_c, const float* count0,
                                      const float* count1, float gscale, const float* dscale, float* loss_out0, float* loss_out1,
                                      int64_t* acc0, int64_t* acc1, hipStream_t stream) {
  VLB_CHECK_ARG(!acc0 == !acc1, "vlb_ce_fwd_bwd_compact: null counters");
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && labels_c && count0 && count1 && loss_out0 && loss_out1, "vlb_ce_fwd_bwd_compact: null argument");
  VLB_CHECK_ARG(ld >= V && (ld % 8) == 0, "vlb_ce_fwd_bwd_compact: ld=%ld must be >= V=%d and a multiple of 8", ld, V);
  const MeanNorm norm = {count0, loss_out0, (vlb_u64*)acc0, count1, loss_out1, (vlb_u64*)acc1, true};
  with_ds_acc(dscale, acc0, [&](auto DS, auto ACC) {
    hipLaunchKernelGGL((ce_row_kernel<MeanNorm, true, DS(), ACC()>), dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, V, labels_c, norm, gscale,
                       (bf16_t*)nullptr, 0L, dscale);
  });
  VLB_CHECK_LAUNCH("vlb_ce_fwd_bwd_compact");
  return VLB_OK;
}

// row validity for the soft-label loss: valid[r] = |sum_c t[r,c] - 1| < 0.1 ; counts[0] += #valid
__global__ __launch_bounds__(256) void soft_valid_kernel(const float* __restrict__ target, long ldt, int C, int rows, float* __restrict__ tsum,
                                                         float* __restrict__ counts) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* t = target + (long)row * ldt;
  // a lane adds its columns lane, lane + 64, ... in ascending order (the sum decides validity: keep that order), eight loads in
  // flight ahead of the adds
  float s = 0.f;
  for (int c = lane; c < C; c += 512) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (c + 64 * u < C) ? t[c + 64 * u] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (c + 64 * u < C) s += v[u];
  }
  s = wave_sum(s);
  if (lane == 0) {
    tsum[row] = s;
    if (fabsf(s - 1.f) < 0.1f) atomicAdd(counts, 1.f);
  }
}

// ---- the row code of the soft-label kernel: one column per thread and step ----
// the thread's online (m, s) and its share of sum(t * x) over [0, C); (ACC) xi / ti, the columns of the largest x and the largest t (tm):
// ascending columns per thread, so `>` keeps the lowest among equals
template <bool ACC>
__device__ __forceinline__ void soft_scan_row(const bf16_t* __restrict__ x, const float* __restrict__ t, int C, float& m, float& s, float& dot,
                                              int& xi, float& tm, int& ti) {
  m = -INFINITY, s = 0.f, dot = 0.f, tm = -INFINITY, xi = INT_MAX, ti = INT_MAX;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float v = bf2f(x[c]), tv = t[c];
    if (ACC) {
      if (v > m) xi = c;
      if (tv > tm) { tm = tv; ti = c; }
    }
    online_merge(m, s, v, 1.f);
    dot += tv * v;
  }
}

// x <- (softmax(x) * sum(t) - t) * sc over [0, C), zero over the padding [C, ldv)
__device__ __forceinline__ void soft_grad_row(bf16_t* __restrict__ x, const float* __restrict__ t, int ldv, int C, float lse, float ts, float sc) {
  for (int c = threadIdx.x; c < ldv; c += 256) {
    float g = 0.f;
    if (c < C) g = (__expf(bf2f(x[c]) - lse) * ts - t[c]) * sc;
    x[c] = f2bf(g);
  }
}

// logits bf16 [rows, ld] -> in place d(logits); target fp32 [rows, ldt]; a row is valid iff |tsum[row] - 1| < 0.1 (soft_valid_kernel).
//   loss_row = lse * sum(t) - sum(t * x);  dlogit_c = mean((softmax_c * sum(t) - t_c) * gscale)
// NORM, BWD, DS: as in ce_row_kernel.  ACC: the pass that reads x and t also takes argmax(x) and argmax(t) over [0, C) (lowest column
// among equals); a valid row where they agree adds 1 to acc[0].
template <class NORM, bool BWD, bool DS, bool ACC>
__global__ __launch_bounds__(256) void soft_ce_row_kernel(bf16_t* __restrict__ logits, long ld, int C, const float* __restrict__ target, long ldt,
                                                          const float* __restrict__ tsum, NORM norm, float gscale,
                                                          bf16_t* __restrict__ logits_copy, long ldcopy, const float* __restrict__ dscale) {
  __shared__ float sh[ACC ? 28 : 16];
  if (DS) gscale = __fmul_rn(gscale, *dscale);
  const int row = blockIdx.x;
  if (ACC) norm.count_up_front(row);
  bf16_t* x = logits + (long)row * ld;
  const float* t = target + (long)row * ldt;
  const int ldv = (int)ld;
  if (BWD && logits_copy) {
    bf16_t* cp = logits_copy + (long)row * ldcopy;
    for (int c = threadIdx.x; c < C; c += 256) cp[c] = x[c];
  }
  const float ts = tsum[row];
  float k;
  if (!(fabsf(ts - 1.f) < 0.1f) || !norm.select(row, k)) {
    if (BWD)
      for (int c = threadIdx.x; c < ldv; c += 256) x[c] = 0;
    return;
  }
  float m, s, dot, tm;
  int xi, ti;
  soft_scan_row<ACC>(x, t, C, m, s, dot, xi, tm, ti);
  if (ACC) {      // the threads' (maximum, its column) pairs -> the row's two argmaxes
    float mv = m;
    block_argmax(mv, xi, sh + 12);
    block_argmax(tm, ti, sh + 20);
    if (threadIdx.x == 0) {
      if (xi == ti) atomicAdd(norm.acc, (vlb_u64)1);
      if (NORM::PER_ROW) atomicAdd(norm.acc + 1, (vlb_u64)1);
    }
  }
  block_online_reduce_as_plain(m, s, sh);
  dot = block_sum(dot, sh + 8);
  const float lse = m + __logf(s);
  if (threadIdx.x == 0) atomicAdd(norm.loss_out, NORM::mean(lse * ts - dot, k));
  if (!BWD) return;
  soft_grad_row(x, t, ldv, C, lse, ts, NORM::mean(gscale, k));
}

// dscale, acc: nullable, as in vlb_ce_fwd_bwd_compact (one group, one int64[2])
extern "C" int vlb_ce_fwd_bwd(void* logits, long ld, int rows, int V, const int64_t* labels, float* counts, float gscale, const float* dscale,
                              float* loss_out, void* logits_copy, long ldcopy, int64_t* acc, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && labels && counts && loss_out, "vlb_ce_fwd_bwd: null argument");
  VLB_CHECK_ARG(ld >= V && (ld % 8) == 0, "vlb_ce_fwd_bwd: ld=%ld must be >= V=%d and a multiple of 8", ld, V);
  (void)hipMemsetAsync(counts, 0, sizeof(float), stream);
  const int cblocks = vlb_cdiv(rows, 256) > 64 ? 64 : vlb_cdiv(rows, 256);
  if (acc) hipLaunchKernelGGL(count_labels_acc_kernel, dim3(cblocks), dim3(256), 0, stream, labels, rows, V, counts, (vlb_u64*)acc);
  else hipLaunchKernelGGL(count_labels_kernel, dim3(cblocks), dim3(256), 0, stream, labels, rows, counts);
  const MeanNorm norm = {counts, loss_out, (vlb_u64*)acc, nullptr, nullptr, nullptr, false};
  with_ds_acc(dscale, acc, [&](auto DS, auto ACC) {
    hipLaunchKernelGGL((ce_row_kernel<MeanNorm, true, DS(), ACC()>), dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, V, labels, norm, gscale,
                       (bf16_t*)logits_copy, ldcopy, dscale);
  });
  VLB_CHECK_LAUNCH("vlb_ce_fwd_bwd");
  return VLB_OK;
}

extern "C" int vlb_soft_ce_fwd_bwd(void* logits, long ld, int rows, int C, const float* target, long ldt, float* tsum, float* counts,
                                   float gscale, const float* dscale, float* loss_out, void* logits_copy, long ldcopy, int64_t* acc,
                                   hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && target && tsum && counts && loss_out, "vlb_soft_ce_fwd_bwd: null argument");
  VLB_CHECK_ARG(ld >= C && ldt >= C, "vlb_soft_ce_fwd_bwd: bad leading dimensions");
  (void)hipMemsetAsync(counts, 0, sizeof(float), stream);
  hipLaunchKernelGGL(soft_valid_kernel, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, target, ldt, C, rows, tsum, counts);
  const MeanNorm norm = {counts, loss_out, (vlb_u64*)acc, nullptr, nullptr, nullptr, true};
  with_ds_acc(dscale, acc, [&](auto DS, auto ACC) {
    hipLaunchKernelGGL((soft_ce_row_kernel<MeanNorm, true, DS(), ACC()>), dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, C, target, ldt,
                       (const float*)tsum, norm, gscale, (bf16_t*)logits_copy, ldcopy, dscale);
  });
  VLB_CHECK_LAUNCH("vlb_soft_ce_fwd_bwd");
  return VLB_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// VQA answer loss (vqa/modules/resnet_vlbert_for_vqa.py:226): F.binary_cross_entropy_with_logits(logits[B,A], label) * A,
// i.e. (1/B) sum_b sum_a ( max(x,0) - x y + log(1 + exp(-|x|)) ); d/dx = (sigmoid(x) - y) / B.  Forward and backward fused like
// the CE kernels: logits (bf16 [rows, ld], columns >= A are padding and are zeroed) are overwritten by gscale * d(loss)/dx, the
// untouched logits are copied out when asked for (label_logits of the reference's outputs dict).  One block per row.
// ------------------------------------------------------------------------------------------------------------------
template <bool DS = false>
__global__ __launch_bounds__(256) void bce_logits_fwd_bwd_kernel(bf16_t* __restrict__ logits, long ld, int A, const float* __restrict__ label,
                                                                 long ldl, int rows, float gscale, float pos_weight,
                                                                 float* __restrict__ loss_out, bf16_t* __restrict__ logits_copy, long ldcopy,
                                                                 const float* __restrict__ dscale = nullptr) {
  __shared__ float sh[4];
  if (DS) gscale = __fmul_rn(gscale, *dscale);
  const int row = blockIdx.x;
  bf16_t* x = logits + (long)row * ld;
  const float* y = label + (long)row * ldl;
  const float inv_rows = 1.0f / (float)rows;
  float acc = 0.f;
  for (int a = threadIdx.x; a < (int)ld; a += 256) {
    if (a < A) {
      const float v = bf2f(x[a]), t = y[a];
      if (logits_copy) logits_copy[(long)row * ldcopy + a] = x[a];
      const float e = __expf(-fabsf(v));
      const float w = t > 0.5f ? pos_weight : 1.0f;       // element weight (the `weight=` tensor of vcr/modules/resnet_vlbert_for_vcr.py:336-339)
      acc += w * (fmaxf(v, 0.f) - v * t + log1pf(e));
      const float sig = v >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
      x[a] = f2bf(w * (sig - t) * inv_rows * gscale);
    } else {
      x[a] = 0;
      if (logits_copy && a < (int)ldcopy) logits_copy[(long)row * ldcopy + a] = 0;
    }
  }
  const float s = block_sum(acc, sh);
  if (threadIdx.x == 0) atomicAdd(loss_out, s * inv_rows);
}

extern "C" int vlb_bce_logits_fwd_bwd(void* logits, long ld, int rows, int A, const float* label, long ldl, float gscale,
                                      const float* dscale, float pos_weight, float* loss_out, void* logits_copy, long ldcopy,
                                      hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && label && loss_out && A > 0 && ld >= A && ldl >= A, "vlb_bce_logits_fwd_bwd: bad argument");
  VLB_CHECK_ARG(!logits_copy || ldcopy >= A, "vlb_bce_logits_fwd_bwd: ldcopy too small");
  if (dscale)
    hipLaunchKernelGGL(bce_logits_fwd_bwd_kernel<true>, dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, A, label, ldl, rows, gscale,
                       pos_weight, loss_out, (bf16_t*)logits_copy, ldcopy, dscale);
  else
    hipLaunchKernelGGL(bce_logits_fwd_bwd_kernel<false>, dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, A, label, ldl, rows, gscale,
                       pos_weight, loss_out, (bf16_t*)logits_copy, ldcopy, (const float*)nullptr);
  VLB_CHECK_LAUNCH("vlb_bce_logits_fwd_bwd");
  return VLB_OK;
}

// y = x * keep(idx) / (1 - p) with the counter RNG (element index = position in the [n] array); the same call on dy is the backward.
__global__ __launch_bounds__(256) void dropout_bf16_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long n, uint32_t drop_thr,
                                                           float drop_scale, const uint32_t* __restrict__ seedp, uint32_t tag) {
  const uint32_t seed = (drop_thr && seedp) ? *seedp : 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = bf2f(x[i]);
    y[i] = f2bf((!drop_thr || vlb_keep(seed, tag, (uint32_t)i, drop_thr)) ? v * (drop_thr ? drop_scale : 1.0f) : 0.f);
  }
}

extern "C" int vlb_dropout_bf16(const void* x, void* y, long n, float drop_p, const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(x && y && n < (1L << 32), "vlb_dropout_bf16: bad argument");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_dropout_bf16: dropout needs a device seed pointer");
  const uint32_t thr = vlb_drop_thr(drop_p);
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dropout_bf16_kernel, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, n, thr, vlb_drop_scale(thr),
                     seed, tag);
  VLB_CHECK_LAUNCH("vlb_dropout_bf16");
  return VLB_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Per-sample loss normalisation (NETWORK.MLM_LOSS_NORM_IN_BATCH_FIRST / MVRC_LOSS_NORM_IN_BATCH_FIRST,
// pretrain/modules/resnet_vlbert_for_pretraining.py:168-174, 183-190; multitask :219-231, 252-259):
//   loss = sum_b ( sum_t l_bt / (n_b + 1e-4) ) / ( #{b : n_b > 0} + 1e-4 )
// with n_b the labelled tokens (valid regions) of sample b.  Every row of sample b therefore carries the one weight
//   w[b] = 1 / ((n_b + 1e-4) (n_has + 1e-4))
// and the entry points below launch the row kernels above with RowWeightNorm: `1 / n_valid` replaced by `w[s(r)]`, s(r) the sample
// of row r -- one more scalar load and one fp32 multiply per row.
//
// sample_norm_weights_kernel: ONE 1024-thread block (a batch has a few hundred samples of at most 512 positions).  Wave v counts the
// rows of samples v, v + 16, ... -- integers, so the order of the additions does not matter -- and leaves n_b in w[b]; after a
// barrier the threads count, per group, the samples with n_b > 0 and the rows (integers again), and every w[b] is formed from
// n_b and its group's n_has.  Hard labels ([B, T] int64, labelled iff 0 <= label < V): samples [0, B_split) are the caption group,
// the rest the text-only group of the multitask wrapper, each with its own n_has.  Soft labels: tsum [B * T] of soft_valid_kernel,
// valid iff |tsum - 1| < 0.1, one group.  count0 / count1 (nullable): the row totals of the two groups, WRITTEN -- the slots the
// unweighted losses fill.  A sample without rows gets weight 0 (no row reads it).
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sample_norm_weights_kernel(const int64_t* __restrict__ labels, const float* __restrict__ tsum, int B,
                                                                   int T, int V, int B_split, float* __restrict__ w,
                                                                   float* __restrict__ count0, float* __restrict__ count1) {
  __shared__ int sh[16 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = wave; b < B; b += 16) {
    int c = 0;
    for (int t = lane; t < T; t += 64) {
      const long i = (long)b * T + t;
      if (labels) {
        const int64_t l = labels[i];
        c += (l >= 0 && l < V);
      } else {
        c += (fabsf(tsum[i] - 1.f) < 0.1f);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) w[b] = (float)c;
  }
  __syncthreads();      // (the block's own global writes are visible to it behind the barrier)
  int has0 = 0, has1 = 0, tot0 = 0, tot1 = 0;
  for (int b = tid; b < B; b += 1024) {
    const int n = (int)w[b];
    if (b < B_split) { has0 += (n > 0); tot0 += n; }
    else { has1 += (n > 0); tot1 += n; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    has0 += __shfl_xor(has0, o, 64);
    has1 += __shfl_xor(has1, o, 64);
    tot0 += __shfl_xor(tot0, o, 64);
    tot1 += __shfl_xor(tot1, o, 64);
  }
  if (lane == 0) {
    sh[wave * 4] = has0;
    sh[wave * 4 + 1] = has1;
    sh[wave * 4 + 2] = tot0;
    sh[wave * 4 + 3] = tot1;
  }
  __syncthreads();      // (also: every n_b has been read before any w[b] is overwritten below -- each thread rewrites only what it read)
  has0 = has1 = tot0 = tot1 = 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    has0 += sh[v * 4];
    has1 += sh[v * 4 + 1];
    tot0 += sh[v * 4 + 2];
    tot1 += sh[v * 4 + 3];
  }
  for (int b = tid; b < B; b += 1024) {
    const float n = w[b];
    const float nh = (float)(b < B_split ? has0 : has1);
    w[b] = n > 0.f ? 1.f / ((n + 1e-4f) * (nh + 1e-4f)) : 0.f;
  }
  if (tid == 0) {
    if (count0) *count0 = (float)tot0;
    if (count1) *count1 = (float)tot1;
  }
}

extern "C" int vlb_sample_norm_weights(const int64_t* labels, const float* tsum, int B, int T, int V, int B_split, float* w, float* count0,
                                       float* count1, hipStream_t stream) {
  if (B <= 0) return VLB_OK;
  VLB_CHECK_ARG(w && (!labels != !tsum), "vlb_sample_norm_weights: needs w and exactly one of labels / tsum");
  VLB_CHECK_ARG(T > 0 && B_split >= 0 && B_split <= B && (labels || B_split == B), "vlb_sample_norm_weights: bad sizes (B=%d T=%d B_split=%d)",
                B, T, B_split);
  hipLaunchKernelGGL(sample_norm_weights_kernel, dim3(1), dim3(1024), 0, stream, labels, tsum, B, T, V, B_split, w, count0, count1);
  VLB_CHECK_LAUNCH("vlb_sample_norm_weights");
  return VLB_OK;
}

static int ce_rowweight_check(const char* who, const void* logits, long ld, int rows, int V, const void* labels, const void* sel_pos, int B, int T,
                              int B_split, const void* w, const void* loss_out0, const void* loss_out1, const void* acc0, const void* acc1) {
  VLB_CHECK_ARG(logits && labels && w && loss_out0, "%s: null argument", who);
  VLB_CHECK_ARG(B > 0 && T > 0 && B_split >= 0 && B_split <= B, "%s: bad sizes (B=%d T=%d B_split=%d)", who, B, T, B_split);
  VLB_CHECK_ARG(sel_pos || (long)rows <= (long)B * T, "%s: %d rows for %d samples of %d positions", who, rows, B, T);
  VLB_CHECK_ARG(B_split == B || (loss_out1 && (!acc0 || acc1)), "%s: two groups need loss_out1 (and acc1 with acc0)", who);
  VLB_CHECK_ARG(ld >= V && (ld % 8) == 0 && ((uintptr_t)logits % 16) == 0, "%s: ld=%ld must be >= V=%d and a multiple of 8, logits 16-byte aligned",
                who, ld, V);
  return VLB_OK;
}

// labels: per ROW ([B, T] flattened, or labels_c of vlb_mlm_compact together with its sel_pos); w: vlb_sample_norm_weights' output over
// the B samples.  dscale, acc0 / acc1, logits_copy: nullable, as in vlb_ce_fwd_bwd.
extern "C" int vlb_ce_rowweight_fwd_bwd(void* logits, long ld, int rows, int V, const int64_t* labels, const int32_t* sel_pos, int B, int T,
                                        int B_split, const float* w, float gscale, const float* dscale, float* loss_out0, float* loss_out1,
                                        void* logits_copy, long ldcopy, int64_t* acc0, int64_t* acc1, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  if (ce_rowweight_check("vlb_ce_rowweight_fwd_bwd", logits, ld, rows, V, labels, sel_pos, B, T, B_split, w, loss_out0, loss_out1, acc0, acc1) !=
      VLB_OK)
    return VLB_ERR_ARG;
  VLB_CHECK_ARG(!logits_copy || ldcopy >= V, "vlb_ce_rowweight_fwd_bwd: ldcopy too small");
  const RowWeightNorm norm = {sel_pos, B, T, B_split, w, loss_out0, (vlb_u64*)acc0, loss_out1, (vlb_u64*)acc1};
  with_ds_acc(dscale, acc0, [&](auto DS, auto ACC) {
    hipLaunchKernelGGL((ce_row_kernel<RowWeightNorm, true, DS(), ACC()>), dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, V, labels, norm,
                       gscale, (bf16_t*)logits_copy, ldcopy, dscale);
  });
  VLB_CHECK_LAUNCH("vlb_ce_rowweight_fwd_bwd");
  return VLB_OK;
}

extern "C" int vlb_ce_rowweight_eval(const void* logits, long ld, int rows, int V, const int64_t* labels, const int32_t* sel_pos, int B, int T,
                                     int B_split, const float* w, float* loss_out0, float* loss_out1, int64_t* acc0, int64_t* acc1,
                                     hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  if (ce_rowweight_check("vlb_ce_rowweight_eval", logits, ld, rows, V, labels, sel_pos, B, T, B_split, w, loss_out0, loss_out1, acc0, acc1) != VLB_OK)
    return VLB_ERR_ARG;
  VLB_CHECK_ARG(acc0, "vlb_ce_rowweight_eval: null counters");
  const RowWeightNorm norm = {sel_pos, B, T, B_split, w, loss_out0, (vlb_u64*)acc0, loss_out1, (vlb_u64*)acc1};
  hipLaunchKernelGGL((ce_row_kernel<RowWeightNorm, false, false, true>), dim3(rows), dim3(256), 0, stream, (bf16_t*)const_cast<void*>(logits), ld, V,
                     labels, norm, 1.f, (bf16_t*)nullptr, 0L, (const float*)nullptr);
  VLB_CHECK_LAUNCH("vlb_ce_rowweight_eval");
  return VLB_OK;
}

// rows = B * R regions; tsum [rows] and w [B] are written here (row validity, then vlb_sample_norm_weights' arithmetic on it), counts[0]
// = the valid rows as vlb_soft_ce_fwd_bwd leaves it.  dscale, acc, logits_copy: nullable, as in vlb_soft_ce_fwd_bwd.
extern "C" int vlb_soft_ce_rowweight_fwd_bwd(void* logits, long ld, int rows, int C, const float* target, long ldt, float* tsum, int R, float* w,
                                             float* counts, float gscale, const float* dscale, float* loss_out, void* logits_copy, long ldcopy,
                                             int64_t* acc, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && target && tsum && w && counts && loss_out, "vlb_soft_ce_rowweight_fwd_bwd: null argument");
  VLB_CHECK_ARG(ld >= C && ldt >= C && R > 0 && rows % R == 0, "vlb_soft_ce_rowweight_fwd_bwd: bad leading dimensions or rows %% R != 0");
  VLB_CHECK_ARG(!logits_copy || ldcopy >= C, "vlb_soft_ce_rowweight_fwd_bwd: ldcopy too small");
  (void)hipMemsetAsync(counts, 0, sizeof(float), stream);
  hipLaunchKernelGGL(soft_valid_kernel, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, target, ldt, C, rows, tsum, counts);
  hipLaunchKernelGGL(sample_norm_weights_kernel, dim3(1), dim3(1024), 0, stream, (const int64_t*)nullptr, (const float*)tsum, rows / R, R, 0,
                     rows / R, w, (float*)nullptr, (float*)nullptr);
  const RowWeightNorm norm = {nullptr, rows / R, R, rows / R, w, loss_out, (vlb_u64*)acc, nullptr, nullptr};
  with_ds_acc(dscale, acc, [&](auto DS, auto ACC) {
    hipLaunchKernelGGL((soft_ce_row_kernel<RowWeightNorm, true, DS(), ACC()>), dim3(rows), dim3(256), 0, stream, (bf16_t*)logits, ld, C, target, ldt,
                       (const float*)tsum, norm, gscale, (bf16_t*)logits_copy, ldcopy, dscale);
  });
  VLB_CHECK_LAUNCH("vlb_soft_ce_rowweight_fwd_bwd");
  return VLB_OK;
}

extern "C" int vlb_soft_ce_rowweight_eval(const void* logits, long ld, int rows, int C, const float* target, long ldt, float* tsum, int R, float* w,
                                          float* counts, float* loss_out, int64_t* acc, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && target && tsum && w && counts && loss_out && acc, "vlb_soft_ce_rowweight_eval: null argument");
  VLB_CHECK_ARG(ld >= C && ldt >= C && R > 0 && rows % R == 0, "vlb_soft_ce_rowweight_eval: bad leading dimensions or rows %% R != 0");
  (void)hipMemsetAsync(counts, 0, sizeof(float), stream);
  hipLaunchKernelGGL(soft_valid_kernel, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, target, ldt, C, rows, tsum, counts);
  hipLaunchKernelGGL(sample_norm_weights_kernel, dim3(1), dim3(1024), 0, stream, (const int64_t*)nullptr, (const float*)tsum, rows / R, R, 0,
                     rows / R, w, (float*)nullptr, (float*)nullptr);
  const RowWeightNorm norm = {nullptr, rows / R, R, rows / R, w, loss_out, (vlb_u64*)acc, nullptr, nullptr};
  hipLaunchKernelGGL((soft_ce_row_kernel<RowWeightNorm, false, false, true>), dim3(rows), dim3(256), 0, stream, (bf16_t*)const_cast<void*>(logits), ld,
                     C, target, ldt, (const float*)tsum, norm, 1.f, (bf16_t*)nullptr, 0L, (const float*)nullptr);
  VLB_CHECK_LAUNCH("vlb_soft_ce_rowweight_eval");
  return VLB_OK;
}
