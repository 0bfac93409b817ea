// fp32 front end, hand-over, and losses of the PRE-TRAINING step (`fp32_full`; host side pretrain_f32.py / engine.py): what the
// pre-training engine runs around the fp32 encoder (f32_path.hip) besides the kernels of f32_ends.hip, with every tensor in fp32.
//   * vlb_mask_feature_f32            - the mvrc_ops == 1 substitution of vlb_obj_prep_fwd, applied to vlb_obj_prep_f32_fwd's output
//   * vlb_masked_colsum_f32           - vlb_masked_colsum on an fp32 source (d object_mask_visual_embedding, through the dropout)
//   * vlb_select_rows2_f32            - out[i] = table[sel[i] != 0] (the objects' linguistic embedding as a dense operand)
//   * vlb_table2_grad_f32             - the [2, H] table gradient from the dense one
//   * vlb_group_rowsum_f32            - dst[g] = sum of the g-th group of rows (d text_vis per sample from the per-token rows)
//   * vlb_add_rows_f32                - dst[r] += src[r] over strided rows
//   * vlb_gather_rows_f32 / vlb_scatter_rows_f32 / vlb_head_grad_combine_f32
//   * vlb_ce_f32_fwd_bwd / vlb_ce_f32_fwd_bwd_compact / vlb_soft_ce_f32_fwd_bwd
// None of them touches the 16-bit type: the two builds of the library hold the same code.  Lanes move 16 bytes.  Every sum here is
// taken in a fixed order (no float atomics between workgroups), so losses and these gradients are the same bits on every run.
#include <math.h>

#include "arg_reduce.h"

namespace {

__device__ __forceinline__ float4 drop4p(float4 v, uint32_t seed, uint32_t tag, uint32_t e, uint32_t thr, float scale) {
  // elements e .. e + 3 (e even): two pair hashes, 16 bits per element (the convention of vlb_keep)
  const uint32_t h0 = vlb_rng_pair(seed, tag, e >> 1), h1 = vlb_rng_pair(seed, tag, (e >> 1) + 1);
  v.x = ((h0 & 0xffffu) >= thr) ? v.x * scale : 0.f;
  v.y = ((h0 >> 16) >= thr) ? v.y * scale : 0.f;
  v.z = ((h1 & 0xffffu) >= thr) ? v.z * scale : 0.f;
  v.w = ((h1 >> 16) >= thr) ? v.w * scale : 0.f;
  return v;
}

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// block-wide (256 threads) reductions in a fixed order; result broadcast.  sh: 4 floats, reusable after the call returns.
__device__ __forceinline__ float block_max4(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float block_sum4(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// a[row, 2048:4096] = dropout(mask_emb) for the valid boxes with sel[row] == 1 (resnet_vlbert_for_pretraining.py:114-117): the feature
// half of vlb_obj_prep_f32_fwd's output, with the element index (row * 4096 + 2048 + e) of that kernel's dropout.  One block per row.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_feature_f32_kernel(float* __restrict__ a, const float* __restrict__ boxes, long ldbox,
                                                               const int64_t* __restrict__ sel, const float* __restrict__ mask_emb,
                                                               uint32_t drop_thr, float drop_scale, const uint32_t* __restrict__ seedp,
                                                               uint32_t tag) {
  const int row = blockIdx.x;
  if (sel[row] != 1 || !(boxes[(long)row * ldbox] > -1.5f)) return;
  const uint32_t seed = (drop_thr && seedp) ? *seedp : 0u;
  const int e0 = threadIdx.x * 8;
  float4 f0 = *(const float4*)(mask_emb + e0), f1 = *(const float4*)(mask_emb + e0 + 4);
  if (drop_thr) {
    const uint32_t e = (uint32_t)row * 4096u + 2048u + (uint32_t)e0;
    f0 = drop4p(f0, seed, tag, e, drop_thr, drop_scale);
    f1 = drop4p(f1, seed, tag, e + 4u, drop_thr, drop_scale);
  }
  float* o = a + (long)row * 4096 + 2048 + e0;
  *(float4*)o = f0;
  *(float4*)(o + 4) = f1;
}

// ------------------------------------------------------------------------------------------
// Column sums over selected rows: dst1[c] += sum_{sel[r] == 1} m(r, c) src[r][c], dst0[c] (nullable) += the same over sel[r] == 0;
// m = the dropout mask of element r * row_elems + col_off + c (drop_thr == 0: none).  One 1024-thread workgroup owns 256 columns (a
// lane four consecutive ones); its 16 waves take the rows 16 apart, four loads in flight, and meet in LDS, where the 16 partial sums of a
// column are added in wave order.  No other workgroup touches the column: plain read-modify-write, the same bits on every run.
// ------------------------------------------------------------------------------------------
template <bool TWO>
__global__ __launch_bounds__(1024) void colsum_sel_f32_kernel(const float* __restrict__ src, long lds, const int64_t* __restrict__ sel, int rows,
                                                              int C, float* __restrict__ dst1, float* __restrict__ dst0, uint32_t drop_thr,
                                                              float drop_scale, const uint32_t* __restrict__ seedp, uint32_t tag,
                                                              uint32_t row_elems, uint32_t col_off) {
  __shared__ __attribute__((aligned(16))) float part[TWO ? 2 : 1][16][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const bool live = c < C;      // C % 4 == 0: a lane's columns are all inside or all outside
  const uint32_t seed = (drop_thr && seedp) ? *seedp : 0u;
  float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a0 = a1;
  for (int r0 = wave; r0 < rows; r0 += 64) {
    float4 v[4];
    int s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + 16 * u;
      s[u] = -1;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) {
        const int64_t q = sel[r];
        s[u] = q == 1 ? 1 : (q == 0 ? 0 : -1);
        if (live && (s[u] == 1 || (TWO && s[u] == 0))) v[u] = *(const float4*)(src + (long)r * lds + c);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s[u] == 1) {
        float4 w = v[u];
        if (drop_thr) w = drop4p(w, seed, tag, (uint32_t)(r0 + 16 * u) * row_elems + col_off + (uint32_t)c, drop_thr, drop_scale);
        a1.x += w.x; a1.y += w.y; a1.z += w.z; a1.w += w.w;
      } else if (TWO && s[u] == 0) {
        a0.x += v[u].x; a0.y += v[u].y; a0.z += v[u].z; a0.w += v[u].w;
      }
    }
  }
  *(float4*)&part[0][wave][lane * 4] = a1;
  if (TWO) *(float4*)&part[TWO ? 1 : 0][wave][lane * 4] = a0;
  __syncthreads();
  for (int i = threadIdx.x; i < (TWO ? 512 : 256); i += 1024) {
    const int which = i >> 8, j = i & 255, col = blockIdx.x * 256 + j;
    if (col >= C) continue;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += part[which][w][j];
    float* d = which == 0 ? dst1 : dst0;
    d[col] += t;
  }
}

// out[i, :] = table[sel[i] != 0 ? 1 : 0, :]; one wave per row
__global__ __launch_bounds__(256) void select_rows2_f32_kernel(const float* __restrict__ table, const int64_t* __restrict__ sel,
                                                               float* __restrict__ out, int n, int H) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const float* src = table + (sel[i] != 0 ? (long)H : 0L);
  for (int c = lane * 4; c < H; c += 256) *(float4*)(out + (long)i * H + c) = *(const float4*)(src + c);
}

// dst[g, :] = sum_{t < group_rows} src[g * group_rows + t, :] in ascending t; grid (groups, column chunks of 1024)
__global__ __launch_bounds__(256) void group_rowsum_f32_kernel(const float* __restrict__ src, int group_rows, int H, float* __restrict__ dst,
                                                               long ldd) {
  const int g = blockIdx.x, c = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (c >= H) return;
  const float* s = src + (long)g * group_rows * H + c;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int t = 0;
  for (; t + 4 <= group_rows; t += 4) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const float4*)(s + (long)(t + u) * H);
#pragma unroll
    for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
  }
  for (; t < group_rows; ++t) {
    const float4 v = *(const float4*)(s + (long)t * H);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *(float4*)(dst + (long)g * ldd + c) = acc;
}

// dst[r, :] += src[r, :]; one wave per row
__global__ __launch_bounds__(256) void add_rows_f32_kernel(float* __restrict__ dst, long ldd, const float* __restrict__ src, long lds, int rows,
                                                           int H) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  for (int c = lane * 4; c < H; c += 256) {
    float4 d = *(float4*)(dst + (long)r * ldd + c);
    const float4 s = *(const float4*)(src + (long)r * lds + c);
    d.x += s.x; d.y += s.y; d.z += s.z; d.w += s.w;
    *(float4*)(dst + (long)r * ldd + c) = d;
  }
}

// ------------------------------------------------------------------------------------------
// hand-over between the packed sequence and the heads: fp32 twins of gather_rows / scatter_rows / head_grad_combine (embed.hip)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                              float* __restrict__ out, int n, int H) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int r = idx[i];
  for (int c = lane * 4; c < H; c += 256) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= 0) v = *(const float4*)(src + (long)r * H + c);
    *(float4*)(out + (long)i * H + c) = v;
  }
}

__global__ __launch_bounds__(256) void scatter_rows_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                               float* __restrict__ out, int n, int H) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int r = idx[i];
  if (r < 0) return;
  for (int c = lane * 4; c < H; c += 256) *(float4*)(out + (long)r * H + c) = *(const float4*)(src + (long)i * H + c);
}

// dX[b, s] = (s < T ? d_text[b, s] : 0) + (row (b, s) is the j-th object ? d_obj[b, j] : 0)
__global__ __launch_bounds__(256) void head_grad_combine_f32_kernel(const float* __restrict__ d_text, const float* __restrict__ d_obj,
                                                                    const int32_t* __restrict__ code, float* __restrict__ dx, int B, int T,
                                                                    int R, int S, int H) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B * S) return;
  const int b = row / S, s = row % S;
  const int c_ = code[row], kind = c_ >> 16, idx = c_ & 0xffff;
  const float* t = (s < T && d_text) ? d_text + ((long)b * T + s) * H : nullptr;
  const float* o = (kind == 2 && d_obj && idx < R) ? d_obj + ((long)b * R + idx) * H : nullptr;      // 2 = the object rows of vlb_seq_layout
  for (int c = lane * 4; c < H; c += 256) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t) v = *(const float4*)(t + c);
    if (o) {
      const float4 w = *(const float4*)(o + c);
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    *(float4*)(dx + (long)row * H + c) = v;
  }
}

// ------------------------------------------------------------------------------------------
// Losses on fp32 logits (the conventions of loss.hip: mean over the counted rows, max(count, 1) as the divisor, the gradient
// gscale / count * d(row loss) written in place, pad columns [V, ld) zeroed).  One workgroup per row of ld % 4 == 0 floats, three
// passes over it (122 KB at V = 30522: the second and third come from the L2): maximum, sum of exp(x - max), gradient.  expf / logf
// are the accurate ones.  A row's loss goes to row_loss[row] (0 for a row that does not count); loss_sum_f32_kernel adds them up.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void count_labels_f32_kernel(const int64_t* __restrict__ labels, int n, float* __restrict__ counts) {
  __shared__ int sh[4];
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) c += (labels[i] >= 0);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[0] = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// the ACC form's count: counts[0] as above, and the rows the accuracy counts (label in [0, V), vlb_ce_eval's rule) added to acc[1]
__global__ __launch_bounds__(256) void count_labels_f32_acc_kernel(const int64_t* __restrict__ labels, int n, int V, float* __restrict__ counts,
                                                                   vlb_u64* __restrict__ acc) {
  __shared__ int sh[8];
  int c = 0, k = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int64_t l = labels[i];
    c += (l >= 0);
    k += (l >= 0 && l < V);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o, 64);
    k += __shfl_xor(k, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = c;
    sh[4 + (threadIdx.x >> 6)] = k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
    const int kk = sh[4] + sh[5] + sh[6] + sh[7];
    if (kk) atomicAdd(acc + 1, (vlb_u64)kk);
  }
}

// ACC (training-time metrics; the *_acc kernels below): the maximum pass also keeps the column of the maximum (lowest among equals,
// arg_reduce.h); a counted row whose argmax is its label adds 1 to acc[0] (acc2[0] in group 1), an integer atomic.  The counted rows are
// known before the launch: thread 0 of block 0 adds *n_valid / *n_valid2 to acc[1] / acc2[1] in the two-group form, before any early
// return; in the one-group form count_labels_f32_acc_kernel has added them.  m, s and everything after them are computed as without ACC:
// the same bits.  dscale (nullable, ACC only): gscale * *dscale, rounded once.
template <bool ACC>
__device__ __forceinline__ void ce_f32_body(float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                            const float* __restrict__ n_valid, const float* __restrict__ n_valid2, float gscale,
                                            float* __restrict__ row_loss, float* __restrict__ logits_copy, long ldcopy,
                                            const float* __restrict__ dscale, vlb_u64* __restrict__ acc, vlb_u64* __restrict__ acc2) {
  __shared__ float sh[ACC ? 12 : 4];
  const int row = blockIdx.x, ldv = (int)ld;
  if (ACC && dscale) gscale = __fmul_rn(gscale, *dscale);
  if (ACC && n_valid2 && row == 0 && threadIdx.x == 0) {
    const vlb_u64 n0 = (vlb_u64)*n_valid, n1 = (vlb_u64)*n_valid2;
    if (n0) atomicAdd(acc + 1, n0);
    if (n1) atomicAdd(acc2 + 1, n1);
  }
  if (n_valid2 && (float)row >= *n_valid) {      // two groups of compacted rows, each with its own mean
    n_valid = n_valid2;
    if (ACC) acc = acc2;
  }
  float* x = logits + (long)row * ld;
  const long label = labels[row];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (logits_copy) {
    float* cp = logits_copy + (long)row * ldcopy;
    for (int c = threadIdx.x * 4; c < ldv && c < (int)ldcopy; c += 1024) {
      float4 v = *(const float4*)(x + c);
      if (c + 1 >= V) v.y = 0.f;
      if (c + 2 >= V) v.z = 0.f;
      if (c + 3 >= V) v.w = 0.f;
      if (c >= V) v.x = 0.f;
      *(float4*)(cp + c) = v;
    }
  }
  if (label < 0 || label >= V) {      // ignore_index: no loss, zero gradient row
    for (int c = threadIdx.x * 4; c < ldv; c += 1024) *(float4*)(x + c) = zero;
    if (threadIdx.x == 0) row_loss[row] = 0.f;
    return;
  }
  const float xl = x[label];      // (every thread reads it here: the barriers of the reductions stand before the pass that overwrites it)
  float m = -INFINITY;
  int idx = INT_MAX;      // (ACC) column of m; a thread's columns ascend, so `>` alone keeps its lowest column among equals
  for (int c = threadIdx.x * 4; c < V; c += 1024) {
    const float4 v = *(const float4*)(x + c);
    if (ACC) {
      float a = m;
      if (v.x > a) { a = v.x; idx = c; }
      if (c + 1 < V && v.y > a) { a = v.y; idx = c + 1; }
      if (c + 2 < V && v.z > a) { a = v.z; idx = c + 2; }
      if (c + 3 < V && v.w > a) { a = v.w; idx = c + 3; }
    }
    m = fmaxf(m, v.x);
    if (c + 1 < V) m = fmaxf(m, v.y);
    if (c + 2 < V) m = fmaxf(m, v.z);
    if (c + 3 < V) m = fmaxf(m, v.w);
  }
  if (ACC) {
    float a = m;
    block_argmax(a, idx, sh + 4);
    if (threadIdx.x == 0 && idx == (int)label) atomicAdd(acc, (vlb_u64)1);
  }
  m = block_max4(m, sh);
  float s = 0.f;
  for (int c = threadIdx.x * 4; c < V; c += 1024) {
    const float4 v = *(const float4*)(x + c);
    s += expf(v.x - m);
    if (c + 1 < V) s += expf(v.y - m);
    if (c + 2 < V) s += expf(v.z - m);
    if (c + 3 < V) s += expf(v.w - m);
  }
  s = block_sum4(s, sh);
  // lse = m + log(s) is never formed: at |m| ~ 1e4 its rounding (1e-3 absolute) would be the error of every exp(x - lse)
  const float inv_s = 1.0f / s;
  const float nv = fmaxf(*n_valid, 1.f), sc = gscale / nv;
  if (threadIdx.x == 0) row_loss[row] = (m - xl) + logf(s);
  const int lab = (int)label;
  for (int c = threadIdx.x * 4; c < ldv; c += 1024) {
    const float4 v = *(const float4*)(x + c);
    float4 g;
    g.x = (c < V) ? (expf(v.x - m) * inv_s - (c == lab ? 1.f : 0.f)) * sc : 0.f;
    g.y = (c + 1 < V) ? (expf(v.y - m) * inv_s - (c + 1 == lab ? 1.f : 0.f)) * sc : 0.f;
    g.z = (c + 2 < V) ? (expf(v.z - m) * inv_s - (c + 2 == lab ? 1.f : 0.f)) * sc : 0.f;
    g.w = (c + 3 < V) ? (expf(v.w - m) * inv_s - (c + 3 == lab ? 1.f : 0.f)) * sc : 0.f;
    *(float4*)(x + c) = g;
  }
}

__global__ __launch_bounds__(256) void ce_f32_kernel(float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ n_valid, const float* __restrict__ n_valid2, float gscale,
                                                     float* __restrict__ row_loss, float* __restrict__ logits_copy, long ldcopy) {
  ce_f32_body<false>(logits, ld, V, labels, n_valid, n_valid2, gscale, row_loss, logits_copy, ldcopy, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void ce_f32_acc_kernel(float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ n_valid, const float* __restrict__ n_valid2, float gscale,
                                                         float* __restrict__ row_loss, float* __restrict__ logits_copy, long ldcopy,
                                                         const float* __restrict__ dscale, vlb_u64* __restrict__ acc, vlb_u64* __restrict__ acc2) {
  ce_f32_body<true>(logits, ld, V, labels, n_valid, n_valid2, gscale, row_loss, logits_copy, ldcopy, dscale, acc, acc2);
}

// loss_out0 += (sum of row_loss[0 .. split)) / max(n_valid, 1), loss_out1 += (sum of the rows behind) / max(n_valid2, 1); split = the
// first group's count (n_valid2 == nullptr: one group, every row).  One wave: lane l adds rows l, l + 64, ... in order, then the butterfly.
__global__ __launch_bounds__(64) void loss_sum_f32_kernel(const float* __restrict__ row_loss, int rows, const float* __restrict__ n_valid,
                                                          const float* __restrict__ n_valid2, float* __restrict__ loss_out0,
                                                          float* __restrict__ loss_out1) {
  int split = rows;
  if (n_valid2) {
    const float f = *n_valid;
    split = f >= (float)rows ? rows : (f > 0.f ? (int)f : 0);
  }
  float a0 = 0.f, a1 = 0.f;
  for (int r = threadIdx.x; r < rows; r += 64) {
    const float v = row_loss[r];
    if (r < split) a0 += v; else a1 += v;
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (threadIdx.x == 0) {
    *loss_out0 += a0 / fmaxf(*n_valid, 1.f);
    if (n_valid2) *loss_out1 += a1 / fmaxf(*n_valid2, 1.f);
  }
}

// row validity of the soft-label loss, with the summation order of soft_valid_kernel (loss.hip): the sum decides validity
__global__ __launch_bounds__(256) void soft_valid_f32_kernel(const float* __restrict__ target, long ldt, int C, int rows, float* __restrict__ tsum) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* t = target + (long)row * ldt;
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
  if (lane == 0) tsum[row] = s;
}

__global__ __launch_bounds__(256) void soft_count_f32_kernel(const float* __restrict__ tsum, int rows, float* __restrict__ counts) {
  __shared__ int sh[4];
  int c = 0;
  for (int i = threadIdx.x; i < rows; i += 256) c += (fabsf(tsum[i] - 1.f) < 0.1f) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[0] = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// loss_row = log(s) * sum(t) - sum(t * (x - max)), s = sum exp(x - max);  dlogit_c = (softmax_c * sum(t) - t_c) * gscale / n_valid
// ACC: the maximum pass also takes argmax(x) and, reading the target row there, argmax(t) over [0, C); a valid row where they agree adds 1
// to acc[0]; thread 0 of block 0 adds the valid rows (*n_valid) to acc[1] before its early return.
template <bool ACC>
__device__ __forceinline__ void soft_ce_f32_body(float* __restrict__ logits, long ld, int C, const float* __restrict__ target, long ldt,
                                                 const float* __restrict__ tsum, const float* __restrict__ n_valid, float gscale,
                                                 float* __restrict__ row_loss, float* __restrict__ logits_copy, long ldcopy,
                                                 const float* __restrict__ dscale, vlb_u64* __restrict__ acc) {
  __shared__ float sh[ACC ? 20 : 4];
  const int row = blockIdx.x, ldv = (int)ld;
  if (ACC && dscale) gscale = __fmul_rn(gscale, *dscale);
  if (ACC && row == 0 && threadIdx.x == 0) {
    const vlb_u64 n = (vlb_u64)*n_valid;
    if (n) atomicAdd(acc + 1, n);
  }
  float* x = logits + (long)row * ld;
  const float* t = target + (long)row * ldt;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (logits_copy) {
    float* cp = logits_copy + (long)row * ldcopy;
    for (int c = threadIdx.x * 4; c < ldv && c < (int)ldcopy; c += 1024) {
      float4 v = *(const float4*)(x + c);
      if (c + 1 >= C) v.y = 0.f;
      if (c + 2 >= C) v.z = 0.f;
      if (c + 3 >= C) v.w = 0.f;
      if (c >= C) v.x = 0.f;
      *(float4*)(cp + c) = v;
    }
  }
  const float ts = tsum[row];
  if (!(fabsf(ts - 1.f) < 0.1f)) {
    for (int c = threadIdx.x * 4; c < ldv; c += 1024) *(float4*)(x + c) = zero;
    if (threadIdx.x == 0) row_loss[row] = 0.f;
    return;
  }
  float m = -INFINITY;
  float a = -INFINITY, tm = -INFINITY;
  int xi = INT_MAX, ti = INT_MAX;      // (ACC) ascending columns per thread: `>` keeps the lowest among equals
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const float4 v = *(const float4*)(x + c);
    if (ACC) {
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (c + k < C) {
          const float tv = t[c + k];
          if (vv[k] > a) { a = vv[k]; xi = c + k; }
          if (tv > tm) { tm = tv; ti = c + k; }
        }
      }
    }
    m = fmaxf(m, v.x);
    if (c + 1 < C) m = fmaxf(m, v.y);
    if (c + 2 < C) m = fmaxf(m, v.z);
    if (c + 3 < C) m = fmaxf(m, v.w);
  }
  if (ACC) {
    block_argmax(a, xi, sh + 4);
    block_argmax(tm, ti, sh + 12);
    if (threadIdx.x == 0 && xi == ti) atomicAdd(acc, (vlb_u64)1);
  }
  m = block_max4(m, sh);
  float s = 0.f, dot = 0.f;
  for (int c = threadIdx.x * 4; c < C; c += 1024) {
    const float4 v = *(const float4*)(x + c);
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c + k < C) {
        s += expf(vv[k] - m);
        dot += t[c + k] * (vv[k] - m);
      }
    }
  }
  s = block_sum4(s, sh);
  dot = block_sum4(dot, sh);
  const float inv_s = 1.0f / s;      // (as in ce_f32_kernel: no lse = m + log(s))
  const float nv = fmaxf(*n_valid, 1.f), sc = gscale / nv;
  if (threadIdx.x == 0) row_loss[row] = logf(s) * ts - dot;
  for (int c = threadIdx.x * 4; c < ldv; c += 1024) {
    const float4 v = *(const float4*)(x + c);
    const float vv[4] = {v.x, v.y, v.z, v.w};
    float g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = (c + k < C) ? (expf(vv[k] - m) * inv_s * ts - t[c + k]) * sc : 0.f;
    *(float4*)(x + c) = make_float4(g[0], g[1], g[2], g[3]);
  }
}

__global__ __launch_bounds__(256) void soft_ce_f32_kernel(float* __restrict__ logits, long ld, int C, const float* __restrict__ target, long ldt,
                                                          const float* __restrict__ tsum, const float* __restrict__ n_valid, float gscale,
                                                          float* __restrict__ row_loss, float* __restrict__ logits_copy, long ldcopy) {
  soft_ce_f32_body<false>(logits, ld, C, target, ldt, tsum, n_valid, gscale, row_loss, logits_copy, ldcopy, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void soft_ce_f32_acc_kernel(float* __restrict__ logits, long ld, int C, const float* __restrict__ target,
                                                              long ldt, const float* __restrict__ tsum, const float* __restrict__ n_valid,
                                                              float gscale, float* __restrict__ row_loss, float* __restrict__ logits_copy,
                                                              long ldcopy, const float* __restrict__ dscale, vlb_u64* __restrict__ acc) {
  soft_ce_f32_body<true>(logits, ld, C, target, ldt, tsum, n_valid, gscale, row_loss, logits_copy, ldcopy, dscale, acc);
}

// ------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------
extern "C" int vlb_mask_feature_f32(float* a, const float* boxes, long ldbox, const int64_t* sel, const float* mask_emb, int rows, float drop_p,
                                    const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(a && boxes && sel && mask_emb && ldbox >= 1 && al16(a) && al16(mask_emb), "vlb_mask_feature_f32: null / unaligned argument");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_mask_feature_f32: dropout needs a device seed pointer");
  VLB_CHECK_ARG((long)rows * 4096 < (1L << 32), "vlb_mask_feature_f32: dropout index overflow");
  const uint32_t thr = vlb_drop_thr(drop_p);
  hipLaunchKernelGGL(mask_feature_f32_kernel, dim3(rows), dim3(256), 0, stream, a, boxes, ldbox, sel, mask_emb, thr, vlb_drop_scale(thr), seed, tag);
  VLB_CHECK_LAUNCH("vlb_mask_feature_f32");
  return VLB_OK;
}

extern "C" int vlb_masked_colsum_f32(const float* src, long lds, const int64_t* sel, int rows, int C, float* dst, float drop_p,
                                     const uint32_t* seed, uint32_t tag, uint32_t row_elems, uint32_t col_off, hipStream_t stream) {
  if (rows <= 0 || C <= 0) return VLB_OK;
  VLB_CHECK_ARG(src && sel && dst && (C % 4) == 0 && (lds % 4) == 0 && lds >= C && al16(src), "vlb_masked_colsum_f32: C and lds multiples of 4, 16-byte aligned rows");
  VLB_CHECK_ARG(!(drop_p > 0.f) || (seed && (row_elems % 2) == 0 && (col_off % 2) == 0),
                "vlb_masked_colsum_f32: dropout needs a device seed pointer and even row_elems / col_off");
  VLB_CHECK_ARG(!(drop_p > 0.f) || ((long)rows * row_elems < (1L << 32) && (long)col_off + C <= (long)row_elems),
                "vlb_masked_colsum_f32: dropout index overflow");
  const uint32_t thr = vlb_drop_thr(drop_p);
  hipLaunchKernelGGL(colsum_sel_f32_kernel<false>, dim3(vlb_cdiv(C, 256)), dim3(1024), 0, stream, src, lds, sel, rows, C, dst, (float*)nullptr, thr,
                     vlb_drop_scale(thr), seed, tag, row_elems, col_off);
  VLB_CHECK_LAUNCH("vlb_masked_colsum_f32");
  return VLB_OK;
}

extern "C" int vlb_table2_grad_f32(const float* src, const int64_t* sel, float* dst, int rows, int H, hipStream_t stream) {
  if (rows <= 0 || H <= 0) return VLB_OK;
  VLB_CHECK_ARG(src && sel && dst && (H % 4) == 0 && al16(src), "vlb_table2_grad_f32: H %% 4 == 0, 16-byte aligned rows");
  hipLaunchKernelGGL(colsum_sel_f32_kernel<true>, dim3(vlb_cdiv(H, 256)), dim3(1024), 0, stream, src, (long)H, sel, rows, H, dst + H, dst, 0u, 1.0f,
                     (const uint32_t*)nullptr, 0u, 0u, 0u);
  VLB_CHECK_LAUNCH("vlb_table2_grad_f32");
  return VLB_OK;
}

extern "C" int vlb_select_rows2_f32(const float* table, const int64_t* sel, float* out, int n, int H, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(table && sel && out && H > 0 && (H % 4) == 0 && al16(table) && al16(out), "vlb_select_rows2_f32: H %% 4 == 0, 16-byte aligned pointers");
  hipLaunchKernelGGL(select_rows2_f32_kernel, dim3(vlb_cdiv(n, 4)), dim3(256), 0, stream, table, sel, out, n, H);
  VLB_CHECK_LAUNCH("vlb_select_rows2_f32");
  return VLB_OK;
}

extern "C" int vlb_group_rowsum_f32(const float* src, int groups, int group_rows, int H, float* dst, long ldd, hipStream_t stream) {
  if (groups <= 0 || group_rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(src && dst && H > 0 && (H % 4) == 0 && (ldd % 4) == 0 && ldd >= H && al16(src) && al16(dst),
                "vlb_group_rowsum_f32: H and ldd multiples of 4, 16-byte aligned pointers");
  VLB_CHECK_ARG(groups <= 65535 * 32, "vlb_group_rowsum_f32: too many groups");
  hipLaunchKernelGGL(group_rowsum_f32_kernel, dim3(groups, vlb_cdiv(H, 1024)), dim3(256), 0, stream, src, group_rows, H, dst, ldd);
  VLB_CHECK_LAUNCH("vlb_group_rowsum_f32");
  return VLB_OK;
}

extern "C" int vlb_add_rows_f32(float* dst, long ldd, const float* src, long lds, int rows, int H, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(dst && src && H > 0 && (H % 4) == 0 && (ldd % 4) == 0 && (lds % 4) == 0 && ldd >= H && lds >= H && al16(dst) && al16(src),
                "vlb_add_rows_f32: H and the leading dimensions multiples of 4, 16-byte aligned pointers");
  hipLaunchKernelGGL(add_rows_f32_kernel, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, dst, ldd, src, lds, rows, H);
  VLB_CHECK_LAUNCH("vlb_add_rows_f32");
  return VLB_OK;
}

extern "C" int vlb_gather_rows_f32(const float* src, const int32_t* idx, float* out, int n, int H, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(src && idx && out && H > 0 && (H % 4) == 0 && al16(src) && al16(out), "vlb_gather_rows_f32: H %% 4 == 0, 16-byte aligned pointers");
  hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(vlb_cdiv(n, 4)), dim3(256), 0, stream, src, idx, out, n, H);
  VLB_CHECK_LAUNCH("vlb_gather_rows_f32");
  return VLB_OK;
}

extern "C" int vlb_scatter_rows_f32(const float* src, const int32_t* idx, float* out, int n, int H, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(src && idx && out && H > 0 && (H % 4) == 0 && al16(src) && al16(out), "vlb_scatter_rows_f32: H %% 4 == 0, 16-byte aligned pointers");
  hipLaunchKernelGGL(scatter_rows_f32_kernel, dim3(vlb_cdiv(n, 4)), dim3(256), 0, stream, src, idx, out, n, H);
  VLB_CHECK_LAUNCH("vlb_scatter_rows_f32");
  return VLB_OK;
}

extern "C" int vlb_head_grad_combine_f32(const float* d_text, const float* d_obj, const int32_t* code, float* dx, int B, int T, int R, int S,
                                         int H, hipStream_t stream) {
  if ((long)B * S <= 0) return VLB_OK;
  VLB_CHECK_ARG(code && dx && H > 0 && (H % 4) == 0 && al16(d_text) && al16(d_obj) && al16(dx) && T <= S,
                "vlb_head_grad_combine_f32: H %% 4 == 0, 16-byte aligned pointers, T <= S");
  hipLaunchKernelGGL(head_grad_combine_f32_kernel, dim3(vlb_cdiv((long)B * S, 4)), dim3(256), 0, stream, d_text, d_obj, code, dx, B, T, R, S, H);
  VLB_CHECK_LAUNCH("vlb_head_grad_combine_f32");
  return VLB_OK;
}

// acc (nullable) selects the ACC kernels: [hits, counted rows] added to an int64[2] per group.  dscale (nullable) is theirs alone: the
// plain kernels take no dynamic scale, so dscale without acc is refused.
static int ce_f32_check(const char* name, const float* logits, long ld, int V, const float* logits_copy, long ldcopy, const float* dscale,
                        const int64_t* acc) {
  VLB_CHECK_ARG(!dscale || acc, "%s: dscale needs acc (the kernels without the counters take no dynamic scale)", name);
  VLB_CHECK_ARG(V > 0 && ld >= V && (ld % 4) == 0 && al16(logits), "%s: ld=%ld must be >= V=%d and a multiple of 4, rows 16-byte aligned", name, ld, V);
  VLB_CHECK_ARG(!logits_copy || (ldcopy >= V && (ldcopy % 4) == 0 && al16(logits_copy)), "%s: logits_copy needs ldcopy >= V, ldcopy %% 4 == 0", name);
  return VLB_OK;
}

extern "C" int vlb_ce_f32_fwd_bwd(float* logits, long ld, int rows, int V, const int64_t* labels, float* counts, float gscale,
                                  const float* dscale, float* loss_out, float* row_loss, float* logits_copy, long ldcopy, int64_t* acc,
                                  hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && labels && counts && loss_out && row_loss, "vlb_ce_f32_fwd_bwd: null argument");
  if (ce_f32_check("vlb_ce_f32_fwd_bwd", logits, ld, V, logits_copy, ldcopy, dscale, acc) != VLB_OK) return VLB_ERR_ARG;
  if (acc) {
    hipLaunchKernelGGL(count_labels_f32_acc_kernel, dim3(1), dim3(256), 0, stream, labels, rows, V, counts, (vlb_u64*)acc);
    hipLaunchKernelGGL(ce_f32_acc_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, V, labels, (const float*)counts, (const float*)nullptr,
                       gscale, row_loss, logits_copy, ldcopy, dscale, (vlb_u64*)acc, (vlb_u64*)nullptr);
  } else {
    hipLaunchKernelGGL(count_labels_f32_kernel, dim3(1), dim3(256), 0, stream, labels, rows, counts);
    hipLaunchKernelGGL(ce_f32_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, V, labels, (const float*)counts, (const float*)nullptr,
                       gscale, row_loss, logits_copy, ldcopy);
  }
  hipLaunchKernelGGL(loss_sum_f32_kernel, dim3(1), dim3(64), 0, stream, (const float*)row_loss, rows, (const float*)counts, (const float*)nullptr,
                     loss_out, (float*)nullptr);
  VLB_CHECK_LAUNCH("vlb_ce_f32_fwd_bwd");
  return VLB_OK;
}

extern "C" int vlb_ce_f32_fwd_bwd_compact(float* logits, long ld, int rows, int V, const int64_t* labels_c, const float* count0,
                                          const float* count1, float gscale, const float* dscale, float* loss_out0, float* loss_out1,
                                          float* row_loss, int64_t* acc0, int64_t* acc1, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && labels_c && count0 && count1 && loss_out0 && loss_out1 && row_loss && !acc0 == !acc1,
                "vlb_ce_f32_fwd_bwd_compact: null argument");
  if (ce_f32_check("vlb_ce_f32_fwd_bwd_compact", logits, ld, V, nullptr, 0, dscale, acc0) != VLB_OK) return VLB_ERR_ARG;
  if (acc0)
    hipLaunchKernelGGL(ce_f32_acc_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, V, labels_c, count0, count1, gscale, row_loss,
                       (float*)nullptr, 0L, dscale, (vlb_u64*)acc0, (vlb_u64*)acc1);
  else
    hipLaunchKernelGGL(ce_f32_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, V, labels_c, count0, count1, gscale, row_loss,
                       (float*)nullptr, 0L);
  hipLaunchKernelGGL(loss_sum_f32_kernel, dim3(1), dim3(64), 0, stream, (const float*)row_loss, rows, count0, count1, loss_out0, loss_out1);
  VLB_CHECK_LAUNCH("vlb_ce_f32_fwd_bwd_compact");
  return VLB_OK;
}

extern "C" int vlb_soft_ce_f32_fwd_bwd(float* logits, long ld, int rows, int C, const float* target, long ldt, float* tsum, float* counts,
                                       float gscale, const float* dscale, float* loss_out, float* row_loss, float* logits_copy, long ldcopy,
                                       int64_t* acc, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && target && tsum && counts && loss_out && row_loss && ldt >= C, "vlb_soft_ce_f32_fwd_bwd: null argument or ldt < C");
  if (ce_f32_check("vlb_soft_ce_f32_fwd_bwd", logits, ld, C, logits_copy, ldcopy, dscale, acc) != VLB_OK) return VLB_ERR_ARG;
  hipLaunchKernelGGL(soft_valid_f32_kernel, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, target, ldt, C, rows, tsum);
  hipLaunchKernelGGL(soft_count_f32_kernel, dim3(1), dim3(256), 0, stream, (const float*)tsum, rows, counts);
  if (acc)
    hipLaunchKernelGGL(soft_ce_f32_acc_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, C, target, ldt, (const float*)tsum,
                       (const float*)counts, gscale, row_loss, logits_copy, ldcopy, dscale, (vlb_u64*)acc);
  else
    hipLaunchKernelGGL(soft_ce_f32_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, C, target, ldt, (const float*)tsum,
                       (const float*)counts, gscale, row_loss, logits_copy, ldcopy);
  hipLaunchKernelGGL(loss_sum_f32_kernel, dim3(1), dim3(64), 0, stream, (const float*)row_loss, rows, (const float*)counts, (const float*)nullptr,
                     loss_out, (float*)nullptr);
  VLB_CHECK_LAUNCH("vlb_soft_ce_f32_fwd_bwd");
  return VLB_OK;
}
