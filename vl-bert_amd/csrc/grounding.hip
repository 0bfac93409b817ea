// RefCOCO+ region-grounding head (refcoco/modules/resnet_vlbert_for_refcoco.py:132-160, :206-225): final_mlp = transform (dense +
// erf-GELU, no LayerNorm) -> Dropout -> Linear(H, 1), masked BCE-with-logits, and the inference box pick.  The transform runs on the
// shared gemm_nt (ACT_GELU_D: g = gelu(u) and gelu'(u) saved); everything after it lives here:
//   * vlb_ground_score_fwd  - logit[b,j] = sum_c dropout(g)[r,c] * w2[c] + b2 (one wave per row, dropout on the fly), -10000 beyond max_len
//   * vlb_ground_bce        - masked BCE (mask from the boxes), mean over the valid boxes, d(logit) in the same launch
//   * vlb_ground_score_bwd  - du = g_loss * dlogit * w2 * keep / (1 - p) * gelu'(u) (16-bit), dw2 / db2 (fp32), column slices in a
//                             fixed summation order (no atomics: bitwise reproducible)
//   * vlb_ground_pick_box   - argmax over the padded logits (first index on ties) -> box / (w_ratio, h_ratio)
// None of them reads anything back to the host.
#include "vlb_common.h"

// ---- score forward: one wave per output element (b, j), 4 per block ----
__global__ __launch_bounds__(256) void ground_score_fwd_kernel(const bf16_t* __restrict__ g, long ldg, int H, const float* __restrict__ w2,
                                                               const float* __restrict__ b2, float* __restrict__ logits, long ldo, int B,
                                                               int max_len, int origin_len, uint32_t thr, float scale,
                                                               const uint32_t* __restrict__ seedp, uint32_t tag) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= B * origin_len) return;
  const int b = i / origin_len, j = i - b * origin_len;
  float* out = logits + (long)b * ldo + j;
  if (j >= max_len) {                      // padded back to origin_len with -10000 (:146-149)
    if (lane == 0) *out = -10000.0f;
    return;
  }
  const long r = (long)b * max_len + j;    // row of the [B * max_len, H] transform output
  const uint32_t seed = thr ? *seedp : 0u;
  const uint32_t key = vlb_rng_key(seed, tag);
  const bf16_t* row = g + r * ldg;
  float acc = 0.f;
  for (int c = lane * 8; c < H; c += 512) {
    const uint4 v = *(const uint4*)(row + c);
    const float4 wa = *(const float4*)(w2 + c), wb = *(const float4*)(w2 + c + 4);
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
    const float w[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
    const uint32_t base = (uint32_t)(r * H + c);          // element index of vlb_dropout_bf16 on a contiguous [rows, H] tensor
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float lo = bflo(u[k]), hi = bfhi(u[k]);
      if (thr) {
        const uint32_t h = vlb_pair_hash((base >> 1) + k, key);   // base is even: elements 2k, 2k+1 share one hash
        lo = (h & 0xffffu) >= thr ? lo * scale : 0.f;
        hi = (h >> 16) >= thr ? hi * scale : 0.f;
      }
      acc = fmaf(lo, w[2 * k], acc);
      acc = fmaf(hi, w[2 * k + 1], acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) *out = acc + b2[0];
}

extern "C" int vlb_ground_score_fwd(const void* g, long ldg, int H, const float* w2, const float* b2, float* logits, long ldo, int B,
                                    int max_len, int origin_len, float drop_p, const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  if (B <= 0 || origin_len <= 0) return VLB_OK;
  VLB_CHECK_ARG(g && w2 && b2 && logits && H > 0 && H % 8 == 0 && ldg >= H && ldg % 8 == 0 && max_len >= 0 && max_len <= origin_len &&
                    ldo >= origin_len, "vlb_ground_score_fwd: bad argument");
  VLB_CHECK_ARG((long)B * max_len * H < (1L << 32), "vlb_ground_score_fwd: too many elements for the dropout counter");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_ground_score_fwd: dropout needs a device seed pointer");
  const uint32_t thr = vlb_drop_thr(drop_p);
  hipLaunchKernelGGL(ground_score_fwd_kernel, dim3(vlb_cdiv((long)B * origin_len, 4)), dim3(256), 0, stream, (const bf16_t*)g, ldg, H, w2,
                     b2, logits, ldo, B, max_len, origin_len, thr, vlb_drop_scale(thr), seed, tag);
  VLB_CHECK_LAUNCH("vlb_ground_score_fwd");
  return VLB_OK;
}

// ---- masked BCE: one block of 256 threads; thread t takes rows t, t + 256, ... (fixed order), then a fixed-shape tree ----
__global__ __launch_bounds__(256) void ground_bce_kernel(const float* __restrict__ logits, long ldo, const float* __restrict__ boxes,
                                                         long sbb, long sbr, const float* __restrict__ label, long ldl, int B, int max_len,
                                                         float* __restrict__ loss_out, float* __restrict__ dlogit) {
  __shared__ float sh_loss[4];
  __shared__ int sh_cnt[4];
  const int n = B * max_len;
  float acc = 0.f;
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int b = i / max_len, j = i - b * max_len;
    if (boxes[(long)b * sbb + (long)j * sbr] > -1.5f) {          // box_mask (:83)
      const float x = logits[(long)b * ldo + j], y = label[(long)b * ldl + j];
      acc += fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x)));
      ++cnt;
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  acc = wave_sum(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) {
    sh_loss[wave] = acc;
    sh_cnt[wave] = cnt;
  }
  __syncthreads();
  const int nv = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
  const float total = (sh_loss[0] + sh_loss[1]) + (sh_loss[2] + sh_loss[3]);
  if (threadIdx.x == 0) *loss_out = total / (float)nv;            // 0 / 0 = NaN: torch's mean over an empty selection
  const float inv = nv > 0 ? 1.0f / (float)nv : 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int b = i / max_len, j = i - b * max_len;
    float d = 0.f;
    if (boxes[(long)b * sbb + (long)j * sbr] > -1.5f) {
      const float x = logits[(long)b * ldo + j], y = label[(long)b * ldl + j];
      const float e = __expf(-fabsf(x));
      const float sig = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
      d = (sig - y) * inv;
    }
    dlogit[i] = d;
  }
}

extern "C" int vlb_ground_bce(const float* logits, long ldo, const float* boxes, long sbb, long sbr, const float* label, long ldl, int B,
                              int max_len, float* loss_out, float* dlogit, hipStream_t stream) {
  VLB_CHECK_ARG(logits && boxes && label && loss_out && dlogit && B >= 0 && max_len >= 0 && ldo >= max_len && ldl >= max_len &&
                    sbb >= 0 && sbr >= 0, "vlb_ground_bce: bad argument");
  hipLaunchKernelGGL(ground_bce_kernel, dim3(1), dim3(256), 0, stream, logits, ldo, boxes, sbb, sbr, label, ldl, B, max_len, loss_out,
                     dlogit);
  VLB_CHECK_LAUNCH("vlb_ground_bce");
  return VLB_OK;
}

// ---- score backward: block = 32 columns (4 groups of 8) x 64 row lanes; row lane l takes rows l, l + 64, ... in order, and the
// 64 partial column sums are added in a fixed order through LDS.  Grid = ceil(H / 32) blocks: every output written by one thread. ----
#define GSB_COLS 32
#define GSB_LANES 64
__global__ __launch_bounds__(256) void ground_score_bwd_kernel(const float* __restrict__ gscale, const float* __restrict__ dlogit, int rows,
                                                               const bf16_t* __restrict__ g, long ldg, const bf16_t* __restrict__ dgelu,
                                                               long ldd, int H, const float* __restrict__ w2, bf16_t* __restrict__ du,
                                                               long lddu, float* __restrict__ dw2, float* __restrict__ db2, uint32_t thr,
                                                               float scale, const uint32_t* __restrict__ seedp, uint32_t tag) {
  __shared__ float sh[GSB_LANES][GSB_COLS + 1];
  __shared__ float shb[GSB_LANES];
  const int grp = threadIdx.x & 3, lr = threadIdx.x >> 2;
  const int c = blockIdx.x * GSB_COLS + grp * 8;
  const bool active = c < H;
  const float gs = *gscale;
  const uint32_t seed = thr ? *seedp : 0u;
  const uint32_t key = vlb_rng_key(seed, tag);
  float w[8], acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    w[k] = active ? w2[c + k] : 0.f;
    acc[k] = 0.f;
  }
  float accb = 0.f;
  if (active) {
    for (int r = lr; r < rows; r += GSB_LANES) {
      const float s = gs * dlogit[r];
      accb += s;
      const uint4 v = *(const uint4*)(g + (long)r * ldg + c);
      const uint4 dv = *(const uint4*)(dgelu + (long)r * ldd + c);
      const uint32_t u[4] = {v.x, v.y, v.z, v.w}, du_[4] = {dv.x, dv.y, dv.z, dv.w};
      const uint32_t base = (uint32_t)((long)r * H + c);
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float mlo = 1.f, mhi = 1.f;
        if (thr) {
          const uint32_t h = vlb_pair_hash((base >> 1) + k, key);
          mlo = (h & 0xffffu) >= thr ? scale : 0.f;
          mhi = (h >> 16) >= thr ? scale : 0.f;
        }
        acc[2 * k] = fmaf(s, bflo(u[k]) * mlo, acc[2 * k]);
        acc[2 * k + 1] = fmaf(s, bfhi(u[k]) * mhi, acc[2 * k + 1]);
        o[k] = pack2bf(s * w[2 * k] * mlo * bflo(du_[k]), s * w[2 * k + 1] * mhi * bfhi(du_[k]));
      }
      *(uint4*)(du + (long)r * lddu + c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[lr][grp * 8 + k] = acc[k];
  if (grp == 0) shb[lr] = accb;
  __syncthreads();
  if (threadIdx.x < GSB_COLS) {             // column threadIdx.x of the slice: 64 row-lane partials, in row-lane order
    float t = 0.f;
    for (int l = 0; l < GSB_LANES; ++l) t += sh[l][threadIdx.x];
    const int col = blockIdx.x * GSB_COLS + threadIdx.x;
    if (col < H) dw2[col] = t;
  } else if (threadIdx.x == GSB_COLS && blockIdx.x == 0) {
    float t = 0.f;
    for (int l = 0; l < GSB_LANES; ++l) t += shb[l];
    db2[0] = t;
  }
}

extern "C" int vlb_ground_score_bwd(const float* gscale, const float* dlogit, int rows, const void* g, long ldg, const void* dgelu, long ldd,
                                    int H, const float* w2, void* du, long lddu, float* dw2, float* db2, float drop_p, const uint32_t* seed,
                                    uint32_t tag, hipStream_t stream) {
  VLB_CHECK_ARG(gscale && dlogit && g && dgelu && w2 && du && dw2 && db2 && rows >= 0 && H > 0 && H % 8 == 0 && ldg >= H && ldd >= H &&
                    lddu >= H && ldg % 8 == 0 && ldd % 8 == 0 && lddu % 8 == 0, "vlb_ground_score_bwd: bad argument");
  VLB_CHECK_ARG((long)rows * H < (1L << 32), "vlb_ground_score_bwd: too many elements for the dropout counter");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_ground_score_bwd: dropout needs a device seed pointer");
  const uint32_t thr = vlb_drop_thr(drop_p);
  hipLaunchKernelGGL(ground_score_bwd_kernel, dim3(vlb_cdiv(H, GSB_COLS)), dim3(256), 0, stream, gscale, dlogit, rows, (const bf16_t*)g, ldg,
                     (const bf16_t*)dgelu, ldd, H, w2, (bf16_t*)du, lddu, dw2, db2, thr, vlb_drop_scale(thr), seed, tag);
  VLB_CHECK_LAUNCH("vlb_ground_score_bwd");
  return VLB_OK;
}

// ---- inference box pick: one wave per sample ----
__device__ __forceinline__ bool ground_better(float a, int ia, float b, int ib) {   // torch.argmax order: NaN is the largest, then first index
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ia < ib);
  return a > b || (a == b && ia < ib);
}

__global__ __launch_bounds__(64) void ground_pick_box_kernel(const float* __restrict__ logits, long ldo, int origin_len,
                                                             const float* __restrict__ boxes, long sbb, long sbr,
                                                             const float* __restrict__ im_info, long ldi, float* __restrict__ pred,
                                                             int64_t* __restrict__ idx_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* row = logits + (long)b * ldo;
  float best = 0.f;
  int bi = -1;
  for (int j = lane; j < origin_len; j += 64) {
    const float v = row[j];
    if (bi < 0 || ground_better(v, j, best, bi)) {
      best = v;
      bi = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi >= 0 && (bi < 0 || ground_better(ov, oi, best, bi))) {
      best = ov;
      bi = oi;
    }
  }
  if (lane < 4) {
    const float* box = boxes + (long)b * sbb + (long)bi * sbr;
    const float ratio = im_info[(long)b * ldi + 2 + (lane & 1)];      // x1, x2 / w_ratio; y1, y2 / h_ratio (:219-222)
    pred[b * 4 + lane] = box[lane] / ratio;
  }
  if (lane == 0 && idx_out) idx_out[b] = bi;
}

extern "C" int vlb_ground_pick_box(const float* logits, long ldo, int B, int origin_len, const float* boxes, long sbb, long sbr,
                                   const float* im_info, long ldi, float* pred_boxes, int64_t* idx, hipStream_t stream) {
  if (B <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && boxes && im_info && pred_boxes && origin_len > 0 && ldo >= origin_len && sbr >= 4 && ldi >= 4,
                "vlb_ground_pick_box: bad argument");
  hipLaunchKernelGGL(ground_pick_box_kernel, dim3(B), dim3(64), 0, stream, logits, ldo, origin_len, boxes, sbb, sbr, im_info, ldi,
                     pred_boxes, idx);
  VLB_CHECK_LAUNCH("vlb_ground_pick_box");
  return VLB_OK;
}
