// Attention probabilities of the fused 16-bit attention path, written out for inspection (d = 64, 1 <= S <= 512) on gfx950:
// probs[b][h][q][k] = exp(Q.K / 8 + (1 - mask[b][k]) * -10000 - lse[b][h][q]) from the QKV and the row log-sum-exp that
// vlb_attention_fwd left behind -- the same recomputation P = exp(score - lse) as both backward kernels (attention.hip,
// attention_long.hip), forward-only, with fp32 output.  No V, no online softmax, no accumulators across blocks, no atomics: every
// output element is written once by one lane, so the result is deterministic.
//
//  layout     probs is fp32 [B, nh, n, ldp]: queries q < n (n <= S), row stride ldp floats (ldp % 4 == 0, n <= ldp <= 512), head stride
//             n * ldp.  Columns S <= k < ldp are written as exact zeros; nothing outside [b, h, q < n, k < ldp] is touched.
//  kernel     one 8-wave workgroup per (b, h, 128-query block); wave w owns queries 16w..16w+15 of the block, its Q fragments come
//             straight from global memory and the additive mask row of the whole sequence sits in LDS, as in attn_long_fwd_kernel.
//             Key blocks of 128 stream through ONE K image in LDS (row permutation, chunk swizzle and fragments of
//             attention_common.h); one kernel covers the whole range of S.  The transposed tile S^T = K Q^T leaves a lane with 8
//             consecutive keys of one query per 32-key group: 32 B of fp32 output, stored as two 16-B pieces; the four g lanes of a
//             query fill a whole 128-B line together.  Key blocks beyond S (ldp > S rounded up to 128) are zero fill.
//  score      score * scale + maskbias is formed by the same expression as in the forward kernels: for an all-masked sample the
//             scores sit at -10000, where one fp32 ulp is 9.8e-4, and lse was formed from those rounded values.
//  dropout    drop_p > 0: the value is multiplied by keep / (1 - p), keep from the counter RNG (drop8) at element index
//             ((b * nh + h) * S + q) * S + k under the forward's key (seed, tag): the masks the forward applied.  The value written
//             is the fp32 product; the forward rounds that product to the 16-bit type before P.V.
//
// Budgets.  512 threads; the kernel holds one 32-key group's 8 scores at a time: at most 64 VGPRs (58 as compiled: up to 8 waves per
// SIMD = four workgroups per CU by registers; amdgpu_waves_per_eu(4, 4) would let the compiler take 128, it has no use for them);
// LDS 18 KB (one 16 KB image + the 512-entry additive mask).  Nothing spills, no scratch.  The kernel is
// output-bound: QK^T at d = 64 is negligible next to B * nh * n * ldp * 4 bytes of stores.
// Loads.  Every global load is unconditional and clamped (attention_common.h, TileRegs); the next key block's tile is issued right
// after the barrier that publishes the current one and flies under its products and stores.
#include "vlb_common.h"
#include "attention_common.h"

#define ATP_BLK 128                                   // keys / queries per block
#define ATP_TILE_BYTES (ATP_BLK * ATT_D * 2)

struct AttnProbsParams {
  const bf16_t* qkv;   // [B*S, 3H]
  const float* mask;   // [B, S]
  const float* lse;    // [B, nh, S]
  float* probs;        // [B, nh, n, ldp]
  int B, S, H, nh, n, ldp;
  float scale;
  uint32_t drop_thr; float drop_scale; const uint32_t* seed; uint32_t tag;
};

__global__ __launch_bounds__(ATT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_probs_kernel(const AttnProbsParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  float* sMB = (float*)(smem + ATP_TILE_BYTES);       // [512] additive mask of the whole sequence (-inf beyond S)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, n = p.n, ldp = p.ldp;
  const int NB = (S + ATP_BLK - 1) / ATP_BLK;         // key blocks that hold keys
  const int NBP = (ldp + ATP_BLK - 1) / ATP_BLK;      // key blocks that hold output columns (>= NB only when ldp runs past them)
  const int NQ = (n + ATP_BLK - 1) / ATP_BLK;
  const int bh = blockIdx.x / NQ, qb = blockIdx.x % NQ;
  const int b = bh / p.nh, h = bh % p.nh;
  const long ld = 3L * p.H;
  const bf16_t* qbase = p.qkv + (long)b * S * ld + h * ATT_D;
  const bf16_t* kbase = qbase + p.H;
  // prologue burst: the first K block, the Q fragments, lse, the mask row, the seed
  TileRegs<ATP_BLK> rk;
  tile_load<ATP_BLK>(kbase, ld, S, tid, rk);
  const int q0 = qb * ATP_BLK + wave * 16, q = q0 + c, qc = min(q, S - 1);
  uint4 qraw[2];
#pragma unroll
  for (int ds = 0; ds < 2; ++ds) qraw[ds] = *(const uint4*)(qbase + (long)qc * ld + ds * 32 + g * 8);
  const float lse = p.lse[(long)bh * S + qc];
  const float mrow = p.mask[b * S + min(tid, S - 1)];
  const uint32_t seed = (p.drop_thr && p.seed) ? *p.seed : 0u;
  sMB[tid] = (tid < S) ? (1.0f - mrow) * -10000.0f : -INFINITY;
  const bf16x8 qf[2] = {__builtin_bit_cast(bf16x8, qraw[0]), __builtin_bit_cast(bf16x8, qraw[1])};
  const uint32_t key = vlb_rng_key(seed, p.tag);
  const uint32_t qrow = ((uint32_t)bh * (uint32_t)S + (uint32_t)qc) * (uint32_t)S;
  const bool active = q0 < n;                         // wave-uniform: the wave has rows to write (it still stages tiles otherwise)
  float* orow = p.probs + ((long)bh * n + min(q, n - 1)) * ldp;
  const bool wr = q < n;

#pragma unroll 1
  for (int kb = 0; kb < NB; ++kb) {
    const int k0 = kb * ATP_BLK;
    tile_store<ATP_BLK>(rk, S - k0, sK, tid);         // key rows beyond S are zero; their mask entry is -inf
    __syncthreads();
    const int kn = min(kb + 1, NB - 1) * ATP_BLK;     // next block, in flight under this block's products (clamped on the last turn)
    tile_load<ATP_BLK>(kbase + (long)kn * ld, ld, S - kn, tid, rk);
    if (active) {
      const int U = min(4, (S - k0 + 31) >> 5);       // 32-key groups that hold keys
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = k0 + 32 * u + 8 * g;           // this lane's 8 consecutive keys
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
        if (u < U) {
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ds = 0; ds < 2; ++ds) s = VLB_MFMA_16x16x32(frag_perm(sK, u, hf, c, ds * 4 + g), qf[ds], s, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * hf + r] = __expf(s[r] * p.scale + sMB[kk + 4 * hf + r] - lse);
          }
          if (p.drop_thr) drop8(v, key, qrow + (uint32_t)kk, p.drop_thr, p.drop_scale);
        }
        if (wr && kk < ldp) *(float4*)(orow + kk) = make_float4(v[0], v[1], v[2], v[3]);
        if (wr && kk + 4 < ldp) *(float4*)(orow + kk + 4) = make_float4(v[4], v[5], v[6], v[7]);
      }
    }
    __syncthreads();                                  // every wave is done with this block's image
  }
  // output columns beyond the last key block (only when ldp > S rounded up to 128): zeros
  if (wr) {
    for (int kk = NB * ATP_BLK + 8 * g; kk < NBP * ATP_BLK; kk += 32) {
      if (kk < ldp) *(float4*)(orow + kk) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kk + 4 < ldp) *(float4*)(orow + kk + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

extern "C" int vlb_attention_probs(const void* qkv, const float* mask, const float* lse, float* probs, int B, int S, int H, int nh,
                                   int n, int ldp, float drop_p, const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  VLB_CHECK_ARG(B > 0 && S > 0 && S <= ATT_LONG_MAX, "vlb_attention_probs: S=%d unsupported (1..%d)", S, ATT_LONG_MAX);
  VLB_CHECK_ARG(nh > 0 && H == nh * ATT_D, "vlb_attention_probs: head dim must be 64 (H=%d, heads=%d)", H, nh);
  VLB_CHECK_ARG((long)B * nh * S * S < (1L << 32), "vlb_attention_probs: dropout index overflow");
  VLB_CHECK_ARG(n >= 1 && n <= S, "vlb_attention_probs: n=%d outside 1..S=%d", n, S);
  VLB_CHECK_ARG(ldp >= n && ldp <= ATT_LONG_MAX && ldp % 4 == 0, "vlb_attention_probs: ldp=%d must be a multiple of 4 in n=%d..%d",
                ldp, n, ATT_LONG_MAX);
  VLB_CHECK_ARG(qkv && mask && lse && probs, "vlb_attention_probs: null argument");
  VLB_CHECK_ARG(((uintptr_t)probs & 15) == 0, "vlb_attention_probs: probs must be 16-byte aligned (16-byte stores)");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_attention_probs: dropout needs a device seed pointer");
  AttnProbsParams p;
  p.qkv = (const bf16_t*)qkv; p.mask = mask; p.lse = lse; p.probs = probs;
  p.B = B; p.S = S; p.H = H; p.nh = nh; p.n = n; p.ldp = ldp; p.scale = 0.125f;
  p.drop_thr = vlb_drop_thr(drop_p); p.drop_scale = vlb_drop_scale(p.drop_thr); p.seed = seed; p.tag = tag;
  const int NQ = (n + ATP_BLK - 1) / ATP_BLK;
  hipLaunchKernelGGL(attn_probs_kernel, dim3(B * nh * NQ), dim3(ATT_THREADS), ATP_TILE_BYTES + ATT_LONG_MAX * 4, stream, p);
  VLB_CHECK_LAUNCH("vlb_attention_probs");
  return VLB_OK;
}
