// Fused multi-head self-attention forward / backward for 256 < S <= 512 (d = 64) on gfx950: the same BertSelfAttention semantics as
// attention.hip (scores = Q K^T / 8 + (1-mask)*-10000, softmax, dropout on P, ctx = P V, lse = logsumexp(scores)), for sequences
// whose S x S tile no longer fits one workgroup's registers and whose four head images no longer fit LDS.  Blocks of 128 keys (or 128
// queries) STREAM through two 16 KB LDS images; the operand plan is that of attention.hip / attention_common.h: row-major images at
// permuted rows rho(s), chunk swizzle, transposed score tiles S^T = K Q^T, V^T / K^T / Q^T / dO^T through ds_read_b64_tr_b16.
//
//  forward    one 8-wave workgroup per (b, h, 128-query block); wave w owns queries 16w..16w+15 of the block, its Q fragments come
//             straight from global memory.  Key blocks of 128 pass through the K | V images; per block the wave forms the 128 x 16
//             score slice (32 VGPRs), updates the running maximum m and sum l of its queries (online softmax), rescales the fp32
//             ctx^T accumulators by exp(m_old - m_new) and adds V^T P~^T with P~ = exp(score - m_new) x keep x 1/(1-p) rounded to
//             the 16-bit type.  At the end ctx = acc / l and lse = m + log l (l, lse: of the un-dropped P).
//             m starts at a large negative FINITE number: key 0 is always a real key, so the first block's maximum is finite (about
//             -10000 when all its keys are masked) and exp(m_old - m_new) is exp(-huge) = 0 with no inf - inf; when a later block
//             holds the first live key, the factor exp(-10000 - m_new) underflows to 0 the same way and the masked keys vanish as in
//             the reference's fp32 softmax.  Padding rows (index >= S, last block only) carry an additive -inf: exp gives 0 exactly.
//  backward   two launches on the same stream, deterministic, no workspace, no atomics:
//    role A   one workgroup per (b, h, 128-KEY block): wave w keeps K and V of its 16 keys as B operands (from global memory) and
//             dK^T, dV^T in 32 accumulator registers while blocks of 128 queries pass through the Q | dO images (+ lse and
//             D = rowsum(dO o O) of the block in LDS, D from the saved 16-bit ctx).  S = Q K^T and dP = dO V^T with the key on the
//             lane, P = exp(score - lse), Pd = P x keep, dS = P (dP x keep - D), both rounded to the 16-bit type, then
//             dV^T += dO^T Pd, dK^T += Q^T dS.
//    role B   one workgroup per (b, h, 128-QUERY block): wave w keeps Q, dO (B operands), lse and D of its 16 queries while blocks
//             of 128 keys pass through the K | V images: S^T = K Q^T, dP^T = V dO^T, dS^T, dQ^T += K^T dS^T.
//             Seven products per tile pair instead of the five of a kernel that sees the whole tile: the price of needing no sum
//             across workgroups.  Only batches longer than 256 positions take this path.
//
// Budgets.  All three kernels: 512 threads and amdgpu_waves_per_eu(4, 4) -> at most 128 VGPRs, two 8-wave workgroups (4 waves per
// SIMD) per CU; LDS 34 KB (forward, role B: two 16 KB images + the 512-entry additive mask) / 33 KB (role A: two images + lse + D of
// a query block), so LDS never limits residency below the two workgroups the register budget allows.  Nothing spills, no scratch.
// Loads.  Every global load is unconditional and clamped (attention_common.h, TileRegs).  Forward and role B issue the next block's
// tiles right after the barrier that publishes the current block; they fly under its MFMAs and are written to LDS at the top of the
// next turn (the turn after the last block re-reads the last block, clamped index, instead of branching around the loads).  Role A
// loads each query block in one burst at the top of its turn: holding 25 more registers across the products put it over 128 VGPRs.
#include "vlb_common.h"
#include "attention_common.h"

#define ATL_BLK 128                                   // keys / queries per streamed block
#define ATL_TILE_BYTES (ATL_BLK * ATT_D * 2)
// 8-wave workgroups, exactly 4 waves per SIMD = two workgroups per CU: the register allocator may use up to 128 VGPRs and no more
#define ATL_KERNEL __global__ __launch_bounds__(ATT_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))

// B-operand fragments of 16 consecutive rows straight from global memory: lane (c, g) <- X[row][32 ds + 8 g .. + 8)
__device__ __forceinline__ void load_rows16(const bf16_t* __restrict__ base, long ld, int row, int g, uint4* f) {
#pragma unroll
  for (int ds = 0; ds < 2; ++ds) f[ds] = *(const uint4*)(base + (long)row * ld + ds * 32 + g * 8);
}

__device__ __forceinline__ float dot8(const uint4& a, const uint4& o) {
  return bflo(a.x) * bflo(o.x) + bfhi(a.x) * bfhi(o.x) + bflo(a.y) * bflo(o.y) + bfhi(a.y) * bfhi(o.y) +
         bflo(a.z) * bflo(o.z) + bfhi(a.z) * bfhi(o.z) + bflo(a.w) * bflo(o.w) + bfhi(a.w) * bfhi(o.w);
}

// =============================================================================================
// forward
// =============================================================================================
ATL_KERNEL void attn_long_fwd_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + ATL_TILE_BYTES;
  float* sMB = (float*)(smem + 2 * ATL_TILE_BYTES);   // [512] additive mask of the whole sequence (-inf beyond S)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, NB = (S + ATL_BLK - 1) / ATL_BLK;
  const int bh = blockIdx.x / NB, qb = blockIdx.x % NB;
  const int b = bh / p.nh, h = bh % p.nh;
  const long ld = 3L * p.H;
  const bf16_t* qbase = p.qkv + (long)b * S * ld + h * ATT_D;
  const bf16_t* kbase = qbase + p.H;
  const bf16_t* vbase = qbase + 2 * p.H;
  // prologue burst: first K and V blocks, the Q fragments, the mask row, the seed
  TileRegs<ATL_BLK> rk, rv;
  tile_load<ATL_BLK>(kbase, ld, S, tid, rk);
  tile_load<ATL_BLK>(vbase, ld, S, tid, rv);
  const int q0 = qb * ATL_BLK + wave * 16, q = q0 + c, qc = min(q, S - 1);
  uint4 qraw[2];
  load_rows16(qbase, ld, qc, g, qraw);
  const float mrow = p.mask[b * S + min(tid, S - 1)];
  const uint32_t seed = (p.drop_thr && p.seed) ? *p.seed : 0u;
  sMB[tid] = (tid < S) ? (1.0f - mrow) * -10000.0f : -INFINITY;
  const bf16x8 qf[2] = {__builtin_bit_cast(bf16x8, qraw[0]), __builtin_bit_cast(bf16x8, qraw[1])};
  const uint32_t key = vlb_rng_key(seed, p.tag);
  const uint32_t qrow = ((uint32_t)bh * (uint32_t)S + (uint32_t)qc) * (uint32_t)S;
  const bool active = q0 < S;                         // wave-uniform: the wave's 16 queries exist (it still stages tiles otherwise)

  float m_run = -3.0e38f, l_run = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int kb = 0; kb < NB; ++kb) {
    const int k0 = kb * ATL_BLK;
    tile_store<ATL_BLK>(rk, S - k0, sK, tid);
    tile_store<ATL_BLK>(rv, S - k0, sV, tid);
    __syncthreads();
    const int kn = min(kb + 1, NB - 1) * ATL_BLK;     // next block, in flight under this block's products (clamped on the last turn)
    tile_load<ATL_BLK>(kbase + (long)kn * ld, ld, S - kn, tid, rk);
    tile_load<ATL_BLK>(vbase + (long)kn * ld, ld, S - kn, tid, rv);
    if (active) {
      const int U = min(4, (S - k0 + 31) >> 5);       // 32-key blocks present in this block
      f32x4 sc[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          sc[u][hf] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (u < U) {
#pragma unroll
            for (int ds = 0; ds < 2; ++ds)
              sc[u][hf] = VLB_MFMA_16x16x32(frag_perm(sK, u, hf, c, ds * 4 + g), qf[ds], sc[u][hf], 0, 0, 0);
          }
        }
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = (u < U) ? sc[u][hf][r] * p.scale + sMB[k0 + 32 * u + 8 * g + 4 * hf + r] : -INFINITY;
            sc[u][hf][r] = v;
            mx = fmaxf(mx, v);
          }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);           // finite: m_run is, and every block holds at least one real key
      const float alpha = __expf(m_run - m_new);      // 0 on the first block and whenever the old keys were all masked
      float sum = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = __expf(sc[u][hf][r] - m_new);
            sc[u][hf][r] = e;
            sum += e;
          }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      l_run = l_run * alpha + sum;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
      bf16x8 pf[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v[8];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[4 * hf + r] = sc[u][hf][r];
        if (p.drop_thr) drop8(v, key, qrow + (uint32_t)(k0 + 32 * u + 8 * g), p.drop_thr, p.drop_scale);
        pf[u] = pack8(v);
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (u < U) o[dt] = VLB_MFMA_16x16x32(frag_tr(sV, u, dt * 16, lane), pf[u], o[dt], 0, 0, 0);
    }
    __syncthreads();                                  // every wave is done with this block's images
  }
  if (active && q < S) {
    const float inv = 1.0f / l_run;
    if (g == 0) p.lse[(long)bh * S + q] = m_run + __logf(l_run);
    bf16_t* orow = p.ctx + ((long)b * S + q) * p.H + h * ATT_D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *(uint2*)(orow + dt * 16) = make_uint2(pack2bf(o[dt][0] * inv, o[dt][1] * inv), pack2bf(o[dt][2] * inv, o[dt][3] * inv));
  }
}

// =============================================================================================
// backward, role A: dK, dV of a 128-key block; query blocks stream
// =============================================================================================
ATL_KERNEL void attn_long_bwd_kv_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sQ = smem;
  char* sdO = smem + ATL_TILE_BYTES;
  float* sLSE = (float*)(smem + 2 * ATL_TILE_BYTES);  // [128] of the current query block (0 beyond S)
  float* sD = sLSE + ATL_BLK;                         // [128] rowsum(dO * O)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, NB = (S + ATL_BLK - 1) / ATL_BLK;
  const int bh = blockIdx.x / NB, kblk = blockIdx.x % NB;
  const int b = bh / p.nh, h = bh % p.nh;
  const long ld = 3L * p.H;
  const bf16_t* qbase = p.qkv + (long)b * S * ld + h * ATT_D;
  const bf16_t* dobase = p.dctx + (long)b * S * p.H + h * ATT_D;
  const bf16_t* obase = p.ctx + (long)b * S * p.H + h * ATT_D;
  const float* lbase = p.lse + (long)bh * S;
  // prologue burst: this wave's K and V rows, its keys' mask, the seed -- and, behind them, the first query block's loads
  const int w16 = kblk * ATL_BLK + wave * 16, pos = w16 + c, posc = min(pos, S - 1);
  uint4 kraw[2], vraw[2];
  load_rows16(qbase + p.H, ld, posc, g, kraw);
  load_rows16(qbase + 2 * p.H, ld, posc, g, vraw);
  const float mkey = p.mask[b * S + posc];
  const uint32_t seed = (p.drop_thr && p.seed) ? *p.seed : 0u;
  const bf16x8 kf[2] = {__builtin_bit_cast(bf16x8, kraw[0]), __builtin_bit_cast(bf16x8, kraw[1])};
  const bf16x8 vf[2] = {__builtin_bit_cast(bf16x8, vraw[0]), __builtin_bit_cast(bf16x8, vraw[1])};
  const float mb = (pos < S) ? (1.0f - mkey) * -10000.0f : -INFINITY;   // a key beyond S: P = exp(-inf) = 0
  const uint32_t key = vlb_rng_key(seed, p.tag);
  const bool active = w16 < S;

  f32x4 dv[4], dk[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dv[dt] = dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int qb = 0; qb < NB; ++qb) {
    const int q0 = qb * ATL_BLK;
    // one burst per query block: Q, dO, O tiles and the lse row.  (Not prefetched under the previous block's products as in the
    // other two kernels: 25 more live registers put this kernel over 128 VGPRs; the co-resident workgroup covers the wait.)
    TileRegs<ATL_BLK> rq, rdo, ro;
    tile_load<ATL_BLK>(qbase + (long)q0 * ld, ld, S - q0, tid, rq);
    tile_load<ATL_BLK>(dobase + (long)q0 * p.H, p.H, S - q0, tid, rdo);
    tile_load<ATL_BLK>(obase + (long)q0 * p.H, p.H, S - q0, tid, ro);
    const float lrow = lbase[min(q0 + (tid & (ATL_BLK - 1)), S - 1)];
    tile_store<ATL_BLK>(rq, S - q0, sQ, tid);         // query rows beyond S are zero: they add nothing to the sums over queries
    tile_store<ATL_BLK>(rdo, S - q0, sdO, tid);
    rowdot_store<ATL_BLK>(rdo, ro, S - q0, sD, tid);
    if (tid < ATL_BLK) sLSE[tid] = (q0 + tid < S) ? lrow : 0.f;
    __syncthreads();
    if (active) {
      const int V = min(4, (S - q0 + 31) >> 5);       // 32-query blocks present in this block
#pragma unroll 1
      for (int v = 0; v < V; ++v) {
        float pv[8], dsv[8];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ds = 0; ds < 2; ++ds) {
            s = VLB_MFMA_16x16x32(frag_perm(sQ, v, hf, c, ds * 4 + g), kf[ds], s, 0, 0, 0);
            dp = VLB_MFMA_16x16x32(frag_perm(sdO, v, hf, c, ds * 4 + g), vf[ds], dp, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ql = 32 * v + 8 * g + 4 * hf + r;
            const float pr = __expf(s[r] * p.scale + mb - sLSE[ql]);
            float keepf = 1.f;
            if (p.drop_thr) {
              const uint32_t idx = ((uint32_t)bh * (uint32_t)S + (uint32_t)min(q0 + ql, S - 1)) * (uint32_t)S + (uint32_t)posc;
              const uint32_t hsh = vlb_pair_hash(idx >> 1, key);
              keepf = (((idx & 1u) ? (hsh >> 16) : (hsh & 0xffffu)) >= p.drop_thr) ? p.drop_scale : 0.f;
            }
            pv[4 * hf + r] = pr * keepf;
            dsv[4 * hf + r] = pr * (dp[r] * keepf - sD[ql]);
          }
        }
        const bf16x8 pd = pack8(pv), dsf = pack8(dsv);   // operands: col = key c, k = query 32v + 8g + j
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[dt] = VLB_MFMA_16x16x32(frag_tr(sdO, v, dt * 16, lane), pd, dv[dt], 0, 0, 0);
          dk[dt] = VLB_MFMA_16x16x32(frag_tr(sQ, v, dt * 16, lane), dsf, dk[dt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (active && pos < S) {
    bf16_t* orow = p.dqkv + ((long)b * S + pos) * ld + h * ATT_D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *(uint2*)(orow + p.H + dt * 16) = make_uint2(pack2bf(dk[dt][0] * p.scale, dk[dt][1] * p.scale),
                                                   pack2bf(dk[dt][2] * p.scale, dk[dt][3] * p.scale));
      *(uint2*)(orow + 2 * p.H + dt * 16) = make_uint2(pack2bf(dv[dt][0], dv[dt][1]), pack2bf(dv[dt][2], dv[dt][3]));
    }
  }
}

// =============================================================================================
// backward, role B: dQ of a 128-query block; key blocks stream
// =============================================================================================
ATL_KERNEL void attn_long_bwd_q_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + ATL_TILE_BYTES;
  float* sMB = (float*)(smem + 2 * ATL_TILE_BYTES);   // [512]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int S = p.S, NB = (S + ATL_BLK - 1) / ATL_BLK;
  const int bh = blockIdx.x / NB, qb = blockIdx.x % NB;
  const int b = bh / p.nh, h = bh % p.nh;
  const long ld = 3L * p.H;
  const bf16_t* qbase = p.qkv + (long)b * S * ld + h * ATT_D;
  const bf16_t* kbase = qbase + p.H;
  const bf16_t* vbase = qbase + 2 * p.H;
  // prologue burst: first K and V blocks, this wave's Q, dO and O rows, lse, the mask row, the seed
  TileRegs<ATL_BLK> rk, rv;
  tile_load<ATL_BLK>(kbase, ld, S, tid, rk);
  tile_load<ATL_BLK>(vbase, ld, S, tid, rv);
  const int q0 = qb * ATL_BLK + wave * 16, q = q0 + c, qc = min(q, S - 1);
  uint4 qraw[2], doraw[2], oraw[2];
  load_rows16(qbase, ld, qc, g, qraw);
  load_rows16(p.dctx + (long)b * S * p.H + h * ATT_D, p.H, qc, g, doraw);
  load_rows16(p.ctx + (long)b * S * p.H + h * ATT_D, p.H, qc, g, oraw);
  const float lse = p.lse[(long)bh * S + qc];
  const float mrow = p.mask[b * S + min(tid, S - 1)];
  const uint32_t seed = (p.drop_thr && p.seed) ? *p.seed : 0u;
  sMB[tid] = (tid < S) ? (1.0f - mrow) * -10000.0f : -INFINITY;
  const bf16x8 qf[2] = {__builtin_bit_cast(bf16x8, qraw[0]), __builtin_bit_cast(bf16x8, qraw[1])};
  const bf16x8 dof[2] = {__builtin_bit_cast(bf16x8, doraw[0]), __builtin_bit_cast(bf16x8, doraw[1])};
  float dd = dot8(doraw[0], oraw[0]) + dot8(doraw[1], oraw[1]);   // D[q]: this lane's 16 of the 64 columns, then across g
  dd += __shfl_xor(dd, 16, 64);
  dd += __shfl_xor(dd, 32, 64);
  const uint32_t key = vlb_rng_key(seed, p.tag);
  const uint32_t qrow = ((uint32_t)bh * (uint32_t)S + (uint32_t)qc) * (uint32_t)S;
  const bool active = q0 < S;

  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int kb = 0; kb < NB; ++kb) {
    const int k0 = kb * ATL_BLK;
    tile_store<ATL_BLK>(rk, S - k0, sK, tid);
    tile_store<ATL_BLK>(rv, S - k0, sV, tid);
    __syncthreads();
    const int kn = min(kb + 1, NB - 1) * ATL_BLK;
    tile_load<ATL_BLK>(kbase + (long)kn * ld, ld, S - kn, tid, rk);
    tile_load<ATL_BLK>(vbase + (long)kn * ld, ld, S - kn, tid, rv);
    if (active) {
      const int U = min(4, (S - k0 + 31) >> 5);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < U) {
          float pr[8], dpv[8];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ds = 0; ds < 2; ++ds) {
              s = VLB_MFMA_16x16x32(frag_perm(sK, u, hf, c, ds * 4 + g), qf[ds], s, 0, 0, 0);
              dp = VLB_MFMA_16x16x32(frag_perm(sV, u, hf, c, ds * 4 + g), dof[ds], dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              pr[4 * hf + r] = __expf(s[r] * p.scale + sMB[k0 + 32 * u + 8 * g + 4 * hf + r] - lse);
              dpv[4 * hf + r] = dp[r];
            }
          }
          if (p.drop_thr) drop8(dpv, key, qrow + (uint32_t)(k0 + 32 * u + 8 * g), p.drop_thr, p.drop_scale);   // dP = dPd * keep * scale
          float dsv[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) dsv[j] = pr[j] * (dpv[j] - dd);
          const bf16x8 dsf = pack8(dsv);
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            dq[dt] = VLB_MFMA_16x16x32(frag_tr(sK, u, dt * 16, lane), dsf, dq[dt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (active && q < S) {
    bf16_t* orow = p.dqkv + ((long)b * S + q) * ld + h * ATT_D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *(uint2*)(orow + dt * 16) = make_uint2(pack2bf(dq[dt][0] * p.scale, dq[dt][1] * p.scale),
                                             pack2bf(dq[dt][2] * p.scale, dq[dt][3] * p.scale));
  }
}

// ---------------------------------------------------------------------------------- launchers (arguments checked by the C ABI in attention.hip)
void vlb_attention_long_fwd_launch(const AttnParams& p, hipStream_t stream) {
  const int NB = (p.S + ATL_BLK - 1) / ATL_BLK;
  const int smem = 2 * ATL_TILE_BYTES + ATT_LONG_MAX * 4;
  hipLaunchKernelGGL(attn_long_fwd_kernel, dim3(p.B * p.nh * NB), dim3(ATT_THREADS), smem, stream, p);
}

void vlb_attention_long_bwd_launch(const AttnParams& p, hipStream_t stream) {
  const int NB = (p.S + ATL_BLK - 1) / ATL_BLK;
  hipLaunchKernelGGL(attn_long_bwd_kv_kernel, dim3(p.B * p.nh * NB), dim3(ATT_THREADS), 2 * ATL_TILE_BYTES + 2 * ATL_BLK * 4, stream, p);
  hipLaunchKernelGGL(attn_long_bwd_q_kernel, dim3(p.B * p.nh * NB), dim3(ATT_THREADS), 2 * ATL_TILE_BYTES + ATT_LONG_MAX * 4, stream, p);
}
