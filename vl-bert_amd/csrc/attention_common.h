// Shared by attention.hip (S <= 256: the whole sequence of one (sample, head) in LDS) and attention_long.hip (256 < S <= 512: key /
// query blocks of 128 streamed through the same images): LDS image addressing, MFMA operand fragments, tile staging, the dropout
// keep-mask of 8 consecutive elements and the kernel parameter block.  See the header of attention.hip for the operand plan.
#pragma once
#include "vlb_common.h"

#define ATT_SP_MAX 256  // longest padded sequence one workgroup handles (template NU = SP / 32 key blocks: 4 or 8)
#define ATT_LONG_MAX 512  // longest sequence of the streaming kernels (attention_long.hip)
#define ATT_D 64
#define ATT_THREADS 512

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// ---- LDS image addressing ------------------------------------------------------------------
__device__ __forceinline__ int rho(int s) { return (s & ~31) | (((s >> 2) & 1) << 4) | (((s >> 3) & 3) << 2) | (s & 3); }
// byte address of 16-B chunk `chunk` (0..7) of LDS row `row`
__device__ __forceinline__ int rm_addr(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ bf16x8 lds_frag(const char* base, int addr) { return *(const bf16x8*)(base + addr); }

// A-operand fragment in permuted order: tile (blk32, half) = LDS rows 32*blk + 16*half + [0..16)
__device__ __forceinline__ bf16x8 frag_perm(const char* img, int blk, int half, int c, int chunk) {
  return lds_frag(img, rm_addr(32 * blk + 16 * half + c, chunk));
}
// B-operand fragment for 16 consecutive sequence positions s0..s0+15 (lane c -> position s0+c)
__device__ __forceinline__ bf16x8 frag_nat(const char* img, int s0, int c, int chunk) {
  return lds_frag(img, rm_addr(rho(s0 + c), chunk));
}
// Transposed fragment: lane (i = L, g) <- X[seq 32*blk + 8g + j][d0 + L], j = 0..7   (two ds_read_b64_tr_b16)
__device__ __forceinline__ bf16x8 frag_tr(const char* img, int blk, int d0, int lane) {
  const int L = lane & 15, g = lane >> 4;
  const int b = d0 * 2 + (L & 3) * 8;                    // byte offset of this lane's 4 columns inside the row
  const int r_lo = 32 * blk + 4 * g + (L >> 2);          // rho of keys 8g+0..3 ; +16 for keys 8g+4..7
  const int r_hi = r_lo + 16;
  const int a_lo = r_lo * 128 + ((((b >> 4) ^ ((r_lo >> 1) & 7)) << 4) | (b & 15));
  const int a_hi = r_hi * 128 + ((((b >> 4) ^ ((r_hi >> 1) & 7)) << 4) | (b & 15));
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + a_lo));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + a_hi));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// Staging of [S][64] head slices (row stride ld elements) into row-major LDS images at permuted rows, rows >= S zero -- in TWO steps,
// so that a kernel issues the global loads of ALL its tiles (and whatever else its prologue reads) before the first wait.  The loads
// are unconditional: a row index beyond the sequence is clamped to the last row and the value replaced by zeros afterwards.  (With a
// load under `if (s < S)` hipcc branches around every single load and waits vmcnt(0) behind it: the prologue of the backward kernel
// was ten dependent HBM round trips, 65 % of its wave cycles parked -- profiles/r03_gemm_pmc.txt, attn_bwd2_kernel.)
template <int SP>
struct TileRegs {
  uint4 v[SP * 8 / ATT_THREADS];
};

template <int SP>
__device__ __forceinline__ void tile_load(const bf16_t* __restrict__ g, long ld, int S, int tid, TileRegs<SP>& r) {
#pragma unroll
  for (int it = 0; it < SP * 8 / ATT_THREADS; ++it) {
    const int P = it * ATT_THREADS + tid, s = min(P >> 3, S - 1), ch = P & 7;
    r.v[it] = *(const uint4*)(g + (long)s * ld + ch * 8);
  }
}

template <int SP>
__device__ __forceinline__ void tile_store(const TileRegs<SP>& r, int S, char* img, int tid) {
#pragma unroll
  for (int it = 0; it < SP * 8 / ATT_THREADS; ++it) {
    const int P = it * ATT_THREADS + tid, s = P >> 3, ch = P & 7;
    const bool in = s < S;
    const uint4 v = make_uint4(in ? r.v[it].x : 0u, in ? r.v[it].y : 0u, in ? r.v[it].z : 0u, in ? r.v[it].w : 0u);
    *(uint4*)(img + rm_addr(rho(s), ch)) = v;
  }
}

// D[q] = sum_d dO[q][d] * O[q][d] from the staged dO chunks and the matching O chunks (8 lanes per row, 8 elements each)
template <int SP>
__device__ __forceinline__ void rowdot_store(const TileRegs<SP>& a_, const TileRegs<SP>& o_, int S, float* sD, int tid) {
#pragma unroll
  for (int it = 0; it < SP * 8 / ATT_THREADS; ++it) {
    const int P = it * ATT_THREADS + tid, row = P >> 3, ch = P & 7;
    const uint4 a = a_.v[it], o = o_.v[it];
    float d = bflo(a.x) * bflo(o.x) + bfhi(a.x) * bfhi(o.x) + bflo(a.y) * bflo(o.y) + bfhi(a.y) * bfhi(o.y) +
              bflo(a.z) * bflo(o.z) + bfhi(a.z) * bfhi(o.z) + bflo(a.w) * bflo(o.w) + bfhi(a.w) * bfhi(o.w);
    d = row < S ? d : 0.f;
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    if (ch == 0) sD[row] = d;
  }
}

__device__ __forceinline__ bf16x8 pack8(const float* v) {
  uint32_t w[4] = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
  return __builtin_bit_cast(bf16x8, *(uint4*)w);
}

// keep-mask x scale for 8 consecutive element indices base..base+7 (any parity): the RNG yields one 32-bit hash per
// PAIR of elements (idx>>1), 16 bits each -- 5 hashes cover the (at most) 5 pairs the run of 8 touches.
__device__ __forceinline__ void drop8(float* v, uint32_t key, uint32_t base, uint32_t thr, float scale) {
  const uint32_t odd = base & 1u, p0 = base >> 1;
  uint32_t h[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) h[k] = vlb_pair_hash(p0 + k, key);
  // the 16-bit fields of the run, in element order, are the 160-bit string h[0..4] read from bit 16 * odd: one funnel shift per
  // pair (v_alignbit_b32) instead of two selects per element
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t w = __builtin_amdgcn_alignbit(h[k + 1], h[k], odd << 4);
    v[2 * k] = ((w & 0xffffu) >= thr) ? v[2 * k] * scale : 0.f;
    v[2 * k + 1] = ((w >> 16) >= thr) ? v[2 * k + 1] * scale : 0.f;
  }
}

struct AttnParams {
  const bf16_t* qkv;   // [B*S, 3H]
  const float* mask;   // [B,S] 1 = attend, 0 = masked (adds -10000 like the reference)
  bf16_t* ctx;         // [B*S, H]          (fwd out / bwd in)
  float* lse;          // [B, nh, S]        (fwd out / bwd in)
  const bf16_t* dctx;  // [B*S, H]          (bwd in)
  bf16_t* dqkv;        // [B*S, 3H]         (bwd out)
  int B, S, H, nh;
  float scale;
  uint32_t drop_thr; float drop_scale; const uint32_t* seed; uint32_t tag;
};

// attention_long.hip: launch the streaming kernels for 256 < S <= 512 (no allocation, no synchronisation)
void vlb_attention_long_fwd_launch(const AttnParams& p, hipStream_t stream);
void vlb_attention_long_bwd_launch(const AttnParams& p, hipStream_t stream);
