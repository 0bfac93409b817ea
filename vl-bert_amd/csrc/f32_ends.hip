// fp32 front and back end of the VQA fine-tuning route (`fp32_ends`; host side engine.py / common/fast_rcnn.py / common/heads.py):
// what stands in front of X[0] and behind X[L] of the fp32 encoder (f32_path.hip) with every tensor in fp32.
//   * vlb_obj_prep_f32_fwd            - vlb_obj_prep_fwd with an fp32 [B*R, 4096] output (coordinate embedding || feature -> dropout)
//   * vlb_zero_padded_rows_f32        - rows of padded boxes -> 0
//   * vlb_embed_f32_fwd / _bwd        - the fused embedding of embed.hip for the module-API call form, tables read from the fp32 master
//   * vlb_dropout_f32                 - elementwise dropout, counter RNG and element index of vlb_dropout_bf16
//   * vlb_mul_f32                     - out = a * b (the kept GELU' multiplied into a gradient where no GEMM epilogue can do it)
//   * vlb_relu_bwd_f32                - out = g where y > 0 else 0 (ReLU backward of obj_downsample: no GEMM writes that gradient)
//   * vlb_bce_logits_f32_fwd_bwd      - vlb_bce_logits_fwd_bwd on fp32 logits
// None of them touches the 16-bit type: the two builds of the library hold the same code.  Lanes move 16 bytes, a row reduction is one
// wave per row (as ln_f32_*); dropout masks use the (seed, tag, element index) convention of their 16-bit twins.
#include "vlb_common.h"

#define E32_MAX_IT 8  // H <= 2048, 4 elements per lane per iteration

enum { K32_PAD = 0, K32_TEXT = 1, K32_OBJ = 2, K32_END = 3 };      // the row kinds of vlb_seq_layout (embed.hip)

__device__ __forceinline__ float4 drop4(float4 v, uint32_t seed, uint32_t tag, uint32_t e, uint32_t thr, float scale) {
  // elements e .. e + 3 (e even): two pair hashes, 16 bits per element
  const uint32_t h0 = vlb_rng_pair(seed, tag, e >> 1), h1 = vlb_rng_pair(seed, tag, (e >> 1) + 1);
  v.x = ((h0 & 0xffffu) >= thr) ? v.x * scale : 0.f;
  v.y = ((h0 >> 16) >= thr) ? v.y * scale : 0.f;
  v.z = ((h1 & 0xffffu) >= thr) ? v.z * scale : 0.f;
  v.w = ((h1 >> 16) >= thr) ? v.w * scale : 0.f;
  return v;
}

// ------------------------------------------------------------------------------------------
// obj_prep: one 256-thread block per region.  Feature half: 8 elements per thread.  Coordinate half: wave `which` owns coordinate
// `which`, lane l the frequencies 4l .. 4l+3 (sine slot j, cosine slot j + 256).  The angle reaches 100 rad, where fp32 rounding of
// the position and of the frequency alone is 1e-5 absolute, so position, frequency and sin / cos are evaluated in double (2048 angles per region:
// nothing against the 32 KB the block moves) and rounded once.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void obj_prep_f32_fwd_kernel(const float* __restrict__ boxes, long ldbox, const float* __restrict__ im_info,
                                                               long ldinfo, float* __restrict__ out, int B, int R, uint32_t drop_thr,
                                                               float drop_scale, const uint32_t* __restrict__ seedp, uint32_t tag) {
  const int row = blockIdx.x;  // b*R + r
  const int b = row / R;
  const float* bx = boxes + (long)row * ldbox;
  float* o = out + (long)row * 4096;
  const int tid = threadIdx.x;
  const uint32_t seed = (drop_thr && seedp) ? *seedp : 0u;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!(bx[0] > -1.5f)) {  // padded box: zero row
#pragma unroll
    for (int k = 0; k < 4; ++k) *(float4*)(o + k * 1024 + tid * 4) = zero;
    return;
  }
  {
    const int e0 = tid * 8;
    float4 f0 = *(const float4*)(bx + 4 + e0), f1 = *(const float4*)(bx + 4 + e0 + 4);
    if (drop_thr) {
      const uint32_t e = (uint32_t)row * 4096u + 2048u + (uint32_t)e0;
      f0 = drop4(f0, seed, tag, e, drop_thr, drop_scale);
      f1 = drop4(f1, seed, tag, e + 4u, drop_thr, drop_scale);
    }
    *(float4*)(o + 2048 + e0) = f0;
    *(float4*)(o + 2048 + e0 + 4) = f1;
  }
  const double W = im_info[b * ldinfo + 0], Hh = im_info[b * ldinfo + 1];
  const double x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
  const int which = tid >> 6, j0 = (tid & 63) * 4;
  const double pos = which == 0 ? (x1 + x2) / 2 / W * 100 : (which == 1 ? (y1 + y2) / 2 / Hh * 100 : (which == 2 ? (x2 - x1) / W * 100 : (y2 - y1) / Hh * 100));
  float sv[4], cv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = pos / pow(1000.0, (double)(j0 + k) / 256.0);
    sv[k] = (float)sin(a);
    cv[k] = (float)cos(a);
  }
  float4 s4 = make_float4(sv[0], sv[1], sv[2], sv[3]), c4 = make_float4(cv[0], cv[1], cv[2], cv[3]);
  if (drop_thr) {
    const uint32_t is = (uint32_t)row * 4096u + (uint32_t)(which * 512 + j0);
    s4 = drop4(s4, seed, tag, is, drop_thr, drop_scale);
    c4 = drop4(c4, seed, tag, is + 256u, drop_thr, drop_scale);
  }
  *(float4*)(o + which * 512 + j0) = s4;
  *(float4*)(o + which * 512 + 256 + j0) = c4;
}

// x[r, :] = 0 for the rows of padded boxes (boxes[r*ldbox] <= -1.5); one wave per row
__global__ __launch_bounds__(256) void zero_padded_rows_f32_kernel(float* __restrict__ x, long ld, const float* __restrict__ boxes, long ldbox,
                                                                   int rows, int H) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows || boxes[(long)row * ldbox] > -1.5f) return;
  for (int c = lane * 4; c < H; c += 256) *(float4*)(x + (long)row * ld + c) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------
// embedding forward: one wave per output row (b, s); lane owns columns (lane + 64 i) * 4 .. + 3
// ------------------------------------------------------------------------------------------
struct Embed32Params {
  const int32_t* code; const int32_t* text_len; const int64_t* text_ids; const int64_t* text_type;
  const float* word_emb; const float* pos_emb; const float* type_emb; const float* end_emb;
  const float* text_vis; long tv_sb, tv_st;
  const float* obj_vis; long ov_sb, ov_sr;
  const float* obj_ling; long ol_sb, ol_sr;
  const float* gamma; const float* beta;
  float* pre; float* stats; float* out;
  int B, T, R, S, H, V, P;
  float eps;
  uint32_t drop_thr; float drop_scale; const uint32_t* seed; uint32_t tag;
};

__device__ __forceinline__ int clamp_type32(int64_t t) { return t < 0 ? 0 : (t > 2 ? 2 : (int)t); }

__device__ __forceinline__ void add_row_f32(const float* src, int H, int lane, float4* acc) {
#pragma unroll
  for (int i = 0; i < E32_MAX_IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      const float4 w = *(const float4*)(src + c);
      acc[i].x += w.x; acc[i].y += w.y; acc[i].z += w.z; acc[i].w += w.w;
    }
  }
}

__global__ __launch_bounds__(256) void embed_f32_fwd_kernel(const Embed32Params p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.B * p.S) return;
  const int b = row / p.S, s = row % p.S;
  const int code = p.code[row], kind = code >> 16, idx = code & 0xffff;
  const int tl = p.text_len[b];
  const int H = p.H;
  float4 acc[E32_MAX_IT];
#pragma unroll
  for (int i = 0; i < E32_MAX_IT; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  int type_id = 0, pos_id = s;  // pad rows: zeros + position s + type 0
  if (kind == K32_TEXT) {
    long id = p.text_ids[b * p.T + idx];
    id = id < 0 ? 0 : (id >= p.V ? p.V - 1 : id);
    add_row_f32(p.word_emb + id * H, H, lane, acc);
    add_row_f32(p.text_vis + b * p.tv_sb + idx * p.tv_st, H, lane, acc);
    type_id = p.text_type ? clamp_type32(p.text_type[b * p.T + idx]) : 0;
  } else if (kind == K32_OBJ) {
    add_row_f32(p.obj_vis + b * p.ov_sb + idx * p.ov_sr, H, lane, acc);
    add_row_f32(p.obj_ling + b * p.ol_sb + idx * p.ol_sr, H, lane, acc);
    type_id = 2;
    pos_id = tl;
  } else if (kind == K32_END) {
    add_row_f32(p.end_emb, H, lane, acc);
    type_id = 2;
    pos_id = tl + 1;
  }
  pos_id = min(pos_id, p.P - 1);
  add_row_f32(p.pos_emb + (long)pos_id * H, H, lane, acc);
  add_row_f32(p.type_emb + (long)type_id * H, H, lane, acc);

  float* pre = p.pre + (long)row * H;
  float s1 = 0.f;
#pragma unroll
  for (int i = 0; i < E32_MAX_IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      *(float4*)(pre + c) = acc[i];
      s1 += (acc[i].x + acc[i].y) + (acc[i].z + acc[i].w);
    }
  }
  const float mean = wave_sum(s1) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < E32_MAX_IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      const float a = acc[i].x - mean, bb = acc[i].y - mean, cc = acc[i].z - mean, d = acc[i].w - mean;
      q += a * a + bb * bb + cc * cc + d * d;
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + p.eps);
  if (lane == 0) {
    p.stats[2 * (long)row] = mean;
    p.stats[2 * (long)row + 1] = rstd;
  }
  const uint32_t seed = (p.drop_thr && p.seed) ? *p.seed : 0u;
  float* o = p.out + (long)row * H;
#pragma unroll
  for (int i = 0; i < E32_MAX_IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      const float4 g = *(const float4*)(p.gamma + c), be = *(const float4*)(p.beta + c);
      float4 y = make_float4((acc[i].x - mean) * rstd * g.x + be.x, (acc[i].y - mean) * rstd * g.y + be.y,
                             (acc[i].z - mean) * rstd * g.z + be.z, (acc[i].w - mean) * rstd * g.w + be.w);
      if (p.drop_thr) y = drop4(y, seed, p.tag, (uint32_t)row * (uint32_t)H + (uint32_t)c, p.drop_thr, p.drop_scale);
      *(float4*)(o + c) = y;
    }
  }
}

// ------------------------------------------------------------------------------------------
// embedding backward: gridDim.y workgroups of four waves per sample, each over a contiguous chunk of its S rows, one row per wave at a
// time.  Per row: dropout mask on dy, LayerNorm backward -> d (registers), then
//   word_emb[id] / position row of a text or end token / end_emb / type row 2 of a text or end token : global fp32 atomics,
//                                                            issued lane-consecutive through a per-wave row image in LDS
//   type rows 0 / 1 of the text tokens, type row 2 + the shared position row `text_len` of the objects,
//   dgamma / dbeta                                          : register sums per wave -> LDS -> one atomic per column and workgroup
//   d(text_vis) per token, d(obj_vis), d(obj_ling)          : plain stores
// Pad rows reach no loss (their dy is zero) and are skipped.
// ------------------------------------------------------------------------------------------
struct Embed32BwdParams {
  const float* dy; const float* pre; const float* stats; const float* gamma;
  const int32_t* code; const int32_t* text_len; const int64_t* text_ids; const int64_t* text_type;
  float* d_word; float* d_pos; float* d_type; float* d_end; float* d_gamma; float* d_beta;
  float* d_text_vis; long dtv_sb, dtv_st;
  float* d_obj_vis; long dov_sb, dov_sr;
  float* d_obj_ling; long dol_sb, dol_sr;
  int B, T, R, S, H, V, P;
  uint32_t drop_thr; float drop_scale; const uint32_t* seed; uint32_t tag;
};

template <int NIT>
__global__ __launch_bounds__(256) void embed_f32_bwd_kernel(const Embed32BwdParams p) {
  constexpr int LWD = NIT * 256;
  __shared__ __attribute__((aligned(16))) float red[4][LWD];
  const int H = p.H;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tl = p.text_len[b];
  const uint32_t seed = (p.drop_thr && p.seed) ? *p.seed : 0u;
  // acc[0] dgamma, [1] dbeta, [2] text rows of type 0, [3] of type 1, [4] object rows
  float4 acc[5][NIT], gam[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
#pragma unroll
    for (int a = 0; a < 5; ++a) acc[a][i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int c = (lane + 64 * i) * 4;
    gam[i] = c < H ? *(const float4*)(p.gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int rows_per = (p.S + gridDim.y - 1) / gridDim.y, s_lo = blockIdx.y * rows_per, s_hi = min(p.S, s_lo + rows_per);
  for (int s = s_lo + wave; s < s_hi; s += 4) {
    const long row = (long)b * p.S + s;
    const int code = p.code[row], kind = code >> 16, idx = code & 0xffff;
    if (kind == K32_PAD) continue;
    const float mean = p.stats[2 * row], rstd = p.stats[2 * row + 1];
    float4 g[NIT], xh[NIT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = (lane + 64 * i) * 4;
      g[i] = xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < H) {
        const float4 xv = *(const float4*)(p.pre + row * H + c);
        float4 d = *(const float4*)(p.dy + row * H + c);
        if (p.drop_thr) d = drop4(d, seed, p.tag, (uint32_t)row * (uint32_t)H + (uint32_t)c, p.drop_thr, p.drop_scale);
        xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
        g[i] = make_float4(d.x * gam[i].x, d.y * gam[i].y, d.z * gam[i].z, d.w * gam[i].w);
        s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        s2 += g[i].x * xh[i].x + g[i].y * xh[i].y + g[i].z * xh[i].z + g[i].w * xh[i].w;
        acc[0][i].x += d.x * xh[i].x; acc[0][i].y += d.y * xh[i].y; acc[0][i].z += d.z * xh[i].z; acc[0][i].w += d.w * xh[i].w;
        acc[1][i].x += d.x; acc[1][i].y += d.y; acc[1][i].z += d.z; acc[1][i].w += d.w;
      }
    }
    const float m1 = wave_sum(s1) / (float)H, m2 = wave_sum(s2) / (float)H;
    // destinations (wave-uniform: one row per wave)
    int type_id = 2, pos_id = s;
    float* w_dst = nullptr;      // atomics: the word / end embedding row
    float* v_dst = nullptr;      // plain stores: the visual part
    float* l_dst = nullptr;      // plain stores: the objects' linguistic part
    if (kind == K32_TEXT) {
      long id = p.text_ids[b * p.T + idx];
      id = id < 0 ? 0 : (id >= p.V ? p.V - 1 : id);
      w_dst = p.d_word + id * H;
      type_id = p.text_type ? clamp_type32(p.text_type[b * p.T + idx]) : 0;
      if (p.d_text_vis) v_dst = p.d_text_vis + b * p.dtv_sb + idx * p.dtv_st;
    } else if (kind == K32_OBJ) {
      if (p.d_obj_vis) v_dst = p.d_obj_vis + b * p.dov_sb + idx * p.dov_sr;
      if (p.d_obj_ling) l_dst = p.d_obj_ling + b * p.dol_sb + idx * p.dol_sr;
    } else {
      pos_id = tl + 1;
      w_dst = p.d_end;
    }
    pos_id = min(pos_id, p.P - 1);
    const int ukind = __builtin_amdgcn_readfirstlane(kind), utype = __builtin_amdgcn_readfirstlane(type_id);
    float* pos_dst = p.d_pos + (long)pos_id * H;
    float* type2_dst = p.d_type + 2 * (long)H;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < H) {
        const float4 d = make_float4(rstd * (g[i].x - m1 - xh[i].x * m2), rstd * (g[i].y - m1 - xh[i].y * m2),
                                     rstd * (g[i].z - m1 - xh[i].z * m2), rstd * (g[i].w - m1 - xh[i].w * m2));
        if (v_dst) *(float4*)(v_dst + c) = d;
        if (l_dst) *(float4*)(l_dst + c) = d;
        if (ukind == K32_OBJ) {
          acc[4][i].x += d.x; acc[4][i].y += d.y; acc[4][i].z += d.z; acc[4][i].w += d.w;
        } else {
          *(float4*)&red[wave][c] = d;      // the wave's row image: the global atomics below go out lane-consecutive
          if (utype == 0) {
            acc[2][i].x += d.x; acc[2][i].y += d.y; acc[2][i].z += d.z; acc[2][i].w += d.w;
          } else if (utype == 1) {
            acc[3][i].x += d.x; acc[3][i].y += d.y; acc[3][i].z += d.z; acc[3][i].w += d.w;
          }
        }
      }
    }
    if (ukind != K32_OBJ) {
      // 64 lanes = 256 contiguous bytes per atomic instruction (in the 4-floats-per-lane register layout one instruction touches every
      // 4th float of 1 KB: four times the requests, the rate embed_bwd_kernel of embed.hip was bound by)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the row image is wave-private: order the writes above before the reads
      __builtin_amdgcn_wave_barrier();
      for (int c = lane; c < H; c += 64) {
        const float v = red[wave][c];
        atomicAdd(w_dst + c, v);
        atomicAdd(pos_dst + c, v);
        if (utype == 2) atomicAdd(type2_dst + c, v);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  // the four waves' register sums, one accumulator at a time: LDS -> one atomic per column and workgroup
  const int pos_obj = min(tl, p.P - 1);
#pragma unroll
  for (int a = 0; a < 5; ++a) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = (lane + 64 * i) * 4;
      if (c < H) *(float4*)&red[wave][c] = acc[a][i];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 256) {
      const float v = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
      if (a == 0) atomicAdd(p.d_gamma + c, v);
      else if (a == 1) atomicAdd(p.d_beta + c, v);
      else if (v != 0.f) {      // (a table row that no token of this chunk selects is not touched)
        if (a == 2) atomicAdd(p.d_type + c, v);
        else if (a == 3) atomicAdd(p.d_type + H + c, v);
        else {
          atomicAdd(p.d_type + 2 * (long)H + c, v);
          atomicAdd(p.d_pos + (long)pos_obj * H + c, v);
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// y = x * keep(i) / (1 - p), i = position in the [n] array: four elements per lane, the last n % 4 by the first lanes
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_f32_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int vec, uint32_t drop_thr,
                                                          float drop_scale, const uint32_t* __restrict__ seedp, uint32_t tag) {
  const uint32_t seed = (drop_thr && seedp) ? *seedp : 0u;
  const long n4 = vec ? n / 4 : 0, t0 = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  for (long i = t0; i < n4; i += stride) {
    float4 v = *(const float4*)(x + 4 * i);
    if (drop_thr) v = drop4(v, seed, tag, (uint32_t)(4 * i), drop_thr, drop_scale);
    *(float4*)(y + 4 * i) = v;
  }
  for (long i = 4 * n4 + t0; i < n; i += stride) {
    const float v = x[i];
    y[i] = (!drop_thr || vlb_keep(seed, tag, (uint32_t)i, drop_thr)) ? (drop_thr ? v * drop_scale : v) : 0.f;
  }
}

// out = a * b, n % 4 == 0
__global__ __launch_bounds__(256) void mul_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 x = *(const float4*)(a + 4 * i), y = *(const float4*)(b + 4 * i);
    *(float4*)(out + 4 * i) = make_float4(x.x * y.x, x.y * y.y, x.z * y.z, x.w * y.w);
  }
}

// out = y > 0 ? g : 0, n % 4 == 0
__global__ __launch_bounds__(256) void relu_bwd_f32_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = *(const float4*)(g + 4 * i), b = *(const float4*)(y + 4 * i);
    *(float4*)(out + 4 * i) = make_float4(b.x > 0.f ? a.x : 0.f, b.y > 0.f ? a.y : 0.f, b.z > 0.f ? a.z : 0.f, b.w > 0.f ? a.w : 0.f);
  }
}

// ------------------------------------------------------------------------------------------
// VQA answer loss on fp32 logits: F.binary_cross_entropy_with_logits(logits[rows, A], label) * A, i.e. (1 / rows) sum ( max(x, 0) - x y +
// log(1 + exp(-|x|)) ); the logits (row stride ld % 4 == 0) are overwritten by gscale * w * (sigmoid(x) - y) / rows, columns >= A by 0.
// One block per row, four columns per lane.  The loss is summed in a fixed order, so that it is the same bits on every run and on both
// builds of the library: each block writes its row's sum to row_loss[row], and bce_loss_sum_f32_kernel (one wave) adds the rows up.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bce_logits_f32_kernel(float* __restrict__ logits, long ld, int A, const float* __restrict__ label, long ldl,
                                                             int rows, float gscale, float pos_weight, float* __restrict__ row_loss,
                                                             float* __restrict__ logits_copy, long ldcopy) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  float* x = logits + (long)row * ld;
  const float* y = label + (long)row * ldl;
  const float inv_rows = 1.0f / (float)rows;
  float acc = 0.f;
  for (int a0 = threadIdx.x * 4; a0 < (int)ld; a0 += 1024) {
    const float4 v4 = *(const float4*)(x + a0);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    float o[4], cp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int a = a0 + k;
      o[k] = cp[k] = 0.f;
      if (a < A) {
        const float t = y[a];
        const float e = expf(-fabsf(v[k]));
        const float w = t > 0.5f ? pos_weight : 1.0f;
        acc += w * (fmaxf(v[k], 0.f) - v[k] * t + log1pf(e));
        const float sig = v[k] >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
        o[k] = w * (sig - t) * inv_rows * gscale;
        cp[k] = v[k];
      }
    }
    *(float4*)(x + a0) = make_float4(o[0], o[1], o[2], o[3]);
    if (logits_copy && a0 < (int)ldcopy) *(float4*)(logits_copy + (long)row * ldcopy + a0) = make_float4(cp[0], cp[1], cp[2], cp[3]);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) row_loss[row] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// loss_out += (1 / rows) sum_r row_loss[r]: lane l takes rows l, l + 64, ... in order, then the butterfly of wave_sum
__global__ __launch_bounds__(64) void bce_loss_sum_f32_kernel(const float* __restrict__ row_loss, int rows, float* __restrict__ loss_out) {
  float acc = 0.f;
  for (int r = threadIdx.x; r < rows; r += 64) acc += row_loss[r];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) atomicAdd(loss_out, acc * (1.0f / (float)rows));
}

// ------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------
static inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

extern "C" int vlb_obj_prep_f32_fwd(const float* boxes, long ldbox, const float* im_info, long ldinfo, float* out, int B, int R, float drop_p,
                                    const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  if (B * R <= 0) return VLB_OK;
  VLB_CHECK_ARG(ldbox >= 4 + 2048 && (ldbox % 4) == 0, "vlb_obj_prep_f32_fwd: ldbox=%ld must be >= 2052 and a multiple of 4", ldbox);
  VLB_CHECK_ARG(boxes && im_info && out && ldinfo >= 2 && al16(boxes) && al16(out),
                "vlb_obj_prep_f32_fwd: null / unaligned argument or im_info rows narrower than (width, height): ldinfo=%ld", ldinfo);
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_obj_prep_f32_fwd: dropout needs a device seed pointer");
  VLB_CHECK_ARG((long)B * R * 4096 < (1L << 32), "vlb_obj_prep_f32_fwd: dropout index overflow");
  const uint32_t thr = vlb_drop_thr(drop_p);
  hipLaunchKernelGGL(obj_prep_f32_fwd_kernel, dim3(B * R), dim3(256), 0, stream, boxes, ldbox, im_info, ldinfo, out, B, R, thr,
                     vlb_drop_scale(thr), seed, tag);
  VLB_CHECK_LAUNCH("vlb_obj_prep_f32_fwd");
  return VLB_OK;
}

extern "C" int vlb_zero_padded_rows_f32(float* x, long ld, const float* boxes, long ldbox, int rows, int H, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(x && boxes && H > 0 && (H % 4) == 0 && (ld % 4) == 0 && ld >= H && al16(x), "vlb_zero_padded_rows_f32: bad argument");
  hipLaunchKernelGGL(zero_padded_rows_f32_kernel, dim3(vlb_cdiv(rows, 4)), dim3(256), 0, stream, x, ld, boxes, ldbox, rows, H);
  VLB_CHECK_LAUNCH("vlb_zero_padded_rows_f32");
  return VLB_OK;
}

extern "C" int vlb_embed_f32_fwd(const int32_t* code, const int32_t* text_len, const int64_t* text_ids, const int64_t* text_type,
                                 const float* word_emb, const float* pos_emb, const float* type_emb, const float* end_emb,
                                 const float* text_vis, long tv_sb, long tv_st, const float* obj_vis, long ov_sb, long ov_sr,
                                 const float* obj_ling, long ol_sb, long ol_sr, const int64_t* obj_ling_idx, const float* gamma,
                                 const float* beta, float* pre, float* stats, float* out, int B, int T, int R, int S, int H, int V, int P,
                                 float eps, float drop_p, const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  if ((long)B * S <= 0) return VLB_OK;
  VLB_CHECK_ARG(H > 0 && (H % 4) == 0 && H <= 256 * E32_MAX_IT, "vlb_embed_f32_fwd: unsupported H=%d", H);
  VLB_CHECK_ARG(!obj_ling_idx, "vlb_embed_f32_fwd: the table-indexed obj_ling_idx form is not built in fp32 (dense obj_ling only)");
  VLB_CHECK_ARG(code && text_len && text_ids && word_emb && pos_emb && type_emb && end_emb && text_vis && obj_vis && obj_ling && gamma &&
                    beta && pre && stats && out, "vlb_embed_f32_fwd: null argument");
  VLB_CHECK_ARG(V > 0 && P > 0 && T < 65536 && R < 65536, "vlb_embed_f32_fwd: bad table / sequence sizes");
  VLB_CHECK_ARG((tv_sb % 4) == 0 && (tv_st % 4) == 0 && (ov_sb % 4) == 0 && (ov_sr % 4) == 0 && (ol_sb % 4) == 0 && (ol_sr % 4) == 0,
                "vlb_embed_f32_fwd: strides must be multiples of 4 floats");
  VLB_CHECK_ARG(al16(word_emb) && al16(pos_emb) && al16(type_emb) && al16(end_emb) && al16(text_vis) && al16(obj_vis) && al16(obj_ling) &&
                    al16(gamma) && al16(beta) && al16(pre) && al16(out), "vlb_embed_f32_fwd: pointers must be 16-byte aligned");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_embed_f32_fwd: dropout needs a device seed pointer");
  VLB_CHECK_ARG((long)B * S * H < (1L << 32), "vlb_embed_f32_fwd: dropout index overflow");
  Embed32Params p;
  p.code = code; p.text_len = text_len; p.text_ids = text_ids; p.text_type = text_type;
  p.word_emb = word_emb; p.pos_emb = pos_emb; p.type_emb = type_emb; p.end_emb = end_emb;
  p.text_vis = text_vis; p.tv_sb = tv_sb; p.tv_st = tv_st;
  p.obj_vis = obj_vis; p.ov_sb = ov_sb; p.ov_sr = ov_sr;
  p.obj_ling = obj_ling; p.ol_sb = ol_sb; p.ol_sr = ol_sr;
  p.gamma = gamma; p.beta = beta; p.pre = pre; p.stats = stats; p.out = out;
  p.B = B; p.T = T; p.R = R; p.S = S; p.H = H; p.V = V; p.P = P; p.eps = eps;
  p.drop_thr = vlb_drop_thr(drop_p); p.drop_scale = vlb_drop_scale(p.drop_thr); p.seed = seed; p.tag = tag;
  hipLaunchKernelGGL(embed_f32_fwd_kernel, dim3(vlb_cdiv((long)B * S, 4)), dim3(256), 0, stream, p);
  VLB_CHECK_LAUNCH("vlb_embed_f32_fwd");
  return VLB_OK;
}

extern "C" int vlb_embed_f32_bwd(const float* dy, const float* pre, const float* stats, const float* gamma, const int32_t* code,
                                 const int32_t* text_len, const int64_t* text_ids, const int64_t* text_type, const int64_t* obj_ling_idx,
                                 float* d_word, float* d_pos, float* d_type, float* d_end, float* d_gamma, float* d_beta, float* d_text_vis,
                                 long dtv_sb, long dtv_st, float* d_obj_vis, long dov_sb, long dov_sr, float* d_obj_ling, long dol_sb,
                                 long dol_sr, int B, int T, int R, int S, int H, int V, int P, float drop_p, const uint32_t* seed,
                                 uint32_t tag, hipStream_t stream) {
  if (B <= 0 || S <= 0) return VLB_OK;
  VLB_CHECK_ARG(H > 0 && (H % 4) == 0 && H <= 256 * E32_MAX_IT, "vlb_embed_f32_bwd: unsupported H=%d", H);
  VLB_CHECK_ARG(!obj_ling_idx, "vlb_embed_f32_bwd: the table-indexed obj_ling_idx form is not built in fp32 (dense obj_ling only)");
  VLB_CHECK_ARG(dy && pre && stats && gamma && code && text_len && text_ids && d_word && d_pos && d_type && d_end && d_gamma && d_beta,
                "vlb_embed_f32_bwd: null argument");
  VLB_CHECK_ARG(V > 0 && P > 0, "vlb_embed_f32_bwd: bad table sizes");
  VLB_CHECK_ARG(!d_text_vis || dtv_st != 0, "vlb_embed_f32_bwd: per-token text_vis gradients only (dtv_st != 0)");
  VLB_CHECK_ARG((dtv_sb % 4) == 0 && (dtv_st % 4) == 0 && (dov_sb % 4) == 0 && (dov_sr % 4) == 0 && (dol_sb % 4) == 0 && (dol_sr % 4) == 0,
                "vlb_embed_f32_bwd: output strides must be multiples of 4 floats");
  VLB_CHECK_ARG(al16(dy) && al16(pre) && al16(gamma) && al16(d_text_vis) && al16(d_obj_vis) && al16(d_obj_ling),
                "vlb_embed_f32_bwd: pointers must be 16-byte aligned");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_embed_f32_bwd: dropout needs a device seed pointer");
  VLB_CHECK_ARG((long)B * S * H < (1L << 32), "vlb_embed_f32_bwd: dropout index overflow");
  Embed32BwdParams p;
  p.dy = dy; p.pre = pre; p.stats = stats; p.gamma = gamma; p.code = code; p.text_len = text_len; p.text_ids = text_ids;
  p.text_type = text_type;
  p.d_word = d_word; p.d_pos = d_pos; p.d_type = d_type; p.d_end = d_end; p.d_gamma = d_gamma; p.d_beta = d_beta;
  p.d_text_vis = d_text_vis; p.dtv_sb = dtv_sb; p.dtv_st = dtv_st;
  p.d_obj_vis = d_obj_vis; p.dov_sb = dov_sb; p.dov_sr = dov_sr;
  p.d_obj_ling = d_obj_ling; p.dol_sb = dol_sb; p.dol_sr = dol_sr;
  p.B = B; p.T = T; p.R = R; p.S = S; p.H = H; p.V = V; p.P = P;
  p.drop_thr = vlb_drop_thr(drop_p); p.drop_scale = vlb_drop_scale(p.drop_thr); p.seed = seed; p.tag = tag;
  int split = vlb_cdiv(512, B);      // small batches: several workgroups per sample
  if (split > 8) split = 8;
  if (split > S) split = S;
  if (split < 1) split = 1;
  const int nit = vlb_cdiv(H, 256);
#define E32_BWD(NIT) hipLaunchKernelGGL(embed_f32_bwd_kernel<NIT>, dim3(B, split), dim3(256), 0, stream, p)
  if (nit <= 1) E32_BWD(1); else if (nit == 2) E32_BWD(2); else if (nit == 3) E32_BWD(3); else if (nit == 4) E32_BWD(4); else E32_BWD(8);
#undef E32_BWD
  VLB_CHECK_LAUNCH("vlb_embed_f32_bwd");
  return VLB_OK;
}

extern "C" int vlb_dropout_f32(const float* x, float* y, long n, float drop_p, const uint32_t* seed, uint32_t tag, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(x && y && n < (1L << 32), "vlb_dropout_f32: bad argument");
  VLB_CHECK_ARG(!(drop_p > 0.f) || seed, "vlb_dropout_f32: dropout needs a device seed pointer");
  const uint32_t thr = vlb_drop_thr(drop_p);
  const int vec = (al16(x) && al16(y)) ? 1 : 0;
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(dropout_f32_kernel, dim3((int)blocks), dim3(256), 0, stream, x, y, n, vec, thr, vlb_drop_scale(thr), seed, tag);
  VLB_CHECK_LAUNCH("vlb_dropout_f32");
  return VLB_OK;
}

extern "C" int vlb_mul_f32(const float* a, const float* b, float* out, long n, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(a && b && out && (n % 4) == 0 && al16(a) && al16(b) && al16(out), "vlb_mul_f32: n %% 4 == 0 and 16-byte aligned pointers");
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mul_f32_kernel, dim3((int)blocks), dim3(256), 0, stream, a, b, out, n / 4);
  VLB_CHECK_LAUNCH("vlb_mul_f32");
  return VLB_OK;
}

extern "C" int vlb_relu_bwd_f32(const float* g, const float* y, float* out, long n, hipStream_t stream) {
  if (n <= 0) return VLB_OK;
  VLB_CHECK_ARG(g && y && out && (n % 4) == 0 && al16(g) && al16(y) && al16(out), "vlb_relu_bwd_f32: n %% 4 == 0 and 16-byte aligned pointers");
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(relu_bwd_f32_kernel, dim3((int)blocks), dim3(256), 0, stream, g, y, out, n / 4);
  VLB_CHECK_LAUNCH("vlb_relu_bwd_f32");
  return VLB_OK;
}

extern "C" int vlb_bce_logits_f32_fwd_bwd(float* logits, long ld, int rows, int A, const float* label, long ldl, float gscale, float pos_weight,
                                          float* loss_out, float* row_loss, float* logits_copy, long ldcopy, hipStream_t stream) {
  if (rows <= 0) return VLB_OK;
  VLB_CHECK_ARG(logits && label && loss_out && row_loss && A > 0 && ld >= A && ldl >= A, "vlb_bce_logits_f32_fwd_bwd: bad argument");
  VLB_CHECK_ARG((ld % 4) == 0 && al16(logits), "vlb_bce_logits_f32_fwd_bwd: logits rows must be 16-byte aligned (ld %% 4 == 0)");
  VLB_CHECK_ARG(!logits_copy || (ldcopy >= ld && (ldcopy % 4) == 0 && al16(logits_copy)),
                "vlb_bce_logits_f32_fwd_bwd: logits_copy needs ldcopy >= ld, ldcopy %% 4 == 0");
  hipLaunchKernelGGL(bce_logits_f32_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, A, label, ldl, rows, gscale, pos_weight, row_loss,
                     logits_copy, ldcopy);
  VLB_CHECK_LAUNCH("vlb_bce_logits_f32_fwd_bwd");
  hipLaunchKernelGGL(bce_loss_sum_f32_kernel, dim3(1), dim3(64), 0, stream, row_loss, rows, loss_out);
  VLB_CHECK_LAUNCH("vlb_bce_logits_f32_fwd_bwd");
  return VLB_OK;
}
