// Block-wide (256 threads) argmax reductions shared by the validation kernels (metrics.hip) and the ACC forms of the fused loss kernels
// (loss.hip, f32_pretrain.hip).  One tie rule everywhere, torch.argmax's: equal values go to the LOWEST column.  A thread that holds no
// column carries (-inf, INT_MAX) and never wins.
#pragma once
#include <limits.h>

#include "vlb_common.h"

// (m, s, i) <- merge with (m2, s2, i2): online softmax pair + argmax; equal maxima keep the lower column
__device__ __forceinline__ void arg_merge(float& m, float& s, int& i, float m2, float s2, int i2) {
  if (m2 > m || (m2 == m && i2 < i)) i = i2;
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;  // both empty
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// block-wide (256 threads) reduction of the triple; result broadcast.  sh: 12 floats
__device__ __forceinline__ void block_arg_reduce(float& m, float& s, int& i, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    arg_merge(m, s, i, m2, s2, i2);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
    sh[wave * 3] = m;
    sh[wave * 3 + 1] = s;
    sh[wave * 3 + 2] = __int_as_float(i);
  }
  __syncthreads();
  m = sh[0];
  s = sh[1];
  i = __float_as_int(sh[2]);
#pragma unroll
  for (int w = 1; w < 4; ++w) arg_merge(m, s, i, sh[w * 3], sh[w * 3 + 1], __float_as_int(sh[w * 3 + 2]));
}

// block-wide argmax (value, lowest column among equals); result broadcast.  sh: 8 floats
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
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
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
}

typedef unsigned long long vlb_u64;      // the counters' type on the device ([hits, counted rows] of an int64[2])
