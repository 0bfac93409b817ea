// The order in which the GEMM kernels visit their output tiles -- plain C++ (no HIP headers), so that a host program can include it
// and check it (tests/tile_order_check.cpp).
//
// A persistent workgroup b takes the work items w = b, b + grid, b + 2 grid, ...  Block b runs on XCD b % 8 and every grid width is a
// multiple of 8, so w & 7 is the XCD that executes work item w.  The order is two maps, one after the other:
//
// 1. vlb_xcd_order: every XCD owns a CONTIGUOUS run of the list (bijective for any item count), i.e. tiles that share operand panels
//    meet in ONE 4 MB L2.  With the plain w -> t = w order neighbouring tiles are spread over all 8 L2s: the profile of the grouped
//    weight-gradient kernel showed 3.1x the algorithmic bytes on the fabric (6.6 TB/s -- the kernel was memory-bound).
// 2. vlb_tile_of: the list is walked in groups of `tile_group` tile-rows, column-major inside a group, so that the ~64 workgroups
//    resident on one XCD share <= tile_group A panels and a few B panels instead of sweeping all of B for every A panel.  For the
//    weight gradients the group height comes from vlb_square_tile_group: the ~tiles/8 workgroups sharing an L2 then cover a
//    near-square patch of the output.  With a row-major run a wide output (dW of output.dense: 6 x 24 tiles) had every XCD stream
//    all of X -- 3.3x the algorithmic HBM bytes, at 4.8 TB/s.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VLB_TILE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define VLB_TILE_FN inline
#endif

// position of work item w (w & 7 = its XCD) when each of the 8 XCDs owns a contiguous run of the n items
VLB_TILE_FN int vlb_xcd_order(int w, int n) {
  const int xcd = w & 7, q = n >> 3, r = n & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (w >> 3);
}

// position t in [0, ntm * ntn) -> tile (tile_m, tile_n), in tile units: groups of tile_group (>= 1) tile-rows, column-major inside a
// group; the last group holds the remaining ntm % tile_group rows
VLB_TILE_FN void vlb_tile_of(int t, int ntm, int ntn, int tile_group, int& tile_m, int& tile_n) {
  const int gm = tile_group, per_group = gm * ntn, gid = t / per_group, first = gid * gm;
  const int gsz = ntm - first < gm ? ntm - first : gm, rem = t - gid * per_group;
  tile_m = first + rem % gsz;
  tile_n = rem / gsz;
}

// host rule for the weight gradients' group height: near-square per-XCD patches for wide outputs; tall outputs (decoder: 239 x 6
// tiles) already share their A panel row-wise.  In [1, ntm].
VLB_TILE_FN int vlb_square_tile_group(int ntm, int ntn) {
  int gm = 1;
  if (2 * ntn >= ntm) gm = (int)(sqrt((double)ntm * ntn / 8.0) + 0.5);
  if (gm > ntm) gm = ntm;
  return gm < 1 ? 1 : gm;
}
