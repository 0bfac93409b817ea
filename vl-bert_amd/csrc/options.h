// The library's integer tuning knobs: ONE table (options.hip) with a row per knob.  A knob takes its value from its environment
// variable (read at most once per process, on first use) or its default; vlb_gemm_set_option(name, value) overrides it at run time,
// before or after that read, for A/B measurements and tests inside one process.  Clamps stay at the use sites.
//
// X(id, option name, environment variable or nullptr, default)
#pragma once

#define VLB_OPTIONS(X)                                                                                                                  \
  /* ---- gemm_p8.hip: large-tile 8-phase NT core ---- */                                                                               \
  /* 0 off | 1 cost model | 3 / 4 / 5: force the 192- / 256- / 320-row tile wherever the kernel applies */                              \
  X(P8_MODE, "p8_mode", "VLB_GEMM_P8", 1)                                                                                               \
  /* 256-row tile: 1 keeps the B0 fragments in registers for the 4th quadrant (16 more VGPRs), 0 re-reads them */                       \
  X(P8_KEEPB, "p8_keepb", "VLB_GEMM_P8_KEEPB", 1)                                                                                       \
  /* tile-rows per L2 group (tile_order.h) */                                                                                           \
  X(P8_GROUP, "p8_group", "VLB_GEMM_P8_GROUP", 2)                                                                                       \
  /* a tile height qualifies with at least this many tiles (below that the 128x128 kernel fills the chip better) */                     \
  X(P8_MIN_TILES, "p8_min_tiles", "VLB_GEMM_P8_MIN_TILES", 160)                                                                         \
  /* persistent workgroups per launch (8..256, else 256 = one per CU).  Fewer leave CUs to a kernel running on another stream (the      \
     weight-gradient GEMMs of the side stream): an MFMA-bound kernel then fills the HBM-bound epilogue bursts of this one */            \
  X(P8_WGS, "p8_wgs", "VLB_GEMM_P8_WGS", 256)                                                                                           \
  /* tools/p8_check.py ablate; results are WRONG when != 0: 1 no epilogue | 2 epilogue without its global stores | 4 (results           \
     correct) per-workgroup clock stamps into the table passed as `pre` (tools/clock_probe.py) */                                       \
  X(P8_ABLATE, "p8_ablate", nullptr, 0)                                                                                                 \
  /* 1: the cost model may pick the 192-row tile */                                                                                     \
  X(P8_TILE192, "p8_tile192", "VLB_GEMM_P8_192", 1)                                                                                     \
  /* 1: vmcnt(0) behind every output tile (round-3 behaviour, for a cold-cache A/B) */                                                  \
  X(P8_DRAIN, "p8_drain", "VLB_GEMM_P8_DRAIN", 0)                                                                                       \
  /* 1: wave-private drain for a workgroup's LAST tile with every epilogue (default: bias-only / plain epilogue only -- with side        \
     tensors the 128-row slab over the idle ring is faster: QKV data gradient 84.7 vs 90.4 us) */                                       \
  X(P8_LASTW, "p8_lastw", "VLB_GEMM_P8_LASTW", 0)                                                                                       \
  /* ---- gemm.hip: NT kernels ---- */                                                                                                  \
  /* ring kernels: 0 off | 1 auto | 2 force 128x128 | 3 force 128x64 */                                                                 \
  X(NT_RING, "nt_ring", "VLB_GEMM_NT_RING", 1)                                                                                          \
  /* 128x128 kernel: second-resident workgroups start `stagger` x ~3.4 us late */                                                       \
  X(NT_STAGGER, "nt_stagger", "VLB_GEMM_NT_STAGGER", 0)                                                                                 \
  /* tile-rows per L2 group of the 128-row NT kernels and the implicit convolution */                                                   \
  X(TILE_GROUP, "tile_group", "VLB_GEMM_TILE_GROUP", 4)                                                                                 \
  /* persistent grid of the two-stage kernel: workgroups resident at once (2 per CU with 48-64 KB LDS each on 256 CUs) */               \
  X(RESIDENT, "resident", "VLB_GEMM_RESIDENT", 512)                                                                                     \
  /* 1: single-epilogue instantiations (0: always the generic kernel with the run-time dispatch; 15.4 -> 14.6 ms / step) */             \
  X(EPI_SPECIALISE, "epi_specialise", "VLB_GEMM_EPI_SPECIALISE", 1)                                                                     \
  /* 256x256 tiles for plain bf16 GEMMs: 0 off | 1 B does not fit the L2s and >= 512 tiles | n >= 2: every plain GEMM with >= n tiles */ \
  X(NT_256, "nt_256", "VLB_GEMM_256", 1)                                                                                                \
  /* tile-rows per L2 group of the 256x256 kernel */                                                                                    \
  X(NT_256_GROUP, "nt_256_group", "VLB_GEMM_256_GROUP", 2)                                                                              \
  /* ---- gemm.hip: 128x128 TN (weight-gradient) kernel ---- */                                                                         \
  /* tile-rows per L2 group; <= 0: the near-square rule of tile_order.h */                                                              \
  X(TN_GROUP, "tn_group", "VLB_GEMM_TN_GROUP", -1)                                                                                      \
  /* ---- gemm_tn8.hip: large-tile weight-gradient core ---- */                                                                         \
  /* 0: the 128x128 TN kernel only */                                                                                                   \
  X(TN8_MODE, "tn8_mode", "VLB_GEMM_TN8", 1)                                                                                            \
  /* persistent workgroups per launch (8..256, else 256 = one per CU) */                                                                \
  X(TN8_WGS, "tn8_wgs", "VLB_GEMM_TN8_WGS", 256)                                                                                        \
  /* measurement builds (-DVLB_TN8_PROBE) only: see the kernel's ABL parameter */                                                       \
  X(TN8_ABLATE, "tn8_ablate", nullptr, 0)                                                                                               \
  /* tile-rows per L2 group; <= 0: the near-square rule of tile_order.h */                                                              \
  X(TN8_GROUP, "tn8_group", "VLB_GEMM_TN8_GROUP", 0)                                                                                    \
  /* ---- layernorm.hip (its variants ride on the same table) ---- */                                                                   \
  /* rows per wave of the forward: 1 | 2 | 4 (else: 2 where at least two full rounds of single-row waves exist) */                      \
  X(LN_FWD_ROWS, "ln_fwd_rows", "VLB_LN_FWD_ROWS", 0)                                                                                   \
  /* backward: 1 one row in flight per wave at H = 768 / 1024 | 2 two rows in flight there; any other value means 1 */                  \
  X(LN_BWD4, "ln_bwd4", "VLB_LN_BWD4", 1)

enum VlbOpt {
#define VLB_OPT_ID(id, name, env, dflt) VLB_OPT_##id,
  VLB_OPTIONS(VLB_OPT_ID)
#undef VLB_OPT_ID
  VLB_OPT_COUNT
};

int vlb_opt(VlbOpt o);                            // the knob's value: on first access reads the environment variable / fills the default
bool vlb_opt_set(const char* name, int value);    // run-time override by option name; false when no row has that name
