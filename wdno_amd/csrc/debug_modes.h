// debug_modes.h -- THE list of the library's debug modes (internal; the public entry point is wdno_set_debug, include/wdno_hip.h).
//
// One global integer, wdno_debug_mode (defined in api.cpp; set by wdno_set_debug() or, through the Python loader, by WDNO_DEBUG), steers
// kernel selection for A/B measurements and for tests that pin a kernel. 0 in production. Host code reads it at launch (or graph capture)
// time; the kernels that read it get it as a kernel argument (ConvP::debug from conv_common.h, the DWT geometry's `debug` from dwt_tiles.h).
// wdno_set_debug() refuses every value that is not listed here.
//
// One line per mode: value | files that read it | what it selects | results: "same bits" (bit-identical to mode 0), "tolerance" (another
// summation order or kernel: equal within the documented tolerances) or "WRONG" (an in-kernel ablation that skips work or overwrites the output
// with a timing; for measurements only). The values are quoted by DESIGN.md, INTEGRATION.md and profiles/: they do not change. Some numbers
// are read by several subsystems and switch all of them at once; those lines list every reader.
#pragma once

#define WDNO_DEBUG_MODES(X)                                                                                                                       \
  X(WDNO_DBG_OFF, 0)                    /* production */                                                                                           \
  /* 5 is a list, not one meaning: attention.hip, linattn.hip: thread-per-row softmax / thread-per-token linear-attention kernels, not the MFMA ones; \
     conv_h3.hip, conv_wgrad_h3.hip: forward and weight gradient on the register-staged kernels, never the LDS-DMA ones | tolerance */           \
  X(WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV, 5)                                                                                                      \
  X(WDNO_DBG_WGRAD_NO_XCD_GROUPING, 6)  /* conv_wgrad_h3.hip, conv_wgrad_h3d.hip: weight-gradient blocks / items in plain round-robin order | tolerance */ \
  X(WDNO_DBG_FORCE_DMA_CONV, 7)         /* conv_h3.hip: forward always on the LDS-DMA kernels, whatever the tile count | tolerance */            \
  /* 8: conv_h3.hip as 7; conv_h3t.hip: never the tap-resident forward; conv_wgrad_h3d.hip: never the window weight gradients | tolerance */     \
  X(WDNO_DBG_CHUNKED_DMA_CONV, 8)                                                                                                                  \
  /* 11 is a list: dwt.hip: the per-axis passes instead of the fused transform (same bits); conv_wgrad_h3d.hip: the window weight gradient       \
     only for K <= 64 (tolerance) */                                                                                                             \
  X(WDNO_DBG_PER_AXIS_DWT_AND_WGRAD_WINDOW_K64, 11)                                                                                                \
  X(WDNO_DBG_DWT_SKIP_W_PASS, 12)       /* dwt_synthesis.hip, in the fused synthesis kernel: without the W pass | WRONG */                      \
  X(WDNO_DBG_DWT_SKIP_H_PASS, 13)       /* dwt_synthesis.hip, same kernel (3-D): without the H pass | WRONG */                                  \
  X(WDNO_DBG_DWT_SKIP_T_PASS, 14)       /* dwt_synthesis.hip, same kernel (3-D): without the T pass and its stores | WRONG */                   \
  /* 21: conv_h3d.hip, conv_h3t.hip, conv_wgrad_h3d.hip, in the kernels: the DMA wave issues nothing, compute waves run on stale LDS | WRONG */   \
  X(WDNO_DBG_NO_DMA, 21)                                                                                                                           \
  X(WDNO_DBG_WGRAD_NO_DMA_NO_PIECE, 22) /* conv_wgrad_h3d.hip, in the kernel: as 21 and without the piece bookkeeping | WRONG */                 \
  /* 23 / 24 / 26: conv_h3d.hip, conv_h3t.hip, in the kernels: the recorded amax is replaced by a time measured by the block | WRONG */          \
  X(WDNO_DBG_STAMP_CYCLES, 23)          /* ... shader-clock cycles from kernel entry to the end */                                               \
  X(WDNO_DBG_STAMP_EPILOGUE, 24)        /* ... cycles spent in the epilogues */                                                                  \
  X(WDNO_DBG_STAMP_REALTIME, 26)        /* ... constant-rate (wall) clock ticks from kernel entry to the end */                                  \
  X(WDNO_DBG_FORCE_TILES_160, 30)       /* conv_h3.hip as 7; conv_h3d.hip: tap-resident tiles 160 x 128 (320 x 64 for K <= 64) | tolerance */    \
  X(WDNO_DBG_FORCE_TILES_320, 31)       /* conv_h3.hip as 7; conv_h3d.hip: tap-resident tiles 320 x 64 | tolerance */                            \
  X(WDNO_DBG_ATTN_GENERIC_NTOK, 44)     /* attention.hip: the generic-length MFMA kernels at 24 tokens, not the <24> instantiation | tolerance */ \
  X(WDNO_DBG_DWT3_SYNTH_LDS, 45)        /* dwt_synthesis.hip: 3-D synthesis with all frames of a tile in LDS, not the streaming kernel | same bits */      \
  X(WDNO_DBG_CONV_NO_RUN_SPLIT, 56)     /* conv_h3t.hip (read through conv_h3d.hip, conv_h3.hip): reductions never cut into four runs | tolerance */ \
  X(WDNO_DBG_STEM_EVERY_STAGE, 57)      /* conv_h3t.hip, in the kernel: the zero-box hint is ignored, every stage runs | same bits */            \
  X(WDNO_DBG_ATTN_FWD_ROWS, 67)         /* attention.hip: forward beyond 64 tokens on the thread-per-row kernel, not the tiled one | tolerance */ \
  X(WDNO_DBG_ATTN_BWD_ROWS, 68)         /* attention.hip: backward beyond 64 tokens likewise | tolerance */                                     \
  X(WDNO_DBG_WGRAD_NO_SPLIT_PAIR, 70)   /* conv_wgrad_h3d.hip: odd tap row paired with an empty window, not across two pixel splits | tolerance */ \
  X(WDNO_DBG_STEM_TILES_256, 72)        /* conv_h3t.hip: the 7-wide stem always on 256-pixel tiles, never 192 | same bits */                     \
  /* 100 + a stamp mode: that stamp with the DMA issue switched off as in 21 (conv_h3d.hip, conv_h3t.hip) | WRONG */                             \
  X(WDNO_DBG_NO_DMA_STAMP_CYCLES, 123)                                                                                                             \
  X(WDNO_DBG_NO_DMA_STAMP_EPILOGUE, 124)                                                                                                           \
  X(WDNO_DBG_NO_DMA_STAMP_REALTIME, 126)

enum wdno_debug : int {
#define WDNO_DBG_ENUM(name, value) name = value,
  WDNO_DEBUG_MODES(WDNO_DBG_ENUM)
#undef WDNO_DBG_ENUM
  WDNO_DBG_NO_DMA_OFFSET = 100          // not a mode: mode >= this means "mode - this, with the DMA issue off"
};

extern int wdno_debug_mode;             // api.cpp
