// linattn_fused.h -- what only the fused SpatialLinearAttention kernels share: the launch parameters of the forward passes (linattn_fused.hip: 64
// channels; linattn_fused_wide.hip: 128 / 256) and the cut of a frame into token chunks (forward and linattn_fused_bwd.hip). The lane-level steps are
// in attn_fused.h.
#pragma once
#include "attn_fused.h"

#define LF_PART (32 + 32 + 32 * 32)          /* floats per (block, head) of the first pass: m[32], Z[32], ctx_raw[32][32] */

struct LFusedP {
  const float* x; const float* gamma; float eps;
  const _Float16* wq_hi; const _Float16* wq_lo; const float* wq_scale;      // packed forward operand of to_qkv: [384][64]
  const _Float16* wo_hi; const _Float16* wo_lo; const float* wo_scale;      // ... of to_out: [64][128]
  const float* bias_out;
  float* part;               // first pass: [units][chunks][heads][LF_PART]
  const float* ctx;          // second pass: [units][heads][32][32] (ctx[d][e])
  float* y; float* amax_rec;
  int n_tok, chunks, tiles_per_chunk; float scale;
};

// token chunks per frame: ~3 blocks per CU in flight, at least two tiles each. The layout of the forward's workspace and of the backward's
// first pass (one partial per chunk) both follow from it.
static inline int lf_chunks(int64_t units, int n_tok) {
  const int ntiles = (n_tok + 31) / 32;
  int64_t c = (3 * (int64_t)wdno_num_cus() + units - 1) / units;
  if (c > ntiles / 2) c = ntiles / 2;
  if (c < 1) c = 1;
  if (c > 64) c = 64;
  return (int)c;
}
// tiles (32 tokens) a chunk walks when a frame is cut into `chunks`: trailing chunks may be short or empty
static inline int lf_tiles_per_chunk(int n_tok, int chunks) {
  const int ntiles = (n_tok + 31) / 32;
  return (ntiles + chunks - 1) / chunks;
}
