// fastdiv.h -- n / d for 0 <= n, n * d < 2^32 as one multiply-high (m = floor(2^32 / d) + 1). A hardware integer division is ~30 VALU
// instructions on gfx950: the item loops of the wavelet kernels (dwt_tiles.h) decode (row, column) from a linear index several times per
// item -- with divisions the 3-D synthesis kernel was ALU-bound at 50 us for 38 MB --, and four per float4 made pack_smoke_state_kernel
// ALU-bound (33 us for 78 MB, profiles/r06_pack_kernel_stats.md). The caller checks the range on the host. (conv_prep.hip keeps a copy of its
// own, ps_div: its kernels change on this one.)
#pragma once
#include <hip/hip_runtime.h>

struct FastDiv { unsigned d, m; };
__host__ __device__ __forceinline__ FastDiv make_fastdiv(int d) {
  FastDiv f;
  f.d = (unsigned)d;
  f.m = d > 1 ? (unsigned)((1ull << 32) / (unsigned)d + 1ull) : 0u;
  return f;
}
__device__ __forceinline__ unsigned fd_div(unsigned n, FastDiv f) { return f.d == 1 ? n : __umulhi(n, f.m); }
__device__ __forceinline__ int fd_div(int n, FastDiv f) { return (int)fd_div((unsigned)n, f); }
