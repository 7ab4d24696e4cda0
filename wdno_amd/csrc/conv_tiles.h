// conv_tiles.h -- the lane-level steps the 16-bit convolution kernels share, each written once (prefix cv_): the split-fp16 / bf16 forward,
// data-gradient and weight-gradient kernels of conv_h3.hip, conv_h3d.hip, conv_h3t.hip, conv_wgrad_h3.hip and conv_wgrad_h3d.hip.
// conv_common.h keeps the host side (ConvP, geometry, the choosers' declarations, fill_params). Every function here is __forceinline__ and
// replaces an inline site only where the kernel compiles to the same code (profiles/conv_tiles_header.md); a site that did not come out that way
// keeps its inline form and says so. A name with a per-file prefix (t_, wd_, ...) exists in that file alone.
#pragma once
#include "conv_common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int int4v __attribute__((ext_vector_type(4)));
// Buffer offset of a piece / load that must deliver zeros (zero padding, ragged tile tails, the pipeline tail): beyond the range of every
// descriptor the host wrappers accept, so the hardware bounds check answers -- no branch and no select.
#define CV_OOB 0x7ffffff0

// LP ("low precision", BASELINE.json configs[1]): ONE bf16 plane per operand and one v_mfma_f32_32x32x16_bf16 per fragment pair
// instead of the (hi, lo) fp16 planes and three products: a third of the matrix instructions, half of the DMA pieces and of
// the LDS traffic; fp32 accumulators, bias / residual / output stay fp32; no scale (bf16 has the fp32 exponent range).
template <bool LP>
__device__ __forceinline__ f32x16 cv_mfma(half8 a, half8 b, f32x16 c) {
  if constexpr (LP) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// A raw buffer descriptor as four SGPR words for the hand-written loads below (stride 0, bounds = bytes).
__device__ __forceinline__ int4v cv_rsrc(const void* ptr, unsigned bytes) {
  uint64_t a = reinterpret_cast<uint64_t>(ptr);
  int4v r;
  r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)((a >> 32) & 0xffffu));
  r.z = __builtin_amdgcn_readfirstlane((int)bytes);
  r.w = 0x00020000;
  return r;
}
// one 1-KiB LDS-DMA piece: lane l's 16 bytes at buffer offset `off` land at LDS byte address lds_dst + 16*l. One VMEM instruction per call:
// the callers count them for their s_waitcnt vmcnt(N).
// PIN_DST: readfirstlane of lds_dst first (wave-uniform by construction; with the nine pieces per wave of conv_h3t.hip the compiler kept it in
// a vector register)
template <bool PIN_DST = false>
__device__ __forceinline__ void cv_piece(int4v rsrc, int off, unsigned lds_dst) {
  if constexpr (PIN_DST) lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds" : : "v"(off), "s"(lds_dst), "s"(rsrc) : "memory");
}
// hipcc turns every counted prefetch of compiler-visible loads into s_waitcnt vmcnt(0) at the next use, which drains the
// queue once per step and leaves the kernel latency bound. This load is therefore invisible to its bookkeeping: the
// destination counts as written at issue, and the kernel waits for it itself, naming the registers.
__device__ __forceinline__ int4v cv_load_b128(int4v rsrc, int byte_off) {
  int4v v;
  asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(byte_off), "s"(rsrc) : "memory");
  return v;
}
// s_waitcnt lgkmcnt(0) + s_barrier. The wait is the BUILTIN so that the compiler's own s_waitcnt bookkeeping sees it: behind an
// asm-only wait it still counts the scalar loads of the previous tile's epilogue as possibly outstanding at the head of the
// step loop, and (scalar loads return out of order) protects the first MFMA of every step with lgkmcnt(0) -- a wait for the
// LDS reads issued just before it.
__device__ __forceinline__ void cv_lgkm0_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);
  asm volatile("s_barrier" : : : "memory");
}

template <int TM, int TN>
__device__ __forceinline__ void cv_zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
}
// The products of one fragment set over a TM x TN accumulator tile: al bh, ah bl, ah bh in this order (LP: the one bf16 product), each pass
// over the whole tile so that consecutive MFMAs never depend on each other. A_ROW: the a fragment is the MFMA row operand (the register-staged
// kernels: accumulator [pixel][channel]); otherwise the b fragment is (the LDS-DMA kernels: [channel][pixel] / [r][k]).
template <bool LP, bool A_ROW, int TM, int TN>
__device__ __forceinline__ void cv_mfma_set(f32x16 (&acc)[TM][TN], const half8 (&ah)[TM], const half8 (&al)[TM], const half8 (&bh)[TN], const half8 (&bl)[TN]) {
  if constexpr (!LP) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b) acc[a][b] = A_ROW ? cv_mfma<false>(al[a], bh[b], acc[a][b]) : cv_mfma<false>(bh[b], al[a], acc[a][b]);
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
      for (int b = 0; b < TN; ++b) acc[a][b] = A_ROW ? cv_mfma<false>(ah[a], bl[b], acc[a][b]) : cv_mfma<false>(bl[b], ah[a], acc[a][b]);
  }
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b) acc[a][b] = A_ROW ? cv_mfma<LP>(ah[a], bh[b], acc[a][b]) : cv_mfma<LP>(bh[b], ah[a], acc[a][b]);
}
// One scheduling region per (half-)step: the NRD fragment reads of the NEXT one are dealt out behind the NMF MFMAs of this one, RPM reads per MFMA
// until they are used up (not all reads first: a wave issues in order, so a block of ds_reads ahead of the MFMAs adds its issue time to every
// step; conv_h3t.hip has the measurement).
template <int NRD, int NMF>
__device__ __forceinline__ void cv_interleave() {
  constexpr int RPM = (NRD + NMF - 1) / NMF;
#pragma unroll
  for (int i = 0; i < NMF; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if (i * RPM < NRD) __builtin_amdgcn_sched_group_barrier(0x100, RPM, 0);
  }
}

// bf16 storage of two accumulator runs (channels 8 e + 4 hh .. + 3 and 8 (e + 1) + 4 hh .. + 3 of one pixel, the two lane halves hh = 0 / 1
// holding the two halves of each group of eight): the halves trade runs (v_permlane32_swap), so that the lower half ends up with the eight
// channels of group e and the upper half with those of group e + 1 -- ONE 16-byte store per lane instead of two 8-byte ones (with the
// 8-byte stores the 256 x 128 single-plane kernel of the Burgers U-Net lost 2.7 %: 356 vs 366 us per launch).
__device__ __forceinline__ uint4 cv_bf16x8_from_runs(float4 va, float4 vb) {
  const uint2 A = bf16x4_pack(va), B = bf16x4_pack(vb);
  const auto sx = __builtin_amdgcn_permlane32_swap(A.x, B.x, false, false);
  const auto sy = __builtin_amdgcn_permlane32_swap(A.y, B.y, false, false);
  return make_uint4(sx[0], sy[0], sx[1], sy[1]);
}
// WDNO_DBG_STAMP_CYCLES / _EPILOGUE / _REALTIME (tools/bench_conv.py --stamps): the amax record of the LDS-DMA forward kernels carries the wave's
// shader cycles in the kernel / in the tile epilogues / its 100 MHz wall ticks instead of max|y|. cv_stamps_begin at the head of the compute
// waves, the epilogue adds its cycles to c_epi, cv_stamps_value is what the record gets.
struct CvStamps {
  int sdbg;
  bool on;
  uint64_t c_begin, r_begin, c_epi;
};
__device__ __forceinline__ CvStamps cv_stamps_begin(int debug) {
  CvStamps s;
  s.sdbg = debug >= WDNO_DBG_NO_DMA_OFFSET ? debug - WDNO_DBG_NO_DMA_OFFSET : debug;      // the same stamp with the DMA issue switched off (WDNO_DBG_NO_DMA)
  s.on = s.sdbg == WDNO_DBG_STAMP_CYCLES || s.sdbg == WDNO_DBG_STAMP_EPILOGUE || s.sdbg == WDNO_DBG_STAMP_REALTIME;
  s.c_begin = s.on ? __builtin_amdgcn_s_memtime() : 0;
  s.r_begin = s.on ? __builtin_amdgcn_s_memrealtime() : 0;
  s.c_epi = 0;
  return s;
}
__device__ __forceinline__ float cv_stamps_value(const CvStamps& s) {
  return s.sdbg == WDNO_DBG_STAMP_CYCLES ? (float)(__builtin_amdgcn_s_memtime() - s.c_begin) : s.sdbg == WDNO_DBG_STAMP_EPILOGUE ? (float)s.c_epi : (float)(__builtin_amdgcn_s_memrealtime() - s.r_begin);
}
