// norm_tiles.h -- the steps the GroupNorm kernels of norm.hip share, each stated once (gn_ prefix). A function stands here only where every
// kernel that calls it compiles to the code its inline form gave; the steps that did not come out like that keep their lines in the kernels,
// each with a one-line note (the figures: profiles/norm_tiles_header.md).
#pragma once
#include "common.h"
#include <type_traits>

#define GN_MAXC 1024
// blocks per sample of the planes backward at the most (gn_planes_grid): every block leaves one row of column-sum partials, so the workspace holds
// N * GN_PLANES_CAP rows of them
#define GN_PLANES_CAP 128

// Element type of an activation operand: float, or bf16 storage (single-product mode, WDNO_CONV_MATH=bf16: the convolution in front of a norm
// writes its output -- and the data gradient that reaches a norm's backward -- as bf16, train_diffusion.py:61-62 mixed-precision semantics;
// the arithmetic here stays fp32 / fp64). e = element offset of four / eight consecutive channels.
struct gn_bf16 {};
template <typename T> struct gn_ld;
template <> struct gn_ld<float> {
  static __device__ __forceinline__ float4 ld4(const void* p, int64_t e) { return *reinterpret_cast<const float4*>(static_cast<const float*>(p) + e); }
};
template <> struct gn_ld<gn_bf16> {
  static __device__ __forceinline__ float4 ld4(const void* p, int64_t e) {
    const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(p) + e);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
  }
};
template <typename T> __device__ __forceinline__ void gn_ld8(const void* p, int64_t e, float (&v)[8]) {
  const float4 a = gn_ld<T>::ld4(p, e), b = gn_ld<T>::ld4(p, e + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
typedef _Float16 gn_half8 __attribute__((ext_vector_type(8)));

// Per-channel totals of the chunk partials of sample n: sa[c], sb[c] for c < C (arrays of GN_MAXC doubles in LDS). All 256
// threads take part -- for C <= 128 a channel's chunk list is cut into 256 / C pieces that are folded through LDS -- so the
// chains of dependent loads are nchunk * C / 256 long instead of nchunk (these one-block-per-sample kernels are pure latency:
// 8.6 and 16.6 us per launch before, ~100 launches per train step).
// (cb0, cn: the channels cb0 .. cb0 + cn - 1 only, results at sa / sb[0 .. cn) -- the finalize kernels run one block per (sample, slice of groups))
__device__ __forceinline__ void gn_chunk_totals(const double* __restrict__ part, int n, int nchunk, int Call, double* sa, double* sb, int cb0 = 0, int cn = -1) {
  const int C = cn < 0 ? Call : cn;
  part += cb0 * 2;
  const int nsub = C <= 128 ? 256 / C : 1;
  for (int idx = threadIdx.x; idx < C * nsub; idx += 256) {
    const int q = idx / C, c = idx - q * C;
    const int k1 = (q + 1) * nchunk / nsub;
    int k = q * nchunk / nsub;
    double a0 = 0, b0 = 0, a1 = 0, b1 = 0;             // two chains (even / odd chunks), as before -- but the loads of EIGHT chunks are
    // requested before the first is added: the adds were chained behind one L2 round trip per pair of chunks (16 chunks per thread at
    // C = 64: ~6 of the 8.8 us of a launch that 8 blocks make 30 times per step, forward and backward)
    for (; k + 7 < k1; k += 8) {
      const double* q0 = part + (((int64_t)n * nchunk + k) * Call + c) * 2;
      double va[8], vb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { va[u] = q0[(int64_t)u * Call * 2]; vb[u] = q0[(int64_t)u * Call * 2 + 1]; }
#pragma unroll
      for (int u = 0; u < 8; u += 2) { a0 += va[u]; b0 += vb[u]; a1 += va[u + 1]; b1 += vb[u + 1]; }
    }
    for (; k + 1 < k1; k += 2) {
      const double* q0 = part + (((int64_t)n * nchunk + k) * Call + c) * 2;
      const double* q1 = q0 + (int64_t)Call * 2;
      a0 += q0[0]; b0 += q0[1]; a1 += q1[0]; b1 += q1[1];
    }
    if (k < k1) {
      const double* q0 = part + (((int64_t)n * nchunk + k) * Call + c) * 2;
      a0 += q0[0]; b0 += q0[1];
    }
    sa[idx] = a0 + a1; sb[idx] = b0 + b1;               // idx = q * C + c
  }
  __syncthreads();
  if (nsub > 1) {
    const int c = threadIdx.x;
    double a = 0, b = 0;
    if (c < C)
      for (int q = 0; q < nsub; ++q) { a += sa[q * C + c]; b += sb[q * C + c]; }
    __syncthreads();
    if (c < C) { sa[c] = a; sb[c] = b; }
    __syncthreads();
  }
}

// A finalize block = (sample blockIdx.x, slice blockIdx.y of the groups): the statistics of the groups are independent, and with one block per sample
// the launch was a chain of dependent loads over nchunk x C partials -- 7.5 us per norm, 60 such launches per training step; a slice of one group of
// 8 channels reads 8 KB of them. A block with gs0 >= gs1 has no group and returns; the others move their parameter and table pointers to the slice's
// first channel / group and index their LDS tables from there.
// (the pointers are moved by the kernel: a function that takes them by reference changed both finalize kernels, profiles/norm_tiles_header.md)
struct gn_slice {
  int gs0, gs1;      // groups gs0 .. gs1 - 1
  int cs0, csn;      // first channel, number of channels
};
__device__ __forceinline__ gn_slice gn_block_slice(int cg, int G) {
  gn_slice sl;
  const int gps = (G + (int)gridDim.y - 1) / (int)gridDim.y;
  sl.gs0 = (int)blockIdx.y * gps; sl.gs1 = min(G, sl.gs0 + gps);
  sl.cs0 = sl.gs0 * cg; sl.csn = (sl.gs1 - sl.gs0) * cg;
  return sl;
}

// Block maximum of Q floats (256 threads): m holds the WAVE maxima (wave_max at the call site), which go through LDS to thread 0.
// true: this is thread 0, and t holds the block maxima.
template <int Q>
__device__ __forceinline__ bool gn_block_max(const float (&m)[Q], float (&t)[Q]) {
  __shared__ float bm[Q][4];
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < Q; ++q) bm[q][threadIdx.x >> 6] = m[q];
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int q = 0; q < Q; ++q) t[q] = fmaxf(fmaxf(bm[q][0], bm[q][1]), fmaxf(bm[q][2], bm[q][3]));
  return true;
}

// What a thread of a planes kernel fixes before its loop: the plane scale and its channels.
// single: one bf16 plane, no scale (lo == nullptr: WDNO_CONV_MATH=bf16). Otherwise the scale comes from the bound the finalize kernel left in `rec`
// (RES: + max|res|, the amax record of the residual); one thread of the grid then writes it to scale_out -- that line stays in the kernels (inside
// the function it changed all eight planes kernels, profiles/norm_tiles_header.md).
template <bool RES = false>
__device__ __forceinline__ float gn_planes_scale(bool single, const float* __restrict__ rec, const float* __restrict__ rec_res = nullptr) {
  return single ? 1.0f : scale_from_amax(RES ? amax_record_read(rec) + amax_record_read(rec_res) : amax_record_read(rec));
}
// A thread owns 8 consecutive channels, the same ones in every round of its grid-stride loop: the host launches the planes kernels only with
// (gridDim.x * 256) % C8 == 0 -- C8 = C / 8 is a power of two <= 256 (gn_planes_ok). So the channel tables and the column sums can stay in registers.
__device__ __forceinline__ int gn_planes_c0(int C8) { return (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % C8) * 8; }

// The forward element: y = act(a x + b) with the folded per-channel affine (a, b) of gn_finalize_kernel.
__device__ __forceinline__ float gn_fwd_elem(float a, float b, float x, int silu) {
  float o = a * x + b;
  if (silu) o = silu_f(o);
  return o;
}
// The backward element. k = cb[n][c] = (a, b, k1 (s + 1), 0); g = gb[n][group] = (mean, rstd, and the two group means gn_bwd_finalize_kernel adds):
// dz = dy * act'(a x + b), xhat = (x - mean) * rstd, dx = k.z dz - g.z - xhat g.w. k and g are locals of the caller (given cbp[c] itself, the loads of k.x, k.y sank into the silu branch).
__device__ __forceinline__ float gn_bwd_dz(float dy, float a, float b, float x, int silu) {
  float dz = dy;
  if (silu) dz *= silu_grad_f(a * x + b);
  return dz;
}
__device__ __forceinline__ float gn_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float gn_bwd_elem(const float4& k, const float4& g, float x, float dy, int silu) {
  const float dz = gn_bwd_dz(dy, k.x, k.y, x, silu);
  const float xh = gn_xhat(x, g.x, g.y);
  return k.z * dz - g.z - xh * g.w;
}

// Channel j of a thread's eight as planes: (hi, lo) fp16 of o * s, or one bf16 in the hi plane (single). The two 16-byte stores of h and l stay in the
// kernels, behind the loop that fills them (as a function, with or without the packing, they changed all eight planes kernels).
__device__ __forceinline__ void gn_pack_at(gn_half8& h, gn_half8& l, int j, float o, float s, bool single) {
  _Float16 th, tl;
  plane_pack(o, s, single, th, tl);
  h[j] = th; l[j] = tl;
}
