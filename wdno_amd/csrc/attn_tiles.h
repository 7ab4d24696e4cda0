// attn_tiles.h -- the lane-level steps of the layer-by-layer attention kernels, each written once under the am_ prefix:
//   softmax attention   attention.hip (one wave per (unit, head) on 32 x 32 tiles, 48 / 64 tokens on two tiles, key tiles with an online softmax)
//   linear attention    linattn.hip (the token kernels on the same tiles and accumulator layout)
// The work-item decode, rows staged into LDS tiles and read back as matrix operands, rows and columns loaded straight into the accumulator
// layout, the two shapes of the exact-fp32 product (v_mfma_f32_32x32x2_f32: sixteen steps; four steps and a scheduling barrier), the masked
// maximum / exp / sum of a softmax over the keys of a lane pair, the row store with its running amax and the row store as fp16 planes, the
// rotation gradient, and the dynamic-LDS opt-in of the launchers. A step only one kernel has stays in its unit, and so does a copy of a step
// at a site where the shared function compiled to other code than the inline form (each such site says so in one line). The arithmetic is
// pinned element by element (tests/test_gpu_attn_kernels_matrix.py); what the compiler made of each kernel before and after these functions
// existed is in profiles/attn_tiles_header.md.
#pragma once
#include "attn_fused.h"      // f32x16; tf_key: the key / feature an accumulator register of a lane half holds; tf_zero

#define DH 32
#define AM_WAVES 4           /* waves (work items in flight) per block of the one-wave-per-item kernels */

// opt a kernel in to `bytes` of dynamic LDS (the runtime refuses a launch above 64 KB without it). Whether a launcher asks every time, only
// above 64 KB or once per process is the launcher's choice: these launches are captured into graphs.
static inline void am_dyn_lds(const void* kernel, size_t bytes) {
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// work item (unit, head) -> head and the row of the item's token 0 in the [rows][features] tensors; a thread without an item
// (!active: the thread-per-row kernels) gets those of item 0. d by value: a reference to a kernel argument costs scalar code.
struct AmItem { int h; int64_t row0; };
__device__ __forceinline__ AmItem am_item(const wdno_attn_desc d, int64_t item, bool active = true) {
  const int h = active ? (int)(item % d.heads) : 0;
  const int64_t unit = active ? item / d.heads : 0;
  const int uo = (int)(unit / d.n_ui), ui = (int)(unit - (int64_t)uo * d.n_ui);
  return AmItem{h, (int64_t)uo * d.so + (int64_t)ui * d.si};
}

// The MFMA accumulator layout gives lane (li, hh) the channel runs 8 e4 + 4 hh + (0..3) of its row: 8-byte plane stores. One
// v_permlane32_swap per component trades the odd run of the low half-wave for the even run of the high one (tools/probes/swap_probe.hip),
// after which a lane owns 8 CONSECUTIVE channels (16 j + 8 hh + 0..7) of each pair j: 16-byte stores. v[e4] = the four runs; off0 = element
// offset of channel 0 of this head in the lane's row. Both lanes of a pair (l, l + 32) must be active.
__device__ __forceinline__ void am_store_row_planes(_Float16* hi, _Float16* lo, int64_t off0, int hh, const float4* v, float s) {
  typedef _Float16 half8v __attribute__((ext_vector_type(8)));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float a[4] = {v[2 * j].x, v[2 * j].y, v[2 * j].z, v[2 * j].w}, b[4] = {v[2 * j + 1].x, v[2 * j + 1].y, v[2 * j + 1].z, v[2 * j + 1].w};
    float t[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a[c]), __float_as_uint(b[c]), false, false);
      t[c] = __uint_as_float(r[0]); t[4 + c] = __uint_as_float(r[1]);
    }
    half8v h, l;
#pragma unroll
    for (int c = 0; c < 8; ++c) { _Float16 th, tl; plane_pack(t[c], s, lo == nullptr, th, tl); h[c] = th; l[c] = tl; }
    const int64_t off = off0 + 16 * j + 8 * hh;
    *reinterpret_cast<half8v*>(hi + off) = h;
    if (lo) *reinterpret_cast<half8v*>(lo + off) = l;
  }
}

// wave-uniform pointer in SGPRs: the per-lane part of an address stays a 32-bit offset (global_load saddr + voffset)
__device__ __forceinline__ const float* am_uniform(const float* p) {
  uint64_t a = reinterpret_cast<uint64_t>(p);
  unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
}

// Rows of one operand ([n][32] floats: q, k, v or dO of one head) -> LDS tile [32][AM_TS], loaded cooperatively (8 lanes
// per 128-byte row, three passes for 24 rows), optionally scaled and rotated on the way; rows >= n are zero-filled.
#define AM_TS 36
template <int NIF = 4>
__device__ __forceinline__ void am_stage_rows(float* __restrict__ tile, const float* __restrict__ ubase, unsigned row_stride,
                                              const float* __restrict__ rc, const float* __restrict__ rs, float scale, int n, int lane) {
  // ubase: wave-uniform pointer to row 0 of the operand (am_uniform); the per-lane part of every address is a 32-bit offset,
  // so nothing 64-bit per lane has to stay live across the item loop
  // NIF of the four 1-KiB row groups are requested together (4 KB in flight per wave; one at a time, sixteen waves per CU keep only
  // ~4 MB in flight chip-wide and the kernel sits at a latency-bound 2.9 TB/s); the rotation tables are fetched pass by pass.
  // NIF = 2 halves the staging registers where the caller is short of them.
#pragma unroll
  for (int k0 = 0; k0 < 4; k0 += NIF) {
    float4 xs[NIF];
#pragma unroll
    for (int k = 0; k < NIF; ++k) {
      const int idx = lane + 64 * (k0 + k);
      const int r = idx >> 3, c4 = (idx & 7) * 4;
      xs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < n) xs[k] = *reinterpret_cast<const float4*>(ubase + ((unsigned)r * row_stride + (unsigned)c4));
    }
#pragma unroll
    for (int k = 0; k < NIF; ++k) {
      const int idx = lane + 64 * (k0 + k);
      const int r = idx >> 3, c4 = (idx & 7) * 4;
      float4 x = xs[k];
      x.x *= scale; x.y *= scale; x.z *= scale; x.w *= scale;
      if (rc && r < n) {
        const float4 c = *reinterpret_cast<const float4*>(rc + r * DH + c4), sn = *reinterpret_cast<const float4*>(rs + r * DH + c4);
        x = make_float4(x.x * c.x - x.y * sn.x, x.y * c.y + x.x * sn.y, x.z * c.z - x.w * sn.z, x.w * c.w + x.z * sn.w);
      }
      *reinterpret_cast<float4*>(tile + r * AM_TS + c4) = x;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}
// the 16 values of row `li` this lane feeds to the MFMA steps of a product that contracts over the 32 channels: step m takes the
// channel pair (m, 16 + m), i.e. lane half hh holds channels d = 16 hh + m -- 16 CONSECUTIVE floats, four conflict-free ds_read_b128
// (any pairing of channels into steps is valid as long as both operands use it; the first version, d = 2 m + hh, needed sixteen
// ds_read_b32 at a row stride of 36 floats = 4-way bank conflicts, a fifth of the temporal-attention kernels' LDS cycles)
#define AM_D(m, hh) (16 * (hh) + (m))
__device__ __forceinline__ void am_sel(const float* __restrict__ tile, int li, int hh, float* sel) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(tile + li * AM_TS + 16 * hh + 4 * q);
    sel[4 * q] = v.x; sel[4 * q + 1] = v.y; sel[4 * q + 2] = v.z; sel[4 * q + 3] = v.w;
  }
}
// four of them (steps 4 g .. 4 g + 3)
__device__ __forceinline__ void am_sel4(const float* __restrict__ tile, int li, int hh, int g, float* sel) {
  const float4 v = *reinterpret_cast<const float4*>(tile + li * AM_TS + 16 * hh + 4 * g);
  sel[0] = v.x; sel[1] = v.y; sel[2] = v.z; sel[3] = v.w;
}

// gradient of the rotation on a run of four consecutive channels d0..d0+3 held by one lane (pairs are inside the run)
__device__ __forceinline__ float4 am_unrotate4(float4 g, const float* __restrict__ rc, const float* __restrict__ rs, int d0) {
  if (!rc) return g;
  const float4 c = *reinterpret_cast<const float4*>(rc + d0), s = *reinterpret_cast<const float4*>(rs + d0);
  return make_float4(g.x * c.x + g.y * s.x, g.y * c.y - g.x * s.y, g.z * c.z + g.w * s.z, g.w * c.w - g.z * s.w);
}

// ---------------------------------------------------------------------------------------------- operands in accumulator layout
// Row of a token as the 16 values a lane feeds to a product over the features: the four runs 8 c + 4 hh + (0..3) of its 32 features, four
// 16-byte loads. p = feature 0 of the row (global memory or an LDS tile); zeros when !ok; times mul.
__device__ __forceinline__ void am_row16(const float* p, int hh, bool ok, float mul, float (&v)[16]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 v4 = ok ? *reinterpret_cast<const float4*>(p + 8 * c + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
    v[4 * c] = v4.x * mul; v[4 * c + 1] = v4.y * mul; v[4 * c + 2] = v4.z * mul; v[4 * c + 3] = v4.w * mul;
  }
}
// Column `col` of the 16 tokens t0 + tf_key(m, hh) (step m of a product over the tokens; coalesced 128-byte rows): V[key][d = li] for
// O^T += V^T P^T. base = wave-uniform pointer to token 0, the per-lane part a 32-bit offset; zeros beyond n; times mul.
__device__ __forceinline__ void am_col16(const float* base, unsigned stride, int t0, unsigned col, int n, int hh, float mul, float (&v)[16]) {
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const int t = t0 + tf_key(m, hh);
    v[m] = t < n ? base[(unsigned)t * stride + col] * mul : 0.f;
  }
}
// quarter c of an accumulator: the run 8 c + 4 hh + (0..3) of the lane's row
__device__ __forceinline__ float4 am_quarter(const f32x16& a, int c) { return make_float4(a[4 * c], a[4 * c + 1], a[4 * c + 2], a[4 * c + 3]); }

// ---------------------------------------------------------------------------------------------- the two shapes of the exact-fp32 product
// c += A B, sixteen steps of two reduction indices each; a[m], b[m] = the lane's row / column operand of step m
template <class A, class B>
__device__ __forceinline__ f32x16 am_mfma16(const A& a, const B& b, f32x16 c) {
#pragma unroll
  for (int m = 0; m < 16; ++m) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[m], c, 0, 0, 0);
  return c;
}
// four steps of such a product and a scheduling barrier: nothing moves across the end of a group -- bounded live registers (the backward
// kernel, which fetches its operands group by group, runs at 128 VGPRs)
template <class A, class B>
__device__ __forceinline__ f32x16 am_mfma4(const A& a, const B& b, f32x16 c) {
#pragma unroll
  for (int q = 0; q < 4; ++q) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], c, 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  return c;
}

// ---------------------------------------------------------------------------------------------- softmax over the keys of a lane pair
// Transposed score tile of this lane's query: register e = key k0 + tf_key(e, hh); the other half of the keys sits in lane ^ 32.
// Masked maximum: the bias row added where there is one, keys beyond n set to -inf (in place).
__device__ __forceinline__ float am_masked_max(f32x16& sT, const float* __restrict__ brow, int k0, int n, int hh, bool tok) {
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int j = k0 + tf_key(e, hh);
    float v = sT[e];
    if (brow && tok && j < n) v += brow[j];
    v = j < n ? v : -INFINITY;
    sT[e] = v;
    mx = fmaxf(mx, v);
  }
  return fmaxf(mx, __shfl_xor(mx, 32));
}
// exp(s - m) in place over NT such tiles, and its sum over the keys of the pair
template <int NT>
__device__ __forceinline__ float am_exp_sum(f32x16* sT, float m) {
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) { sT[t][e] = expf(sT[t][e] - m); l += sT[t][e]; }
  return l + __shfl_xor(l, 32);
}
// one tile, normalised in place: softmax over the keys of query `li` from the transposed score tile (masked beyond n); returns P^T
__device__ __forceinline__ void am_softmax(f32x16& sT, const float* __restrict__ brow, int n, int hh, bool tok) {
  const float mx = am_masked_max(sT, brow, 0, n, hh, tok);
  const float inv = 1.0f / am_exp_sum<1>(&sT, mx);
#pragma unroll
  for (int e = 0; e < 16; ++e) sT[e] *= inv;
}

// ---------------------------------------------------------------------------------------------- results
// Store a row of the result in accumulator layout (row = feature 0 of the lane's row) and fold it into the lane's running amax. The sites
// that can deliver fp16 planes instead (am_store_row_planes) keep their store loops: with the choice inside a shared function the compiler
// duplicates the amax on both paths or reorders the waits of the three backward stores (profiles/attn_tiles_header.md).
__device__ __forceinline__ void am_store_row(const f32x16& acc, float* row, int hh, float& am) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 v = am_quarter(acc, c);
    *reinterpret_cast<float4*>(row + 8 * c + 4 * hh) = v;
    am = amax4(am, v);
  }
}
