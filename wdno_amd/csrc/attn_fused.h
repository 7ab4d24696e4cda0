// attn_fused.h -- the lane-level steps of the fused attention family, each written once under the tf_ prefix:
//   temporal attention         attn_fused.hip (24 frames), attn_fused48.hip (48), attn_fused_wide.hip (128 / 256 channels), attn_fused_bwd.hip
//   spatial linear attention   linattn_fused.hip, linattn_fused_wide.hip, linattn_fused_bwd.hip (through linattn_fused.h where they share more)
// Reductions (DPP / permlane), streamed-fragment loads and waits, accumulator helpers and the split MFMA, transpose reads of the swizzled
// W image, (hi, lo) splits, LayerNorm rows, the rotary / bias tables, and the steps of the temporal forward pass (projection, rotary,
// softmax over 24 keys, to_out, head sum). A name with another prefix (t48_, tb_, lw_, lb_, ...) is a thing only its own file has.
// The arithmetic of these steps is pinned bit for bit by the tests (fused == layer by layer, 24 == 48 frames == wide == backward recompute):
// the expression trees -- in particular the orders of the sums -- are part of the contract.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));

// Streamed weight fragments (attn_fused_wide.hip, linattn_fused_wide.hip): raw buffer loads, address = descriptor (SGPRs) + one loop-invariant
// 32-bit lane offset (VGPR) + a uniform offset (SGPR) -- no address arithmetic in the vector registers.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tf_rsrc(const void* ptr, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ half8 tf_frag(__amdgpu_buffer_rsrc_t r, unsigned lane_bytes, unsigned uniform_bytes) {
  return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(r, (int)lane_bytes, (int)uniform_bytes, 0));
}
// Hand-over of streamed fragments: a trip of the streaming loops requests two sets, waits for them IN FULL (s_waitcnt vmcnt(0)), then runs their
// matrix instructions -- no fragment load is in flight while the matrix pipe reads fragments. The overlapped form (the loads of set B in
// flight while the matrix instructions consume set A, handed over by the counted waits vmcnt(5), vmcnt(1), ... the compiler derives -- or
// by full waits) gave run-to-run differences of ~1e-6 in the first pass of the 256-channel linear-attention block whenever two blocks shared
// a CU: not with one block per CU, not with constant fragments or constant token planes, not with this serial form; unchanged by 64-bit lane
// vs buffer addressing, by extra barriers, by idle cycles behind the matrix instructions (tools/probes/lattn_wide_repro.py; the cause was not
// found -- the counted waits are correct for in-order returns). The other waves of the SIMD fill the wait: no time lost (measured), so every
// streaming loop of the wide kernels uses the serial form; tests/test_gpu_wide_repro.py repeats each kernel 40 times under two blocks per CU.
// The fragments are tied to the asm statements so that no consumer is scheduled above the wait and no later load above the consumers.
#define TF_WAIT_SET4(a, b, c, d) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) :: "memory")
#define TF_WAIT_SET8(a, b, c, d, e, f, g, h) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) :: "memory")
#define TF_WAIT_SET12(a, b, c, d, e, f, g, h, i, j, k, l) \
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i), "+v"(j), "+v"(k), "+v"(l) :: "memory")

#define TF_C 64
#define TF_NT 24
#define TF_HEADS 4
#define TF_HD 128
#define TF_AST 72     /* halves per token row of an A plane (144 B) */
#define TF_VST 36     /* floats per row of the V tile */
#define TF_YST 68     /* floats per row of a partial output tile */
#define TF_RST 18     /* float2 per row of the rotary table (16 pairs + pad: the two lane halves start 2 pairs apart) */
#define TF_BST 28     /* floats per query row of the bias table (24 keys + pad: conflict-free 16-byte reads down a column of rows) */
#define TF_PS 36      /* halves per row of a per-head plane tile (the backward kernels' transpose reads) */

__device__ __forceinline__ int tf_key(int m, int hh) { return 8 * (m >> 2) + 4 * hh + (m & 3); }

// Reductions without the LDS crossbar (a __shfl_xor is a ds_bpermute: ~100 cycles of latency each, and the LayerNorm of a row is a chain of
// eight of them): DPP operands inside a row of 16 lanes -- quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror -- leave the
// sum / maximum of the row in all of its lanes; v_permlane32_swap joins the two halves of the wave.
template <int CTRL>
__device__ __forceinline__ float tf_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float tf_row16_sum(float v) {
  v += tf_dpp<0xB1>(v); v += tf_dpp<0x4E>(v); v += tf_dpp<0x141>(v); v += tf_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ float tf_row16_max(float v) {
  v = fmaxf(v, tf_dpp<0xB1>(v)); v = fmaxf(v, tf_dpp<0x4E>(v)); v = fmaxf(v, tf_dpp<0x141>(v)); v = fmaxf(v, tf_dpp<0x140>(v));
  return v;
}
__device__ __forceinline__ float tf_wave_max(float v) {      // uniform result
  v = tf_row16_max(v);
  const unsigned u = __float_as_uint(v);
  const float a = __uint_as_float(__builtin_amdgcn_readlane(u, 0)), b = __uint_as_float(__builtin_amdgcn_readlane(u, 16));
  const float c = __uint_as_float(__builtin_amdgcn_readlane(u, 32)), d = __uint_as_float(__builtin_amdgcn_readlane(u, 48));
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ void tf_halves(float v, float& lo, float& hi) {      // the value of lane (l & 31) and of lane (l & 31) + 32, in every lane
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  lo = __uint_as_float(r[0]); hi = __uint_as_float(r[1]);
}

// ---------------------------------------------------------------------------------------------- accumulators, split products, planes
__device__ __forceinline__ f32x16 tf_zero() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}
// the three products hi*lo + lo*hi + hi*hi of the (hi, lo) fp16 split
__device__ __forceinline__ f32x16 tf_mfma3(half8 ah, half8 al, half8 bh, half8 bl, f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, c, 0, 0, 0);
}
__device__ __forceinline__ float tf_absmax16(const f32x16& v) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(v[e]));
  return m;
}
// the 16 accumulator values of a lane as (hi, lo) halves at scale s: k-step s' of a product that contracts over the features takes
// elements 8 s' .. 8 s' + 7
__device__ __forceinline__ void tf_split16(const f32x16& v, float s, half8 (&h)[2], half8 (&l)[2]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const float t = v[e] * s;
    const _Float16 th = (_Float16)t;
    h[e >> 3][e & 7] = th;
    l[e >> 3][e & 7] = (_Float16)(t - (float)th);
  }
}
// ... also written as planes [token li < ROWS][32 features] (pitch TF_PS) for the transpose reads of the weight-gradient products
template <int ROWS>
__device__ __forceinline__ void tf_split16(const f32x16& v, float s, half8 (&h)[2], half8 (&l)[2], _Float16* __restrict__ Ph, _Float16* __restrict__ Pl,
                                           int li, int hh) {
  tf_split16(v, s, h, l);
  if (ROWS == 32 || li < ROWS) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      half4v a, b;
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] = h[c >> 1][4 * (c & 1) + j]; b[j] = l[c >> 1][4 * (c & 1) + j]; }
      *reinterpret_cast<half4v*>(Ph + li * TF_PS + 8 * c + 4 * hh) = a;
      *reinterpret_cast<half4v*>(Pl + li * TF_PS + 8 * c + 4 * hh) = b;
    }
  }
}
// four values of a row at scale s -> (hi, lo) planes of an LDS token tile (pitch TF_AST halves)
__device__ __forceinline__ void tf_plane_row(float4 v, float s, _Float16* __restrict__ Ah, _Float16* __restrict__ Al, int row, int c4) {
  const float o[4] = {v.x, v.y, v.z, v.w};
  half4v h, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float t = o[j] * s;
    h[j] = (_Float16)t;
    l[j] = (_Float16)(t - (float)h[j]);
  }
  *reinterpret_cast<half4v*>(Ah + row * TF_AST + 4 * c4) = h;
  *reinterpret_cast<half4v*>(Al + row * TF_AST + 4 * c4) = l;
}

// ---------------------------------------------------------------------------------------------- transpose reads, the swizzled W image
typedef short tf_short4 __attribute__((ext_vector_type(4)));
typedef short tf_short8 __attribute__((ext_vector_type(8)));
typedef tf_short4 __attribute__((address_space(3))) * tf_lds_s4;

__device__ __forceinline__ half8 tf_tr2(const _Float16* p0, const _Float16* p1) {
  const tf_short4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tf_lds_s4)(p0));
  const tf_short4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tf_lds_s4)(p1));
  const tf_short8 c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(half8, c);
}
// halves offset of the 16-byte chunk `chunk` of row f in a swizzled W plane
__device__ __forceinline__ int tf_woff(int f, int chunk) { return f * TF_C + ((chunk ^ ((f >> 1) & 7)) << 3); }
// W^T fragment for dxn^T[c][tok] = sum_f W[f][c] d[tok][f]: lane (li, hh) receives channel 32 ct + li of the rows f0 + 4 hh + (0..3) and
// f0 + 8 + 4 hh + (0..3) -- the features a lane half holds in accumulator registers 8 s .. 8 s + 7 when f0 = base + 16 s
__device__ __forceinline__ half8 tf_wtr(const _Float16* W, int f0, int ct, int lane) {
  const int g = lane >> 4, xl = lane & 15;
  const int ra = f0 + 4 * (g >> 1) + (xl >> 2), rb = ra + 8;
  const int col = 32 * ct + 16 * (g & 1) + 4 * (xl & 3);
  return tf_tr2(W + tf_woff(ra, col >> 3) + (col & 7), W + tf_woff(rb, col >> 3) + (col & 7));
}

// ---------------------------------------------------------------------------------------------- running plane scales (backward kernels)
// power-of-two plane scale for a tensor bounded by `bound`, kept inside [2^-100, 2^100]
__device__ __forceinline__ float tf_scale(float bound) { return fminf(fmaxf(scale_from_amax(bound), 0x1p-100f), 0x1p100f); }
// w *= r without a VALU instruction touching the accumulator (a value the VALU multiplies has to live in the architectural half of the
// register file for its whole life -- 128 such registers spill) and IN PLACE (a fresh result tile merged back at the end of a rare branch
// costs the allocator ~100 registers): sixteen accumulating steps of the exact-fp32 matrix instruction, step e adding (r - 1) * (the two
// rows accumulator register e holds) -- row operand (r - 1) * unit vector, column operand the accumulator register itself. One rounding
// per entry (r is a power of two, (r - 1) w is not exactly representable): 2^-24 relative, a handful of times per launch.
__device__ __forceinline__ void tf_rescale(f32x16& w, float r, int li, int hh) {
  const float r1 = r - 1.0f;
#pragma unroll
  for (int e = 0; e < 16; ++e) w = __builtin_amdgcn_mfma_f32_32x32x2f32(li == tf_key(e, hh) ? r1 : 0.f, w[e], w, 0, 0, 0);
}
// a gradient tile larger than every one before it: the tensor's two weight-gradient tiles move to the new scale (exact: a power of two)
__device__ __forceinline__ void tf_fit(float& sc, float amax, f32x16& w0, f32x16& w1, int li, int hh) {
  const float need = tf_scale(amax);
  if (need < sc) {
    const float r = need / sc;
    tf_rescale(w0, r, li, hh);
    tf_rescale(w1, r, li, hh);
    sc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(need)));
  }
}

// ---------------------------------------------------------------------------------------------- LayerNorm rows
// one row of 64 channels, 16 lanes x float4: LayerNorm (gain g) -> fp16 (hi, lo) planes of an LDS token tile (pitch TF_AST halves);
// mean and 1/std handed back (the backward kernels keep them)
__device__ __forceinline__ void tf_ln_row(float4 xv, float4 g, float eps, float ps, _Float16* __restrict__ Ah, _Float16* __restrict__ Al, int row, int c4,
                                          float& mean, float& rstd) {
  // layernorm.hip's layernorm_kernel (two-pass mean / variance over the 16 lanes of the row), the lane sums taken in DPP order
  mean = tf_row16_sum((xv.x + xv.y) + (xv.z + xv.w)) * (1.0f / TF_C);
  xv.x -= mean; xv.y -= mean; xv.z -= mean; xv.w -= mean;
  const float var = tf_row16_sum((xv.x * xv.x + xv.y * xv.y) + (xv.z * xv.z + xv.w * xv.w)) * (1.0f / TF_C);
  rstd = 1.0f / sqrtf(var + eps);
  const float o[4] = {xv.x * rstd * g.x, xv.y * rstd * g.y, xv.z * rstd * g.z, xv.w * rstd * g.w};
  half4v h, l;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float t = o[j] * ps;
    h[j] = (_Float16)t;
    l[j] = (_Float16)(t - (float)h[j]);
  }
  *reinterpret_cast<half4v*>(Ah + row * TF_AST + 4 * c4) = h;
  *reinterpret_cast<half4v*>(Al + row * TF_AST + 4 * c4) = l;
}
__device__ __forceinline__ void tf_ln_row(float4 xv, float4 g, float eps, float ps, _Float16* __restrict__ Ah, _Float16* __restrict__ Al, int row, int c4) {
  float mean, rstd;
  tf_ln_row(xv, g, eps, ps, Ah, Al, row, c4, mean, rstd);
}
// one row of C = 128 / 256 channels by its 16 lanes (gain re-read per row -- L1 hits -- rather than held across the matrix phases:
// registers) -> (hi, lo) planes of pitch C + 8 halves
template <int C>
__device__ __forceinline__ void tf_ln_row_wide(const float4 (&xin)[C / 64], const float* __restrict__ gamma, float eps, float ps, _Float16* __restrict__ Ah,
                                               _Float16* __restrict__ Al, int row, int lc4) {
  constexpr int NJ = C / 64, AST = C + 8;
  float4 xv[NJ];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) { xv[j] = xin[j]; s += (xv[j].x + xv[j].y) + (xv[j].z + xv[j].w); }
  const float mean = tf_row16_sum(s) * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    xv[j].x -= mean; xv[j].y -= mean; xv[j].z -= mean; xv[j].w -= mean;
    q += (xv[j].x * xv[j].x + xv[j].y * xv[j].y) + (xv[j].z * xv[j].z + xv[j].w * xv[j].w);
  }
  const float rstd = 1.0f / sqrtf(tf_row16_sum(q) * (1.0f / C) + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float4 g = reinterpret_cast<const float4*>(gamma)[16 * j + lc4];
    const float o[4] = {xv[j].x * rstd * g.x, xv[j].y * rstd * g.y, xv[j].z * rstd * g.z, xv[j].w * rstd * g.w};
    half4v hv, lv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = o[e] * ps;
      hv[e] = (_Float16)t;
      lv[e] = (_Float16)(t - (float)hv[e]);
    }
    *reinterpret_cast<half4v*>(Ah + row * AST + 64 * j + 4 * lc4) = hv;
    *reinterpret_cast<half4v*>(Al + row * AST + 64 * j + 4 * lc4) = lv;
  }
}
// scale of those planes: |LayerNorm(x)| <= sqrt(C) max|g|
template <int C>
__device__ __forceinline__ float tf_plane_scale_wide(const float* __restrict__ gamma, int lc4) {
  float gm = 0.f;
#pragma unroll
  for (int j = 0; j < C / 64; ++j) gm = amax4(gm, reinterpret_cast<const float4*>(gamma)[16 * j + lc4]);
  return scale_from_amax(sqrtf((float)C) * group_max<16>(gm));
}

// ---------------------------------------------------------------------------------------------- tables of the temporal kernels
// rotary table in LDS as (cos, sin) pairs: entry [token][pair i] -> (cos, sin) of features (2 i, 2 i + 1), row pitch TF_RST; rows
// NTOK .. ROWS - 1 (and every row when the block has no rotary embedding) = identity. Whole block of BLOCK threads.
template <int ROWS, int NTOK, int BLOCK>
__device__ __forceinline__ void tf_rotary_table(float2* __restrict__ Rt, const float* __restrict__ rcos, const float* __restrict__ rsin, int tid) {
  for (int i = tid; i < ROWS * 16; i += BLOCK) {
    const int t = i >> 4, j = i & 15;
    float2 v = make_float2(1.f, 0.f);
    if (rcos && t < NTOK) v = make_float2(rcos[t * 32 + 2 * j], rsin[t * 32 + 2 * j]);
    Rt[t * TF_RST + j] = v;
  }
}
// relative-position bias [head][query row < ROWS][PITCH] from [head][NTOK][NTOK] (zeros where absent / beyond the NTOK tokens)
template <int ROWS, int NTOK, int PITCH, int BLOCK>
__device__ __forceinline__ void tf_bias_table(float* __restrict__ Bs, const float* __restrict__ bias, int tid) {
  for (int i = tid; i < TF_HEADS * ROWS * PITCH; i += BLOCK) {
    const int hd = i / (ROWS * PITCH), r = i - hd * (ROWS * PITCH), q = r / PITCH, k = r - q * PITCH;
    Bs[i] = (bias && (ROWS == NTOK || q < NTOK) && k < NTOK) ? bias[(hd * NTOK + q) * NTOK + k] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------- steps of the temporal forward pass
// (q | k | v)^T of a head, [feature][token], from the head's resident weight fragments (A) and the token planes (B, this lane's token = plane
// row `row`), scaled back to fp32 units
__device__ __forceinline__ void tf_qkv_project(const half8 (&wqh)[3][4], const half8 (&wql)[3][4], const _Float16* __restrict__ Ah,
                                               const _Float16* __restrict__ Al, int row, int hh, float inv_qkv, f32x16& aq, f32x16& ak, f32x16& av) {
#pragma unroll
  for (int e = 0; e < 16; ++e) { aq[e] = 0.f; ak[e] = 0.f; av[e] = 0.f; }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const half8 ah = *reinterpret_cast<const half8*>(Ah + row * TF_AST + 16 * s + 8 * hh);
    const half8 al = *reinterpret_cast<const half8*>(Al + row * TF_AST + 16 * s + 8 * hh);
    aq = __builtin_amdgcn_mfma_f32_32x32x16_f16(wqh[0][s], al, aq, 0, 0, 0);
    ak = __builtin_amdgcn_mfma_f32_32x32x16_f16(wqh[1][s], al, ak, 0, 0, 0);
    av = __builtin_amdgcn_mfma_f32_32x32x16_f16(wqh[2][s], al, av, 0, 0, 0);
    aq = __builtin_amdgcn_mfma_f32_32x32x16_f16(wql[0][s], ah, aq, 0, 0, 0);
    ak = __builtin_amdgcn_mfma_f32_32x32x16_f16(wql[1][s], ah, ak, 0, 0, 0);
    av = __builtin_amdgcn_mfma_f32_32x32x16_f16(wql[2][s], ah, av, 0, 0, 0);
    aq = __builtin_amdgcn_mfma_f32_32x32x16_f16(wqh[0][s], ah, aq, 0, 0, 0);
    ak = __builtin_amdgcn_mfma_f32_32x32x16_f16(wqh[1][s], ah, ak, 0, 0, 0);
    av = __builtin_amdgcn_mfma_f32_32x32x16_f16(wqh[2][s], ah, av, 0, 0, 0);
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) { aq[e] *= inv_qkv; ak[e] *= inv_qkv; av[e] *= inv_qkv; }
}
// q * scale, rotary on q and k (pairs (2i, 2i + 1) = accumulator registers (2 j, 2 j + 1)); `row` = this lane's token in the table
__device__ __forceinline__ void tf_rotary_qk(f32x16& aq, f32x16& ak, const float2* __restrict__ Rt, int row, int hh, float scale) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    // features 8 c + 4 hh + (0..3) = pairs 4 c + 2 hh, 4 c + 2 hh + 1
    const float4 r4 = *reinterpret_cast<const float4*>(Rt + row * TF_RST + 4 * c + 2 * hh);
    const float cs2[2] = {r4.x, r4.z}, sn2[2] = {r4.y, r4.w};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = 2 * c + q;
      const float qx = aq[2 * j] * scale, qy = aq[2 * j + 1] * scale;
      aq[2 * j] = qx * cs2[q] - qy * sn2[q];
      aq[2 * j + 1] = qy * cs2[q] + qx * sn2[q];
      const float kx = ak[2 * j], ky = ak[2 * j + 1];
      ak[2 * j] = kx * cs2[q] - ky * sn2[q];
      ak[2 * j + 1] = ky * cs2[q] + kx * sn2[q];
    }
  }
}
// softmax over the 24 keys of this lane's query inside the lane pair, S^T in accumulator layout; Bh = the head's bias table (pitch
// TF_BST), `row` = the query's row in it
__device__ __forceinline__ void tf_softmax24(f32x16& sT, const float* __restrict__ Bh, int row, int hh) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                     // keys 8 c + 4 hh + (0..3) < 24
    const float4 b4 = *reinterpret_cast<const float4*>(Bh + row * TF_BST + 8 * c + 4 * hh);
    sT[4 * c] += b4.x; sT[4 * c + 1] += b4.y; sT[4 * c + 2] += b4.z; sT[4 * c + 3] += b4.w;
    mx = fmaxf(fmaxf(mx, fmaxf(sT[4 * c], sT[4 * c + 1])), fmaxf(sT[4 * c + 2], sT[4 * c + 3]));
  }
  float m0, m1;
  tf_halves(mx, m0, m1);
  mx = fmaxf(m0, m1);
  float l = 0.f;
#pragma unroll
  for (int e = 0; e < 12; ++e) { sT[e] = expf(sT[e] - mx); l += sT[e]; }
#pragma unroll
  for (int e = 12; e < 16; ++e) sT[e] = 0.f;            // keys 24 .. 31 do not exist
  float l0, l1;
  tf_halves(l, l0, l1);
  const float il = 1.0f / (l0 + l1);
#pragma unroll
  for (int e = 0; e < 12; ++e) sT[e] *= il;
}
// to_out fragments of W_out for output channel 32 ct + li and k-step s of head h: reduction slot t <-> feature
// d = 16 s + 8 (t >> 2) + 4 hh + (t & 3) of the head (the order in which accumulator registers 8 s .. 8 s + 7 of O^T hold them)
__device__ __forceinline__ void tf_wout_frag(const _Float16* __restrict__ wo_hi, const _Float16* __restrict__ wo_lo, int ct, int h, int s, int li, int hh,
                                             half8& woh, half8& wol) {
  const int off = (32 * ct + li) * TF_HD + 32 * h + 16 * s + 4 * hh;
  const half4v a = *reinterpret_cast<const half4v*>(wo_hi + off), b = *reinterpret_cast<const half4v*>(wo_hi + off + 8);
  const half4v c = *reinterpret_cast<const half4v*>(wo_lo + off), d = *reinterpret_cast<const half4v*>(wo_lo + off + 8);
  woh = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  wol = __builtin_shufflevector(c, d, 0, 1, 2, 3, 4, 5, 6, 7);
}
// one k-step of the head's to_out product (32 of the 128 reduction values): y_part[c][token], channels 0..31 (y0) and 32..63 (y1)
__device__ __forceinline__ void tf_to_out_step(half8 woh0, half8 woh1, half8 wol0, half8 wol1, half8 oh, half8 ol, f32x16& y0, f32x16& y1) {
  y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(woh0, ol, y0, 0, 0, 0);
  y1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(woh1, ol, y1, 0, 0, 0);
  y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wol0, oh, y0, 0, 0, 0);
  y1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wol1, oh, y1, 0, 0, 0);
  y0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(woh0, oh, y0, 0, 0, 0);
  y1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(woh1, oh, y1, 0, 0, 0);
}
// the head's partial output of a token: yp = its row of the head's [token][TF_YST] tile + 4 hh
__device__ __forceinline__ void tf_partial_store(float* __restrict__ yp, const f32x16& y0, const f32x16& y1, float inv_o) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    *reinterpret_cast<float4*>(yp + 8 * c) = make_float4(y0[4 * c] * inv_o, y0[4 * c + 1] * inv_o, y0[4 * c + 2] * inv_o, y0[4 * c + 3] * inv_o);
    *reinterpret_cast<float4*>(yp + 32 + 8 * c) = make_float4(y1[4 * c] * inv_o, y1[4 * c + 1] * inv_o, y1[4 * c + 2] * inv_o, y1[4 * c + 3] * inv_o);
  }
}
// heads summed, residual added, one row stored: Yp = the four heads' partial tiles (hstride floats apart), x = the residual values
__device__ __forceinline__ void tf_head_sum_store(const float* __restrict__ Yp, int hstride, int row, int lc4, const float4& x, float* __restrict__ yb,
                                                  int64_t fstride, float& am) {
  const int o = row * TF_YST + 4 * lc4;
  const float4 a = *reinterpret_cast<const float4*>(Yp + o), b2 = *reinterpret_cast<const float4*>(Yp + hstride + o);
  const float4 c = *reinterpret_cast<const float4*>(Yp + 2 * hstride + o), d = *reinterpret_cast<const float4*>(Yp + 3 * hstride + o);
  float4 r;
  r.x = ((a.x + b2.x) + (c.x + d.x)) + x.x; r.y = ((a.y + b2.y) + (c.y + d.y)) + x.y;
  r.z = ((a.z + b2.z) + (c.z + d.z)) + x.z; r.w = ((a.w + b2.w) + (c.w + d.w)) + x.w;
  *reinterpret_cast<float4*>(yb + row * fstride + 4 * lc4) = r;
  am = amax4(am, r);
}

// ---------------------------------------------------------------------------------------------- linear attention
// qs = scale softmax over the head's 32 features of the token (16 in this lane, 16 in lane ^ 32), in place
__device__ __forceinline__ void tf_softmax_d(f32x16& aq, float scale) {
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) mx = fmaxf(mx, aq[e]);
  float m0, m1;
  tf_halves(mx, m0, m1);
  mx = fmaxf(m0, m1);
  float l = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) { aq[e] = expf(aq[e] - mx); l += aq[e]; }
  float l0, l1;
  tf_halves(l, l0, l1);
  const float il = scale / (l0 + l1);
#pragma unroll
  for (int e = 0; e < 16; ++e) aq[e] *= il;
}

// launch parameters of the forward kernels (attn_fused.hip: 24 frames; attn_fused48.hip: 48)
struct TFusedP {
  const float* x; const float* gamma; float eps;
  const _Float16* wq_hi; const _Float16* wq_lo; const float* wq_scale;      // packed forward operand of to_qkv: [384][64]
  const _Float16* wo_hi; const _Float16* wo_lo; const float* wo_scale;      // ... of to_out: [64][128]
  const float* rcos; const float* rsin; const float* bias;                  // [24][32], [24][32], [4][24][24] (any may be null)
  float* y; float* amax_rec;
  float* qkv_out;                                                           // optional: raw projections [rows][384] (the un-fused backward reads them)
  float* rec_v;                                                             // optional amax record of v (attn_fused_bwd.hip: the plane scale of the attention output)
  int HW; float scale; int64_t nseq;
};

// blocks per CU of the four temporal kernels' persistent grids, and the grid itself (at most one block per sequence): what the launchers
// launch and what wdno_tattn_fused_plan (attn_fused.hip) answers
#define TF_BPC_FWD 2       /* attn_fused.hip */
#define TF_BPC_FWD48 1     /* attn_fused48.hip */
#define TF_BPC_WIDE 2      /* attn_fused_wide.hip */
#define TF_BPC_BWD 1       /* attn_fused_bwd.hip */
static inline int64_t tf_grid(int blocks_per_cu, int64_t nseq) {
  const int64_t grid = blocks_per_cu * (int64_t)wdno_num_cus();
  return grid > nseq ? nseq : grid;
}
