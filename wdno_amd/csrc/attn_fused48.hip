// attn_fused48.hip -- the fused temporal attention block (attn_fused.hip: LayerNorm -> to_qkv -> rotary / attention over frames -> to_out +
// residual of Residual(PreNorm(EinopsToAndFrom(Attention))), conv3d.py:165-174, :277-353) for sequences of 48 frames: the super-resolution
// U-Net of the smoke tree works on 48 wavelet frames (inference_2d.py, BASELINE configs[4]), where the 24-frame kernel does not apply and a
// level-0 site costs LayerNorm + a 64 -> 384 projection (944 MB of qkv at [2,48,80,80]) + attention + to_out + two split passes.
// Forward only (sampling); a training step of that model runs the block layer by layer.
//
// One block = EIGHT waves = (head h, token tile tt) for ONE sequence at a time: tokens 0..31 and 32..47 (+ 16 rows of padding) are two MFMA
// row tiles. Per sequence:
//   * LayerNorm by the whole block into the fp16 (hi, lo) token planes [64][72] (rows 48..63 zero), as attn_fused.hip.
//   * wave (h, tt): (q | k | v)^T of its head and token tile on the split MFMA, accumulators [feature][token]; scale and rotary in place.
//   * k (rotated) and v go to LDS tiles [token][feature] of the head; after one block barrier every wave reads the OTHER token tile's k in
//     accumulator layout, so both score products S^T[kt] = K[kt] Q^T run on v_mfma_f32_32x32x2_f32 with operands in place; softmax over
//     the 48 keys of the lane's query is lane-pair-local (two accumulator tiles); O^T = sum_kt V[kt]^T P[kt]^T reads V transposed.
//   * to_out as attn_fused.hip; the partial [token][64] tiles of the four heads go through LDS (aliased onto the k / v tiles, which are
//     dead by then), summed with the residual x by the threads that loaded the rows.
// LDS 141 KB (planes 18, k + v tiles 74, rotary 9, bias 40): one block per CU, eight waves -- the occupancy of the 24-frame kernel.
// Steps shared with the 24-frame kernel are the tf_ functions of attn_fused.h; t48_ / T48_ names are what only this file has: the two token
// tiles per head, the exchange of k through LDS, the softmax over 48 keys, W_out fetched per sequence.
#include "attn_fused.h"

#define T48_NT 48
#define T48_BST 52     /* floats per query row of the bias table (48 keys + pad: 13 sixteen-byte slots, coprime with the 8 slot classes) */
#define T48_A_BYTES (64 * TF_AST * 2)
#define T48_KV_BYTES (TF_HEADS * 64 * TF_VST * 4)
#define T48_RT_BYTES (64 * TF_RST * 8)
#define T48_BS_BYTES (TF_HEADS * T48_NT * T48_BST * 4)
#define T48_LDS_BYTES (2 * T48_A_BYTES + 2 * T48_KV_BYTES + T48_RT_BYTES + T48_BS_BYTES + 64)
static_assert(TF_HEADS * T48_NT * TF_YST * 4 <= 2 * T48_KV_BYTES, "the partial output tiles alias the k / v tiles");

__global__ __launch_bounds__(512, 1) void tattn_fused_fwd48_kernel(TFusedP p) {
  extern __shared__ __attribute__((aligned(16))) char smem48[];
  _Float16* Ah = reinterpret_cast<_Float16*>(smem48);
  _Float16* Al = reinterpret_cast<_Float16*>(smem48 + T48_A_BYTES);
  float* Kt = reinterpret_cast<float*>(smem48 + 2 * T48_A_BYTES);                  // [head][64 tokens][TF_VST]
  float* Vt = reinterpret_cast<float*>(smem48 + 2 * T48_A_BYTES + T48_KV_BYTES);
  float* Yp = Kt;                                                                  // [head][48 tokens][TF_YST], once k / v are dead
  float2* Rt = reinterpret_cast<float2*>(smem48 + 2 * T48_A_BYTES + 2 * T48_KV_BYTES);
  float* Bs = reinterpret_cast<float*>(smem48 + 2 * T48_A_BYTES + 2 * T48_KV_BYTES + T48_RT_BYTES);      // [head][48 queries][T48_BST]
  float* Av = reinterpret_cast<float*>(smem48 + 2 * T48_A_BYTES + 2 * T48_KV_BYTES + T48_RT_BYTES + T48_BS_BYTES);      // max|v| per (head, tile)
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = wave & 3, tt = wave >> 2;
  const int lane = tid & 63, li = lane & 31, hh = lane >> 5;
  const int trow = 32 * tt + li;                          // this lane's token
  const bool tok = trow < T48_NT;
  const int lrow = tid >> 4, lc4 = tid & 15;              // loader role: rows lrow (0..31) and 32 + lrow (lrow < 16)

  // ---- per-kernel operands
  half8 wqh[3][4], wql[3][4];
#pragma unroll
  for (int ti = 0; ti < 3; ++ti)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int off = (ti * TF_HD + h * 32 + li) * TF_C + 16 * s + 8 * hh;
      wqh[ti][s] = *reinterpret_cast<const half8*>(p.wq_hi + off);
      wql[ti][s] = *reinterpret_cast<const half8*>(p.wq_lo + off);
    }
  tf_rotary_table<64, T48_NT, 512>(Rt, p.rcos, p.rsin, tid);
  tf_bias_table<T48_NT, T48_NT, T48_BST, 512>(Bs, p.bias, tid);
  const float4 g4 = reinterpret_cast<const float4*>(p.gamma)[lc4];
  const float ps = scale_from_amax(8.0f * group_max<16>(amax4(0.f, g4)));        // |LayerNorm(x)| <= sqrt(64) max|g|
  const float inv_qkv = 1.0f / (ps * p.wq_scale[0]);
  const float sw_o = p.wo_scale[0];
  const int64_t fstride = (int64_t)p.HW * TF_C;
  const int qrow = trow < T48_NT ? trow : T48_NT - 1;     // bias row of this lane's query (lanes beyond the sequence read a real row; unused)
  float am = 0.f, stv = 0.f;

  float4 nx0 = make_float4(0.f, 0.f, 0.f, 0.f), nx1 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto fetch = [&](int64_t r0) {
    const float* xr = p.x + r0 * TF_C;
    nx0 = *reinterpret_cast<const float4*>(xr + lrow * fstride + 4 * lc4);
    if (lrow < 16) nx1 = *reinterpret_cast<const float4*>(xr + (32 + lrow) * fstride + 4 * lc4);
  };
  int nb = (int)(blockIdx.x / (unsigned)p.HW), npix = (int)(blockIdx.x - (unsigned)nb * (unsigned)p.HW);
  const int gstep_b = (int)(gridDim.x / (unsigned)p.HW), gstep_p = (int)(gridDim.x - (unsigned)gstep_b * (unsigned)p.HW);
  if ((int64_t)blockIdx.x < p.nseq) fetch((int64_t)nb * T48_NT * p.HW + npix);
  for (int64_t seq = blockIdx.x; seq < p.nseq; seq += gridDim.x) {
    const int64_t row0 = (int64_t)nb * T48_NT * p.HW + npix;
    const float* xb = p.x + row0 * TF_C;
    nb += gstep_b; npix += gstep_p;
    if (npix >= p.HW) { npix -= p.HW; ++nb; }
    // ---- rows -> LayerNorm -> planes (rows 48..63: zeros in, zeros out)
    tf_ln_row(nx0, g4, p.eps, ps, Ah, Al, lrow, lc4);
    tf_ln_row(nx1, g4, p.eps, ps, Ah, Al, 32 + lrow, lc4);
    __syncthreads();                                                            // (1) planes; also: the previous sequence's partial tiles are read
    if (seq + gridDim.x < p.nseq) fetch((int64_t)nb * T48_NT * p.HW + npix);
    // ---- (q | k | v)^T of this head and token tile: [feature][token]
    f32x16 aq, ak, av;
    tf_qkv_project(wqh, wql, Ah, Al, trow, hh, inv_qkv, aq, ak, av);
    tf_rotary_qk(aq, ak, Rt, trow, hh, p.scale);
    // k and v tiles of the head: [token][feature]; max|v| bounds |out| (rows of P sum to 1)
    float amv = 0.f;
    {
      float* kt = Kt + (h * 64 + trow) * TF_VST + 4 * hh;
      float* vt = Vt + (h * 64 + trow) * TF_VST + 4 * hh;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 v4 = make_float4(av[4 * c], av[4 * c + 1], av[4 * c + 2], av[4 * c + 3]);
        amv = amax4(amv, v4);
        *reinterpret_cast<float4*>(vt + 8 * c) = v4;
        *reinterpret_cast<float4*>(kt + 8 * c) = make_float4(ak[4 * c], ak[4 * c + 1], ak[4 * c + 2], ak[4 * c + 3]);
      }
    }
    stv = fmaxf(stv, amv);
    amv = tf_wave_max(amv);
    if (lane == 0) Av[h * 2 + tt] = amv;
    __syncthreads();                                                            // (2) k / v tiles, max|v|
    amv = fmaxf(Av[h * 2], Av[h * 2 + 1]);
    // ---- S^T[kt] = K[kt] Q^T (exact fp32); the other token tile's k in accumulator layout from its LDS tile
    f32x16 ako;
    {
      const float* ko = Kt + (h * 64 + 32 * (1 - tt) + li) * TF_VST + 4 * hh;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 k4 = *reinterpret_cast<const float4*>(ko + 8 * c);
        ako[4 * c] = k4.x; ako[4 * c + 1] = k4.y; ako[4 * c + 2] = k4.z; ako[4 * c + 3] = k4.w;
      }
    }
    f32x16 s0 = tf_zero(), s1 = tf_zero();                // keys 0..31, keys 32..63
    if (tt == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[e], aq[e], s0, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 16; ++e) s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ako[e], aq[e], s1, 0, 0, 0);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ako[e], aq[e], s0, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 16; ++e) s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[e], aq[e], s1, 0, 0, 0);
    }
    {
      // softmax over the 48 keys of this lane's query: keys 8 c + 4 hh + (0..3) of tile 0 (c < 4) and 32 + the same of tile 1 (c < 2)
      const float* bq = Bs + (h * T48_NT + qrow) * T48_BST + 4 * hh;
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 b4 = *reinterpret_cast<const float4*>(bq + 8 * c);
        s0[4 * c] += b4.x; s0[4 * c + 1] += b4.y; s0[4 * c + 2] += b4.z; s0[4 * c + 3] += b4.w;
        mx = fmaxf(fmaxf(mx, fmaxf(s0[4 * c], s0[4 * c + 1])), fmaxf(s0[4 * c + 2], s0[4 * c + 3]));
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float4 b4 = *reinterpret_cast<const float4*>(bq + 32 + 8 * c);
        s1[4 * c] += b4.x; s1[4 * c + 1] += b4.y; s1[4 * c + 2] += b4.z; s1[4 * c + 3] += b4.w;
        mx = fmaxf(fmaxf(mx, fmaxf(s1[4 * c], s1[4 * c + 1])), fmaxf(s1[4 * c + 2], s1[4 * c + 3]));
      }
      float m0, m1;
      tf_halves(mx, m0, m1);
      mx = fmaxf(m0, m1);
      float l = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s0[e] = expf(s0[e] - mx); l += s0[e]; }
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[e] = expf(s1[e] - mx); l += s1[e]; }
      float l0, l1;
      tf_halves(l, l0, l1);
      const float il = 1.0f / (l0 + l1);
#pragma unroll
      for (int e = 0; e < 16; ++e) s0[e] *= il;
#pragma unroll
      for (int e = 0; e < 8; ++e) s1[e] *= il;
    }
    // ---- O^T = V[0]^T P[0]^T + V[1]^T P[1]^T (keys 48..63 do not exist: eight steps of the second tile)
    f32x16 oT = tf_zero();
    {
      const float* v0 = Vt + h * 64 * TF_VST + li;
#pragma unroll
      for (int m = 0; m < 16; ++m) oT = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[tf_key(m, hh) * TF_VST], s0[m], oT, 0, 0, 0);
#pragma unroll
      for (int m = 0; m < 8; ++m) oT = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[(32 + tf_key(m, hh)) * TF_VST], s1[m], oT, 0, 0, 0);
    }
    // the residual rows again (L2 hits)
    const float4 x0 = *reinterpret_cast<const float4*>(xb + lrow * fstride + 4 * lc4);
    float4 x1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lrow < 16) x1 = *reinterpret_cast<const float4*>(xb + (32 + lrow) * fstride + 4 * lc4);
    // ---- to_out, this head's 32 of the 128 reduction values (the fragments of W_out are fetched per sequence: L1 / L2 hits; held across
    // the products they would not leave room for the second score tile)
    const float so = scale_from_amax(amv);
    half8 oh[2], ol[2];
    tf_split16(oT, so, oh, ol);
    f32x16 y0 = tf_zero(), y1 = tf_zero();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      half8 woh[2], wol[2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) tf_wout_frag(p.wo_hi, p.wo_lo, ct, h, s, li, hh, woh[ct], wol[ct]);
      tf_to_out_step(woh[0], woh[1], wol[0], wol[1], oh[s], ol[s], y0, y1);
    }
    const float inv_o = 1.0f / (so * sw_o);
    __syncthreads();                                                            // (3) every wave is done with the k / v tiles
    if (tok) tf_partial_store(Yp + (h * T48_NT + trow) * TF_YST + 4 * hh, y0, y1, inv_o);
    __syncthreads();                                                            // (4) partial tiles
    // ---- heads summed, residual added, rows stored (the threads that loaded a row finish it)
    float* yb = p.y + row0 * TF_C;
    tf_head_sum_store(Yp, T48_NT * TF_YST, lrow, lc4, x0, yb, fstride, am);
    if (lrow < 16) tf_head_sum_store(Yp, T48_NT * TF_YST, 32 + lrow, lc4, x1, yb, fstride, am);
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * 8 + wave);
  if (p.rec_v) wave_amax_emit(stv, p.rec_v, (int)blockIdx.x * 8 + wave);
}

// called by wdno_tattn_fused_fwd (attn_fused.hip) for n_tok == 48
int wdno_tattn_fused_fwd48_launch(const TFusedP& p, hipStream_t st) {
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)tattn_fused_fwd48_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, T48_LDS_BYTES) != hipSuccess) return WDNO_ELAUNCH;
    attr_done = true;
  }
  const int64_t grid = tf_grid(TF_BPC_FWD48, p.nseq);
  tattn_fused_fwd48_kernel<<<(int)grid, 512, T48_LDS_BYTES, st>>>(p);
  return wdno_check_launch();
}
