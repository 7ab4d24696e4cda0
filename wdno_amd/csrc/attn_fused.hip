// attn_fused.hip -- the temporal attention block of the smoke U-Net (conv3d.py:165-174 LayerNorm, :277-353 Attention, wrapped as
// Residual(PreNorm(dim, EinopsToAndFrom('b c f h w', 'b (h w) f c', Attention)))) as ONE kernel at the network's first level:
//
//     y = x + W_out . softmax(rot(scale q) rot(k)^T + bias) v ,      (q | k | v) = W_qkv . LayerNorm(x)
//
// for C = 64 channels, 24 frames, 4 heads of 32. Un-fused, the block moves the [pixels x 384] qkv tensor (472 MB at the bench size)
// HBM -> HBM twice in the forward pass alone, plus the LayerNorm planes and the attention output planes; fused, a sequence (the 24
// frames of one pixel: 24 rows of 256 B, 409 600 B apart) is read once and written once.
//
// One block = four waves = the four heads of ONE sequence at a time; blocks walk sequences with a grid stride, two blocks per CU.
//   * LayerNorm by the whole block (16 lanes per row), result split into fp16 (hi, lo) planes in LDS [32 tokens][64] (rows 24..31 zero;
//     row pitch 144 B = conflict-free ds_read_b128 fragments). Plane scale from the bound |LN| <= sqrt(C) max|g| (as layernorm.hip does).
//   * Projection on v_mfma_f32_32x32x16_f16 with the three products hi*lo + lo*hi + hi*hi (the fp32-equivalent arithmetic of the
//     convolutions, conv_h3t.hip): A = the head's 96 rows of the packed W_qkv planes, held in registers for the whole kernel
//     (24 fragments), B = the token planes. Accumulators come out as [feature][token]: a lane owns one token and the features
//     8 c + 4 hh + (0..3).
//   * That layout IS the operand layout of the exact-fp32 score product (attention.hip: S^T = K Q^T on v_mfma_f32_32x32x2_f32, step e
//     contracts the features the two lane halves hold in accumulator register e), so q and k never move; rotary pairs (2i, 2i+1) are
//     lane-local. Softmax over the keys inside a lane pair; P^T feeds the second product in place; V goes through a 32 x 32 LDS tile
//     to be read transposed.
//   * to_out: the head's slice of the reduction (32 of 128) on the split MFMA again -- the accumulator registers of O^T are the
//     B fragments once W_out's fragments are gathered in the matching feature order -- partial [64][token] tiles of the four heads
//     summed through LDS together with the residual x (kept in registers by the lanes that loaded it), one coalesced store per row.
// The steps (tf_ names) are written once in attn_fused.h and shared with the 48-frame, wide and backward kernels; here: the order of the
// steps for 24 frames, the resident W_out fragments, the optional qkv_out / rec_v outputs, and the entry point that routes to the siblings.
#include "attn_fused.h"


__global__ __launch_bounds__(256, 2) void tattn_fused_fwd_kernel(TFusedP p) {
  __shared__ __attribute__((aligned(16))) _Float16 Ah[32 * TF_AST];
  __shared__ __attribute__((aligned(16))) _Float16 Al[32 * TF_AST];
  __shared__ __attribute__((aligned(16))) float Vt[TF_HEADS][32 * TF_VST];
  __shared__ __attribute__((aligned(16))) float Yp[TF_HEADS][TF_NT * TF_YST];
  __shared__ __attribute__((aligned(16))) float2 Rt[32 * TF_RST];
  __shared__ __attribute__((aligned(16))) float Bs[TF_HEADS][32 * TF_BST];
  const int tid = threadIdx.x;
  const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, li = lane & 31, hh = lane >> 5;
  const bool tok = li < TF_NT;
  const int lrow = tid >> 4, lc4 = tid & 15;

  // ---- per-kernel operands: the head's weight fragments, the lane's rotary entries, the LayerNorm gain
  half8 wqh[3][4], wql[3][4];
#pragma unroll
  for (int ti = 0; ti < 3; ++ti)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int off = (ti * TF_HD + h * 32 + li) * TF_C + 16 * s + 8 * hh;
      wqh[ti][s] = *reinterpret_cast<const half8*>(p.wq_hi + off);
      wql[ti][s] = *reinterpret_cast<const half8*>(p.wq_lo + off);
    }
  // to_out: output channel 32 ct + li; reduction slot t of k-step s <-> feature d = 16 s + 8 (t >> 2) + 4 hh + (t & 3) of the head (the
  // order in which accumulator registers 8 s .. 8 s + 7 of O^T hold them)
  half8 woh[2][2], wol[2][2];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int s = 0; s < 2; ++s) tf_wout_frag(p.wo_hi, p.wo_lo, ct, h, s, li, hh, woh[ct][s], wol[ct][s]);
  // rotary (cos, sin) pairs (rows 24..31 = identity) and relative-position bias [head][query][key] in LDS
  tf_rotary_table<32, TF_NT, 256>(Rt, p.rcos, p.rsin, tid);
  tf_bias_table<32, TF_NT, TF_BST, 256>(&Bs[0][0], p.bias, tid);
  const float4 g4 = reinterpret_cast<const float4*>(p.gamma)[lc4];
  const float ps = scale_from_amax(8.0f * group_max<16>(amax4(0.f, g4)));        // |LayerNorm(x)| <= sqrt(64) max|g|
  const float inv_qkv = 1.0f / (ps * p.wq_scale[0]);
  const float sw_o = p.wo_scale[0];
  const int64_t fstride = (int64_t)p.HW * TF_C;
  float am = 0.f, stv = 0.f;

  // rows of the first sequence; afterwards the rows of sequence n + 1 are requested while sequence n is in the matrix pipes
  float4 nx0 = make_float4(0.f, 0.f, 0.f, 0.f), nx1 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto fetch = [&](int64_t r0) {
    const float* xr = p.x + r0 * TF_C;
    nx0 = *reinterpret_cast<const float4*>(xr + lrow * fstride + 4 * lc4);
    if (lrow < 8) nx1 = *reinterpret_cast<const float4*>(xr + (16 + lrow) * fstride + 4 * lc4);
  };
  // sequence -> (sample b, pixel): advanced incrementally (a 64-bit division per sequence is ~200 instructions of every wave)
  int nb = (int)(blockIdx.x / (unsigned)p.HW), npix = (int)(blockIdx.x - (unsigned)nb * (unsigned)p.HW);
  const int gstep_b = (int)(gridDim.x / (unsigned)p.HW), gstep_p = (int)(gridDim.x - (unsigned)gstep_b * (unsigned)p.HW);
  if ((int64_t)blockIdx.x < p.nseq) fetch((int64_t)nb * TF_NT * p.HW + npix);
  for (int64_t seq = blockIdx.x; seq < p.nseq; seq += gridDim.x) {
    const int64_t row0 = (int64_t)nb * TF_NT * p.HW + npix;      // row of frame 0; frame f at + f * HW
    const float* xb = p.x + row0 * TF_C;
    nb += gstep_b; npix += gstep_p;
    if (npix >= p.HW) { npix -= p.HW; ++nb; }
    // ---- rows -> LayerNorm -> planes (rows 24..31: zeros in, zeros out)
    tf_ln_row(nx0, g4, p.eps, ps, Ah, Al, lrow, lc4);
    tf_ln_row(nx1, g4, p.eps, ps, Ah, Al, 16 + lrow, lc4);
    __syncthreads();
    if (seq + gridDim.x < p.nseq) fetch((int64_t)nb * TF_NT * p.HW + npix);
    // ---- (q | k | v)^T of this head: [feature][token]
    f32x16 aq, ak, av;
    tf_qkv_project(wqh, wql, Ah, Al, li, hh, inv_qkv, aq, ak, av);
    if (p.qkv_out && tok) {
      float* qr = p.qkv_out + (row0 + (int64_t)li * p.HW) * (3 * TF_HD) + h * 32 + 4 * hh;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        *reinterpret_cast<float4*>(qr + 8 * c) = make_float4(aq[4 * c], aq[4 * c + 1], aq[4 * c + 2], aq[4 * c + 3]);
        *reinterpret_cast<float4*>(qr + TF_HD + 8 * c) = make_float4(ak[4 * c], ak[4 * c + 1], ak[4 * c + 2], ak[4 * c + 3]);
        *reinterpret_cast<float4*>(qr + 2 * TF_HD + 8 * c) = make_float4(av[4 * c], av[4 * c + 1], av[4 * c + 2], av[4 * c + 3]);
      }
    }
    // V tile for the transposed read; max|v| bounds |out| (rows of P sum to 1)
    float amv = 0.f;
    float* vt = Vt[h];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 v4 = make_float4(av[4 * c], av[4 * c + 1], av[4 * c + 2], av[4 * c + 3]);
      amv = amax4(amv, v4);
      *reinterpret_cast<float4*>(vt + li * TF_VST + 8 * c + 4 * hh) = v4;
    }
    stv = fmaxf(stv, amv);
    amv = tf_wave_max(amv);
    tf_rotary_qk(aq, ak, Rt, li, hh, p.scale);
    // ---- S^T = K Q^T (exact fp32), softmax over the keys of this lane's query
    f32x16 sT = tf_zero();
#pragma unroll
    for (int e = 0; e < 16; ++e) sT = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[e], aq[e], sT, 0, 0, 0);
    tf_softmax24(sT, Bs[h], li, hh);
    // ---- O^T = V^T P^T
    __builtin_amdgcn_wave_barrier();
    float va[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) va[m] = vt[tf_key(m, hh) * TF_VST + li];
    f32x16 oT = tf_zero();
#pragma unroll
    for (int m = 0; m < 16; ++m) oT = __builtin_amdgcn_mfma_f32_32x32x2f32(va[m], sT[m], oT, 0, 0, 0);
    // the residual rows again (L2 hits; not held in registers across the products: the weight fragments own the register file)
    const float4 x0 = *reinterpret_cast<const float4*>(xb + lrow * fstride + 4 * lc4);
    float4 x1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lrow < 8) x1 = *reinterpret_cast<const float4*>(xb + (16 + lrow) * fstride + 4 * lc4);
    // ---- to_out, this head's 32 of the 128 reduction values: y_part[c][token]
    const float so = scale_from_amax(amv);
    half8 oh[2], ol[2];
    tf_split16(oT, so, oh, ol);
    f32x16 y0 = tf_zero(), y1 = tf_zero();
#pragma unroll
    for (int s = 0; s < 2; ++s) tf_to_out_step(woh[0][s], woh[1][s], wol[0][s], wol[1][s], oh[s], ol[s], y0, y1);
    const float inv_o = 1.0f / (so * sw_o);
    if (tok) tf_partial_store(Yp[h] + li * TF_YST + 4 * hh, y0, y1, inv_o);
    __syncthreads();
    // ---- heads summed, residual added, rows stored (the lanes that loaded a row finish it)
    float* yb = p.y + row0 * TF_C;
    tf_head_sum_store(Yp[0], TF_NT * TF_YST, lrow, lc4, x0, yb, fstride, am);
    if (lrow < 8) tf_head_sum_store(Yp[0], TF_NT * TF_YST, 16 + lrow, lc4, x1, yb, fstride, am);
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * TF_HEADS + h);
  if (p.rec_v) wave_amax_emit(stv, p.rec_v, (int)blockIdx.x * TF_HEADS + h);
}

// 24 frames: this file (and attn_fused_bwd.hip for the gradients); 48 frames: attn_fused48.hip, forward only
int wdno_tattn_fused_fwd48_launch(const TFusedP& p, hipStream_t st);
// 128 / 256 channels, 24 frames: attn_fused_wide.hip, forward only
int wdno_tattn_fused_fwd_wide_launch(const TFusedP& p, int C, hipStream_t st);
extern "C" int wdno_tattn_fused_takes(int C, int n_tok, int heads) {
  if (heads != TF_HEADS) return 0;
  if (C == TF_C) return n_tok == TF_NT || n_tok == 48;
  return (C == 128 || C == 256) && n_tok == TF_NT;
}

extern "C" int wdno_tattn_fused_fwd(const float* x, const float* gamma, float eps, const void* wq_hi, const void* wq_lo, const float* wq_scale,
                                    const void* wo_hi, const void* wo_lo, const float* wo_scale, const float* rot_cos, const float* rot_sin,
                                    const float* bias, float* y, float* amax_rec, float* qkv_out, float* rec_v,
                                    int64_t n_batch, int n_tok, int64_t hw, int C, int heads, float scale, wdno_stream_t s) {
  WDNO_REQUIRE(x && gamma && wq_hi && wq_lo && wq_scale && wo_hi && wo_lo && wo_scale && y && n_batch > 0 && hw > 0);
  WDNO_REQUIRE((rot_cos == nullptr) == (rot_sin == nullptr));
  if (!wdno_tattn_fused_takes(C, n_tok, heads) || hw > 0x7fffffff / (C * 48)) return WDNO_EUNSUPPORTED;
  TFusedP p;
  p.x = x; p.gamma = gamma; p.eps = eps;
  p.wq_hi = (const _Float16*)wq_hi; p.wq_lo = (const _Float16*)wq_lo; p.wq_scale = wq_scale;
  p.wo_hi = (const _Float16*)wo_hi; p.wo_lo = (const _Float16*)wo_lo; p.wo_scale = wo_scale;
  p.rcos = rot_cos; p.rsin = rot_sin; p.bias = bias;
  p.y = y; p.amax_rec = amax_rec; p.qkv_out = qkv_out;
  p.rec_v = rec_v;
  p.HW = (int)hw; p.scale = scale; p.nseq = n_batch * hw;
  if (C != TF_C) {
    if (qkv_out) return WDNO_EUNSUPPORTED;            // (nothing is kept for a backward: these levels train layer by layer; rec_v stays untouched)
    return wdno_tattn_fused_fwd_wide_launch(p, C, as_stream(s));
  }
  if (n_tok == 48) {
    if (qkv_out) return WDNO_EUNSUPPORTED;          // (only the un-fused backward of the 24-frame block asks for the projections)
    return wdno_tattn_fused_fwd48_launch(p, as_stream(s));
  }
  const int64_t grid = tf_grid(TF_BPC_FWD, p.nseq);
  tattn_fused_fwd_kernel<<<(int)grid, 256, 0, as_stream(s)>>>(p);
  return wdno_check_launch();
}

// the grids wdno_tattn_fused_fwd / wdno_tattn_fused_bwd launch for this shape (0: no such kernel). Blocks walk the n_batch * hw sequences
// with a stride of the grid: passes = ceil(nseq / grid), per step the sample advances by grid / hw and the pixel by grid % hw (with a carry).
extern "C" int wdno_tattn_fused_plan(int C, int n_tok, int64_t n_batch, int64_t hw, int* grid_fwd, int* grid_bwd) {
  WDNO_REQUIRE(grid_fwd && grid_bwd && n_batch > 0 && hw > 0);
  if (!wdno_tattn_fused_takes(C, n_tok, TF_HEADS)) return WDNO_EUNSUPPORTED;
  const int64_t nseq = n_batch * hw;
  *grid_fwd = (int)tf_grid(C != TF_C ? TF_BPC_WIDE : n_tok == 48 ? TF_BPC_FWD48 : TF_BPC_FWD, nseq);
  *grid_bwd = C == TF_C && n_tok == TF_NT ? (int)tf_grid(TF_BPC_BWD, nseq) : 0;
  return WDNO_OK;
}
