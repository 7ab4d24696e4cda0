// conv_h3.hip -- fp32-equivalent implicit-GEMM convolution on the fp16 matrix cores ("3 x fp16 split").
//
// An fp32 value v (scaled by a per-tensor power of two s so that max|v*s| < 2^15) is represented as hi + lo with
//   hi = fp16(v*s),  lo = fp16(v*s - hi)            (hi carries 11 significant bits, lo the next 11)
// and a product a*b is evaluated as  ah*bh + ah*bl + al*bh  on v_mfma_f32_32x32x16_f16 (fp16 products are exact in the
// fp32 accumulator; the dropped al*bl term and the residual of lo are <= 2^-22 relative). The result is fp32-class
// (tests: <= 2e-6 rel-L2 against fp64), while the matrix pipe runs at 1/3 of the 2.5 PFLOP/s fp16 rate instead of the
// 157 TFLOP/s of the exact-fp32 MFMA. Sub-normal flushing of lo is harmless because of the per-tensor scale: it
// perturbs only elements below 2^-18 of the tensor maximum, by <= 2^-40 of that maximum.
//
// Pre-pass (HBM-bound, conv_prep.hip): wdno_amax -> wdno_split_f16 produce the two fp16 planes [rows][C8] (C padded to 8) and the
// scale; the weight gradient with its split reductions is conv_wgrad_h3.hip. The convolution kernel is the fp32 kernel's structure (conv.hip) with 16-byte loads of 8 halves, LDS planes
// [rows][32+8] halves (80-byte rows: conflict-free ds_read_b128 / ds_write_b128) and 3 MFMAs per fragment pair.
#include "conv_tiles.h"
#include <type_traits>

#define HBK 32   // reduction elements per step
#define HST 40   // LDS row stride in halves

// ---------------------------------------------------------------------------------------------- convolution
// The fp16 MFMAs of one 32-deep step take only ~400 cycles per wave, so the per-step integer work matters as much as the
// math. All operand fetches are raw buffer loads with 32-bit byte offsets: out-of-range pieces (zero padding, tile tails)
// are given an offset beyond the descriptor's range and come back as zeros from the hardware bounds check, so there is
// no branch and no select. Offsets are (per-thread constant) + (uniform per tap) + (uniform per chunk).
// The loads are cv_load_b128 (conv_tiles.h): the kernel counts and waits for them itself, wait_set() below.

template <int BM, int BN, int WM, int WN, bool LP>
__global__ __launch_bounds__(256) void conv_fwd_h3_kernel(const _Float16* __restrict__ xh, const _Float16* __restrict__ xl,
                                                           const _Float16* __restrict__ wh, const _Float16* __restrict__ wl,
                                                           const float* __restrict__ sx, const float* __restrict__ sw,
                                                           const float* __restrict__ bias, const float* __restrict__ res,
                                                           float* __restrict__ y, ConvP p, unsigned x_bytes, unsigned w_bytes) {
  constexpr int TM = BM / (WM * 32);
  constexpr int TN = BN / (WN * 32);
  constexpr int AROWS = BM / 64;   // row passes of the 256 loader threads (64 rows x 4 column groups per pass)
  constexpr int BROWS = BN / 64;
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  constexpr int NPL = LP ? 1 : 2;                // planes per operand
  constexpr int STAGE = NPL * (BM + BN) * HST;   // [Ah | Al | Bh | Bl]  (LP: [A | B])
  const wdno_conv_geom& g = p.g;
  const int tid = threadIdx.x;
  const int tile = xcd_swizzle(blockIdx.x, p.ntiles);
  const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
  const int64_t m0 = (int64_t)tile_m * BM;
  const int n0 = tile_n * BN;
  int4v rxh = cv_rsrc(xh, x_bytes), rxl = cv_rsrc(xl, x_bytes);
  int4v rwh = cv_rsrc(wh, w_bytes), rwl = cv_rsrc(wl, w_bytes);
  asm volatile("s_nop 4" : "+s"(rxh), "+s"(rxl), "+s"(rwh), "+s"(rwl));      // SGPR write -> VMEM descriptor read wait states

  // 4 lanes cover one 64-byte row piece; consecutive lane quads take rows r and r+4 so that the 8 lanes of a
  // ds_write_b128 group hit 32 distinct banks with the 80-byte row stride (r and r+1 would overlap by 16 bytes)
  const int lq = tid >> 2;
  const int lrow = (lq & ~7) | ((lq & 1) << 2) | ((lq >> 1) & 3);          // 0..63, bijective
  const int c8 = (tid & 3) * 8;       // element offset inside the 32-wide chunk
  int a_d0[AROWS], a_h0[AROWS], a_w0[AROWS], a_base[AROWS];
  bool a_ok[AROWS];
#pragma unroll
  for (int i = 0; i < AROWS; ++i) {
    int64_t pm = m0 + lrow + 64 * i;
    a_ok[i] = pm < p.P;
    int q = a_ok[i] ? (int)pm : 0;                 // the host wrapper guarantees P < 2^31
    int ow = q % g.OW; q /= g.OW;
    int oh = q % g.OH; q /= g.OH;
    int od = q % g.OD;
    int n = q / g.OD;
    a_d0[i] = od * g.sd - g.pd;
    a_h0[i] = oh * g.sh - g.ph;
    a_w0[i] = ow * g.sw - g.pw;
    a_base[i] = (((n * g.D + a_d0[i]) * g.H + a_h0[i]) * g.W + a_w0[i]) * g.C + c8;   // element offset of (tap 0, chunk 0)
  }
  int b_base[BROWS];
  bool b_ok[BROWS];
#pragma unroll
  for (int i = 0; i < BROWS; ++i) {
    int k = n0 + lrow + 64 * i;
    b_ok[i] = k < g.K;
    b_base[i] = k * p.R + c8;
  }

  // Split over the tap rows (p.ksplit = 2, blockIdx.y): a wide layer with few pixels -- 8 x 8 x 16 samples x 1024 channels in the Burgers
  // U-Net -- has fewer tiles than CUs and 288 steps per tile; two blocks per tile each take half of the (dz, dy) rows and add their
  // partial sums with atomics onto a zeroed output (two addends: the order cannot change the result).
  const int ntap = g.kd * g.kh;
  const int t_first = p.ksplit > 1 ? ntap * (int)blockIdx.y / p.ksplit : 0;
  const int t_last = p.ksplit > 1 ? ntap * ((int)blockIdx.y + 1) / p.ksplit : ntap;
  const int nst = (t_last - t_first) * p.nchunk;          // steps of this block
  // load cursor: (tap, chunk) uniform; (dx, cc) per thread because a chunk may straddle pixels when C % 32 != 0
  int l_chunk = 0, l_dz = t_first / g.kh, l_dy = t_first % g.kh, l_r = c8, l_dx = c8 / g.C, l_cc = c8 % g.C;
  const int dx0 = l_dx, cc0 = l_cc;
  int tap_off = (l_dz * g.H + l_dy) * g.W * g.C, wtap_off = t_first * g.K * p.R;      // uniform element offsets of the current tap row in x and in the packed weights
  const int step_dx = HBK / g.C, step_cc = HBK % g.C;
  bool row_ok[AROWS];
  auto refresh_tap = [&]() {
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
      int d = a_d0[i] + l_dz, h = a_h0[i] + l_dy;
      row_ok[i] = a_ok[i] && (unsigned)d < (unsigned)g.D && (unsigned)h < (unsigned)g.H;
    }
  };
  refresh_tap();

  int4v ah[2][AROWS], al[2][AROWS], bh[2][BROWS], bl[2][BROWS];     // two register sets: loads run 2 steps ahead
  auto load_tile = [&](auto SET) {
    constexpr int S = decltype(SET)::value;
    const bool r_ok = l_r < p.R;
    const int chunk_off = l_chunk * HBK;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
      const bool ok = row_ok[i] && r_ok && (unsigned)(a_w0[i] + l_dx) < (unsigned)g.W;
      const int off = ok ? (a_base[i] + tap_off + chunk_off) * 2 : CV_OOB;
      ah[S][i] = cv_load_b128(rxh, off);
      if (!LP) al[S][i] = cv_load_b128(rxl, off);
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      const bool ok = b_ok[i] && r_ok;
      const int off = ok ? (b_base[i] + wtap_off + chunk_off) * 2 : CV_OOB;
      bh[S][i] = cv_load_b128(rwh, off);
      if (!LP) bl[S][i] = cv_load_b128(rwl, off);
    }
    ++l_chunk;
    l_r += HBK;
    l_dx += step_dx;
    l_cc += step_cc;
    if (l_cc >= g.C) { l_cc -= g.C; ++l_dx; }
    if (l_chunk == p.nchunk) {
      l_chunk = 0; l_r = c8; l_dx = dx0; l_cc = cc0;
      wtap_off += g.K * p.R;
      if (++l_dy == g.kh) { l_dy = 0; ++l_dz; }
      tap_off = (l_dz * g.H + l_dy) * g.W * g.C;
      refresh_tap();
    }
  };
  // wait until at most `newer` younger loads are outstanding; names every register of the set so that no consumer of
  // them can be scheduled above the wait
  constexpr int NLOADS = NPL * (AROWS + BROWS);
  auto wait_set = [&](auto SET, bool newer_in_flight) {
    constexpr int S = decltype(SET)::value;
    if (newer_in_flight) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NLOADS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
      int4v &r0 = ah[S][i], &r1 = al[S][LP ? 0 : i];
      if (LP) asm volatile("" : "+v"(r0));
      else asm volatile("" : "+v"(r0), "+v"(r1));
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      int4v &r0 = bh[S][i], &r1 = bl[S][LP ? 0 : i];
      if (LP) asm volatile("" : "+v"(r0));
      else asm volatile("" : "+v"(r0), "+v"(r1));
    }
  };
  auto store_tile = [&](auto SET, int buf) {
    constexpr int S = decltype(SET)::value;
    _Float16* Ah = hsm + buf * STAGE;
    _Float16* Al = Ah + BM * HST;
    _Float16* Bh = Ah + NPL * BM * HST;
    _Float16* Bl = Bh + BN * HST;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
      *reinterpret_cast<int4v*>(&Ah[(lrow + 64 * i) * HST + c8]) = ah[S][i];
      if (!LP) *reinterpret_cast<int4v*>(&Al[(lrow + 64 * i) * HST + c8]) = al[S][i];
    }
#pragma unroll
    for (int i = 0; i < BROWS; ++i) {
      *reinterpret_cast<int4v*>(&Bh[(lrow + 64 * i) * HST + c8]) = bh[S][i];
      if (!LP) *reinterpret_cast<int4v*>(&Bl[(lrow + 64 * i) * HST + c8]) = bl[S][i];
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int li = lane & 31, hh = lane >> 5;
  const int m_base = wm * (TM * 32), n_base = wn * (TN * 32);

  f32x16 acc[TM][TN];
  cv_zero_acc(acc);

  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  // step t lives in register set t & 1 and LDS stage t & 1
  auto iter = [&](auto PAR, int step) {
    constexpr int B = decltype(PAR)::value;
    const _Float16* Ah = hsm + B * STAGE;
    const _Float16* Al = Ah + BM * HST;
    const _Float16* Bh = Ah + NPL * BM * HST;
    const _Float16* Bl = Bh + BN * HST;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      half8 fah[TM], fal[TM], fbh[TN], fbl[TN];
      const int col = ks * 16 + hh * 8;
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        fah[a] = *reinterpret_cast<const half8*>(&Ah[(m_base + a * 32 + li) * HST + col]);
        if (!LP) fal[a] = *reinterpret_cast<const half8*>(&Al[(m_base + a * 32 + li) * HST + col]);
      }
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        fbh[b] = *reinterpret_cast<const half8*>(&Bh[(n_base + b * 32 + li) * HST + col]);
        if (!LP) fbl[b] = *reinterpret_cast<const half8*>(&Bl[(n_base + b * 32 + li) * HST + col]);
      }
      cv_mfma_set<LP, true>(acc, fah, fal, fbh, fbl);      // the pixel fragment is the row operand: acc is [pixel][channel]
    }
    using NXT = std::integral_constant<int, 1 - B>;
    if (step + 1 < nst) {
      wait_set(NXT{}, step + 2 < nst);      // the set of step+2 (issued one iteration later) may stay in flight
      store_tile(NXT{}, 1 - B);
    }
    __syncthreads();
    if (step + 3 < nst) load_tile(NXT{});
  };
  load_tile(S0{});
  wait_set(S0{}, false);
  store_tile(S0{}, 0);
  __syncthreads();
  if (nst > 1) load_tile(S1{});
  if (nst > 2) load_tile(S0{});
  for (int step = 0; step < nst; step += 2) {
    iter(S0{}, step);
    if (step + 1 < nst) iter(S1{}, step + 1);
  }

  const float inv = LP ? 1.0f : 1.0f / (sx[0] * sw[0]);
  float am = 0.f;
#pragma unroll
  for (int a = 0; a < TM; ++a) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      int row = (e & 3) + 8 * (e >> 2) + 4 * hh;
      int64_t pm = m0 + m_base + a * 32 + row;
      if (pm >= p.P) continue;
      int64_t yr = p.identity_out ? pm : out_row(g, pm);
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        int kc = n0 + n_base + b * 32 + li;
        if (kc < g.K) {
          float v = acc[a][b][e] * inv;
          if (p.ksplit > 1) {                    // partial sum: bias / residual ride on the first one
            if (blockIdx.y == 0) {
              if (bias) v += bias[kc];
              if (res) v += res[yr * g.K + kc];
            }
            unsafeAtomicAdd(&y[yr * g.K + kc], v);
            continue;
          }
          if (bias) v += bias[kc];
          if (res) v += res[yr * g.K + kc];
          if (LP && p.out_bf16) reinterpret_cast<unsigned short*>(y)[yr * g.K + kc] = bf16_rne(v);
          else y[yr * g.K + kc] = v;
          am = fmaxf(am, fabsf(v));
        }
      }
    }
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * 4 + wave);
}

template <int BM, int BN, int WM, int WN, bool LP>
static int launch_h3(const void* xh, const void* xl, const void* wh, const void* wl, const float* sx, const float* sw,
                     const float* bias, const float* residual, float* y, ConvP& p, const ConvFwdChoice& c, hipStream_t st) {
  const wdno_conv_geom& g = p.g;
  p.tiles_n = cdiv(g.K, BN);
  p.ntiles = c.plan.ntiles;
  p.ksplit = c.plan.ksplit;
  size_t lds = (size_t)2 * (LP ? 1 : 2) * (BM + BN) * HST * sizeof(_Float16);
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)conv_fwd_h3_kernel<BM, BN, WM, WN, LP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_done = true;
  }
  const int64_t x_elems = (int64_t)g.N * g.D * g.H * g.W * g.C;
  const int64_t w_elems = (int64_t)g.kd * g.kh * g.K * p.R;
  float* rec = p.amax_rec;
  if (p.ksplit > 1) {                     // partial sums are added onto zeros; the amax record is filled by a sweep afterwards
    if (hipMemsetAsync(y, 0, (size_t)p.P * g.K * sizeof(float), st) != hipSuccess) return WDNO_ELAUNCH;
    p.amax_rec = nullptr;
  }
  conv_fwd_h3_kernel<BM, BN, WM, WN, LP><<<dim3((unsigned)c.plan.grid, (unsigned)p.ksplit), 256, lds, st>>>(
      (const _Float16*)xh, (const _Float16*)xl, (const _Float16*)wh, (const _Float16*)wl, sx, sw, bias, residual, y, p,
      (unsigned)(x_elems * 2), (unsigned)(w_elems * 2));
  if (p.ksplit > 1 && rec) {
    conv_amax_record_launch(y, p.P * g.K, rec, st);
    p.amax_rec = rec;
  }
  return WDNO_OK;
}

// THE choice of the forward / data-gradient kernel: family, tile, splits and grid for the geometry in p (p.split_ws_bytes = what the caller
// lends for a split reduction). conv_fwd_16 launches what this says and wdno_conv_fwd_plan reports it. res_is_y: the residual is y itself.
static int conv_fwd_choose(const ConvP& p, bool lp, bool res_is_y, ConvFwdChoice& c) {
  const wdno_conv_geom* g = &p.g;
  const int64_t P = p.P;
  const int K = g->K;
  auto blocks = [&](int bm, int bn) { return cdiv64(P, bm) * cdiv(K, bn); };
  // problems with at least 100 tiles: persistent LDS-DMA kernels (256x64 / 128x128 tiles, 64x64 per compute wave); even with
  // fewer tiles than CUs they beat the register-staged kernels (l2 512->128: 0.36 -> 0.24 ms). WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV = never, _FORCE_DMA_CONV = always, _CHUNKED_DMA_CONV = always and not the tap-resident variant, _FORCE_TILES_160 / _320 = always with the five-row tile shapes (conv_h3d.hip)
  const int dbg = wdno_debug_mode;
  // ... and the tap-resident kernel (stride 1, equal grids, 3-wide) has 64 x 64 / 128 x 64 tiles for problems of fewer tiles
  const bool small_tap = p.identity_out && wdno_conv_h3t_takes(*g) && g->kw == 3 && blocks(64, 64) >= 64;
  if (dbg != WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV && (dbg == WDNO_DBG_FORCE_DMA_CONV || dbg == WDNO_DBG_CHUNKED_DMA_CONV || dbg == WDNO_DBG_FORCE_TILES_160 || dbg == WDNO_DBG_FORCE_TILES_320 || small_tap || (K > 64 ? blocks(128, 128) : blocks(256, 64)) >= 100)) {
    int rc = wdno_conv_fwd_h3_dma_choose(p, lp, c);
    if (rc != WDNO_EUNSUPPORTED) return rc;
  }
  int bm, bn, ksplit = 1;
  if (K > 64) {
    if (blocks(128, 128) >= 512 || blocks(64, 128) < 2 * blocks(128, 128)) { bm = 128; bn = 128; }
    // fewer 64 x 128 tiles than CUs (the 8 x 8 level of the Burgers U-Net at batch 16: 128 tiles of 288 steps each): 64 x 64 tiles
    else if (blocks(64, 128) < 200) {
      // ... and when even those leave CUs with a single block of several hundred steps, two blocks per tile (split over the tap rows)
      if (blocks(64, 64) <= 384 && g->kd * g->kh >= 2 && p.nsteps >= 64 && p.identity_out && !res_is_y && !lp) ksplit = 2;
      bm = 64; bn = 64;
    }
    else { bm = 64; bn = 128; }
  } else {
    if (blocks(128, 64) >= 512 || P <= 128) { bm = 128; bn = 64; }
    else { bm = 64; bn = 64; }
  }
  const int64_t nt = blocks(bm, bn);
  const int64_t x_elems = (int64_t)g->N * g->D * g->H * g->W * g->C;
  const int64_t w_elems = (int64_t)g->kd * g->kh * g->K * p.R;
  if (nt > 0x7fffffff || x_elems * 2 >= CV_OOB || w_elems * 2 >= CV_OOB || p.P >= 0x7fffffff) return WDNO_EUNSUPPORTED;   // 32-bit buffer offsets
  c.kw = g->kw; c.sp = 0;
  c.plan.family = WDNO_CONV_REG_H3;
  c.plan.bm = bm; c.plan.bn = bn;
  c.plan.uniform = 0;
  c.plan.tsplit = 1; c.plan.ksplit = ksplit;
  c.plan.ntiles = (int)nt;
  c.plan.grid = (int)nt;
  return WDNO_OK;
}

extern "C" int wdno_conv_fwd_f16x3(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                                   const float* bias, const float* residual, float* y, const wdno_conv_geom* g, wdno_stream_t s) {
  return wdno_conv_fwd_f16x3_amax(xh, xl, sx, wph, wpl, sw, bias, residual, y, nullptr, g, s);
}
template <bool LP>
static int conv_fwd_16(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                       const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g, wdno_stream_t s,
                       float* split_ws = nullptr, size_t split_ws_bytes = 0, const wdno_zero_box* zb = nullptr, int y_bf16 = 0) {
  int rc = check_geom(g);
  if (rc) return rc;
  if (g->C & 7) return WDNO_EUNSUPPORTED;       // 16-bit rows must be 16-byte multiples
  if (y_bf16 && (!LP || residual)) return WDNO_EUNSUPPORTED;      // bf16 output: single-product mode, no residual (its reader is a GroupNorm)
  ConvP p;
  fill_params(p, g);
  p.out_bf16 = y_bf16 ? 1 : 0;
  if (zb) {                                     // a statement about x, used where a kernel can (conv_h3t.hip, 7-wide taps): whole 16-channel blocks
    if (zb->channels < 0 || zb->d0 < 0 || zb->h0 < 0 || zb->w0 < 0) return WDNO_EINVAL;
    p.zb_blocks = zb->channels / 16; p.zb_d = zb->d0; p.zb_h = zb->h0;
  }
  p.amax_rec = amax_rec;
  p.split_ws = split_ws;
  p.split_ws_bytes = split_ws_bytes;
  p.nchunk = cdiv(p.R, HBK);
  p.nsteps = g->kd * g->kh * p.nchunk;
  hipStream_t st = as_stream(s);
  ConvFwdChoice c;
  rc = conv_fwd_choose(p, LP, residual != nullptr && residual == y, c);
  if (rc) return rc;
  if (c.plan.family != WDNO_CONV_REG_H3) {
    rc = wdno_conv_fwd_h3_dma(xh, LP ? nullptr : xl, wph, LP ? nullptr : wpl, sx, sw, bias, residual, y, p, c, st);
    if (rc) return rc;
    return wdno_check_launch();
  }
  const int bm = c.plan.bm, bn = c.plan.bn;
  if (bm == 128 && bn == 128) rc = launch_h3<128, 128, 2, 2, LP>(xh, xl, wph, wpl, sx, sw, bias, residual, y, p, c, st);
  else if (bm == 64 && bn == 128) rc = launch_h3<64, 128, 1, 4, LP>(xh, xl, wph, wpl, sx, sw, bias, residual, y, p, c, st);
  else if (bm == 128 && bn == 64) rc = launch_h3<128, 64, 4, 1, LP>(xh, xl, wph, wpl, sx, sw, bias, residual, y, p, c, st);
  else rc = launch_h3<64, 64, 2, 2, LP>(xh, xl, wph, wpl, sx, sw, bias, residual, y, p, c, st);
  if (rc) return rc;
  return wdno_check_launch();
}
extern "C" int wdno_conv_fwd_f16x3_amax(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                                        const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g,
                                        wdno_stream_t s) {
  return conv_fwd_16<false>(xh, xl, sx, wph, wpl, sw, bias, residual, y, amax_rec, g, s);
}
// ... with a workspace for the partial sums of a split reduction (conv_h3t.hip): wdno_conv_fwd_split_ws_bytes() bytes, 0 = this geometry
// never splits. Same results contract; the partial sums are added in a fixed order.
extern "C" int wdno_conv_fwd_f16x3_ws(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                                      const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g,
                                      void* ws, size_t ws_bytes, wdno_stream_t s) {
  return conv_fwd_16<false>(xh, xl, sx, wph, wpl, sw, bias, residual, y, amax_rec, g, s, (float*)ws, ws ? ws_bytes : 0);
}
// ... with a statement about structural zeros of x (wdno_zero_box, include/wdno_hip.h): same results bit for bit (up to the sign of a zero),
// the 7 x 7 x 7 stem skips the reduction stages that only see such zeros
extern "C" int wdno_conv_fwd_f16x3_zbox(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                                        const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g,
                                        const wdno_zero_box* zb, wdno_stream_t s) {
  return conv_fwd_16<false>(xh, xl, sx, wph, wpl, sw, bias, residual, y, amax_rec, g, s, nullptr, 0, zb);
}
// single-product form with both options: zb (may be NULL) as above; y_bf16 != 0: y is bf16 storage [rows][K] -- the output of a convolution whose
// only reader is a GroupNorm (and the data gradient whose only reader is a GroupNorm's backward): wdno_groupnorm_*_t take it as it is
extern "C" int wdno_conv_fwd_bf16_ex(const void* x16, const void* wp16, const float* bias, const float* residual, void* y, int y_bf16, float* amax_rec,
                                     const wdno_conv_geom* g, const wdno_zero_box* zb, wdno_stream_t s) {
  return conv_fwd_16<true>(x16, x16, nullptr, wp16, wp16, nullptr, bias, residual, (float*)y, amax_rec, g, s, nullptr, 0, zb, y_bf16);
}
extern "C" size_t wdno_conv_fwd_split_ws_bytes(const wdno_conv_geom* g) {
  if (!g || check_geom(g) || (g->C & 7)) return 0;
  ConvP p;
  fill_params(p, g);
  if (!p.identity_out || !wdno_conv_h3t_takes(*g)) return 0;
  const int runs = wdno_conv_h3t_split(*g, p.P, wdno_num_cus() & ~7);
  return runs > 1 ? (size_t)runs * p.P * g->K * sizeof(float) : 0;
}
extern "C" int wdno_conv_fwd_plan(const wdno_conv_geom* g, int lowp, int residual_is_y, size_t split_ws_bytes, wdno_conv_plan* out) {
  WDNO_REQUIRE(out);
  int rc = check_geom(g);
  if (rc) return rc;
  if (lowp < 0 || (g->C & 7)) return wdno_conv_fwd_fp32_plan(g, out);
  ConvP p;
  fill_params(p, g);
  p.split_ws_bytes = split_ws_bytes;
  p.nchunk = cdiv(p.R, HBK);
  p.nsteps = g->kd * g->kh * p.nchunk;
  ConvFwdChoice c;
  rc = conv_fwd_choose(p, lowp != 0, residual_is_y != 0, c);
  if (rc) return rc;
  *out = c.plan;
  return WDNO_OK;
}
extern "C" int wdno_conv_fwd_bf16(const void* x16, const void* wp16, const float* bias, const float* residual, float* y, float* amax_rec,
                                  const wdno_conv_geom* g, wdno_stream_t s) {
  return conv_fwd_16<true>(x16, x16, nullptr, wp16, wp16, nullptr, bias, residual, y, amax_rec, g, s);
}
