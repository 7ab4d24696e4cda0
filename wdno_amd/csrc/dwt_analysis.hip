// dwt_analysis.hip -- the fused single-launch analysis (2-D / 3-D signal -> packed coefficients) and the choice of its tile; the scheme of
// the fused transforms and the steps shared with the synthesis kernels are in dwt_tiles.h, the per-axis reference in dwt.hip.
#include "dwt_tiles.h"
#include <algorithm>

// ND = 3: register pass along T, NK coefficient frames per block.  ND = 2: register pass along H, NK coefficient rows per item.
template <int ND, int L, int MODE, int NK, bool PACKED = false>
__global__ __launch_bounds__(256) void dwt_analysis_fused_kernel(const float* __restrict__ x, float* __restrict__ coef, FusedGeom g, Taps t) {
  extern __shared__ float lds[];
  int img, tt, th;
  dw_tile<ND>(blockIdx.x, g, img, tt, th);
  const int FW = g.FW, NH = g.NH, off = g.off;
  const int kh0 = th * NH;
  const int nh = min(NH, g.Ho - kh0);
  const float* __restrict__ xi = x + (int64_t)img * g.T * g.H * g.W;
  constexpr int NP = (ND == 3) ? 2 * NK : 1;
  float* S2;                                     // [NP][2][NH][FW]
  int kt0 = 0;
  if (ND == 3) {
    const int FH = 2 * NH + L - 2;               // signal rows under the tile: row r <-> h = 2 kh0 - off + r
    const int rows = 2 * nh + L - 2;
    float* S1 = lds;                             // [2 NK][FH][FW]
    S2 = lds + 2 * NK * FH * FW;                 // (sized by fused_analysis below; as a call to a layout function 12 of the 15 3-D kernels change)
    kt0 = tt * NK;
    const int64_t fs = (int64_t)g.H * g.W;
    // (measured and dropped: batches of 2 / 3 items with all their frame loads requested first and 32-bit offsets: 25.4-25.9 us against 17.8)
    for (int it = threadIdx.x; it < rows * FW; it += 256) {
      const int r = fd_div(it, g.dFW), c = it - r * FW;
      const int h = amap<MODE>(2 * kh0 - off + r, g.H, g.odd_h);
      const int w = amap<MODE>(c - off, g.W, g.odd_w);
      float lo[NK], hi[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) { lo[k] = 0.f; hi[k] = 0.f; }
      if (h >= 0 && w >= 0) {
        const float* col = xi + (int64_t)h * g.W + w;
#pragma unroll
        for (int jj = 0; jj < 2 * NK + L - 2; ++jj) {
          const int tj = amap<MODE>(2 * kt0 - off + jj, g.T, g.odd_t);
          const float v = tj >= 0 ? col[tj * fs] : 0.f;
          dw_scatter<L, NK>(v, jj, t, lo, hi);
        }
      }
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        S1[(k * FH + r) * FW + c] = lo[k];
        S1[((NK + k) * FH + r) * FW + c] = hi[k];
      }
    }
    __syncthreads();
    // pass H: an item is a COLUMN (plane p, column c) of S1: its nh outputs slide a window of L values down the column (two new reads per
    // output instead of L, one index decode per column instead of one per output); every sum in the order m = 0 .. L - 1 as before
    for (int it = threadIdx.x; it < NP * FW; it += 256) {
      const int p = fd_div(it, g.dFW), c = it - p * FW;
      const float* col = S1 + p * FH * FW + c;
      float* o0 = S2 + (p * 2 * NH) * FW + c;
      float w[L];
#pragma unroll
      for (int m = 0; m < L - 2; ++m) w[m + 2] = col[m * FW];
      col += (L - 2) * FW;
      for (int kh = 0; kh < nh; ++kh) {
#pragma unroll
        for (int m = 0; m < L - 2; ++m) w[m] = w[m + 2];
        w[L - 2] = col[0]; w[L - 1] = col[FW];
        col += 2 * FW;
        float lo, hi;
        dw_dot<L>(w, t, lo, hi);
        o0[kh * FW] = lo;
        o0[(NH + kh) * FW] = hi;
      }
    }
  } else {
    // 2-D: register pass along H straight from global memory. With periodization (MODE 0) a row of S2 holds ONE period (FW = 2 Wo columns,
    // set by the host): column c <-> w = (c - off) mod period, and the W pass below wraps its reads -- the L - 2 boundary columns of the
    // extended row were 272 items for 256 threads at W = 128 (a second round of global loads for 16 threads). The source rows of an item
    // are consecutive modulo the period: one wrap, then increments (16 boundary maps and 64-bit address products per item before).
    S2 = lds;
    const int ngroups = (nh + NK - 1) / NK;
    const int PH = g.H + g.odd_h;
    for (int it = threadIdx.x; it < ngroups * FW; it += 256) {
      const int gq = fd_div(it, g.dFW);
      const int c = it - gq * FW, k0 = gq * NK;
      const int w = amap<MODE>(c - off, g.W, g.odd_w);
      float lo[NK], hi[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) { lo[k] = 0.f; hi[k] = 0.f; }
      if (w >= 0) {
        const int hb = 2 * (kh0 + k0) - off;
        int hv = MODE == 0 ? wrap_period(hb, PH) : hb;              // MODE 0: position within the period; MODE 1: the row index itself
        float v[2 * NK + L - 2];
#pragma unroll
        for (int jj = 0; jj < 2 * NK + L - 2; ++jj) {
          int hj;
          if (MODE == 0) { hj = min(hv, g.H - 1); hv = hv + 1 == PH ? 0 : hv + 1; }
          else { hj = (hv >= 0 && hv < g.H) ? hv : -1; ++hv; }
          v[jj] = hj >= 0 ? xi[hj * g.W + w] : 0.f;                  // (host: an image has < 2^31 elements)
        }
#pragma unroll
        for (int jj = 0; jj < 2 * NK + L - 2; ++jj) dw_scatter<L, NK>(v[jj], jj, t, lo, hi);
      }
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k0 + k < nh) {
          S2[(k0 + k) * FW + c] = lo[k];
          S2[(NH + k0 + k) * FW + c] = hi[k];
        }
    }
  }
  __syncthreads();
  // pass W: LDS -> packed coefficients. float2 reads (index 2 kw + m): conflict-free, and m ascends inside each pair
  float* __restrict__ ci = coef + (int64_t)img * g.cs_img;
  const float* __restrict__ rs = nullptr;
  if (PACKED) {
    const int io = fd_div(img, g.dInner), ii = img - io * g.img_inner;
    ci = coef + (int64_t)io * g.cs_outer + (int64_t)ii * g.cs_img;
    rs = g.resc + ii * (1 << ND);
  }
  const int Wo = g.Wo;
  constexpr bool PERIOD_ROWS = ND == 2 && MODE == 0;          // S2 rows hold one period: float2 index kw + i wraps at Wo
  // an item = FOUR consecutive coefficients of one row: a window of L / 2 + 3 float2 reads (instead of 4 L / 2) and one row decode
  constexpr int HLW = L / 2;
  const int Wo4 = PACKED ? g.row_w >> 2 : (Wo + 3) >> 2;
  const int rmax = PERIOD_ROWS ? Wo - 1 : (FW >> 1) - 1;       // last float2 of a row
  for (int it = threadIdx.x; it < NP * 2 * NH * Wo4; it += 256) {
    int q = fd_div(it, g.dQW4);
    const int kw0 = (it - q * Wo4) * 4;
    const int q2 = fd_div(q, g.dNH), kh = q - q2 * NH;
    if (kh >= nh) continue;
    const int bh = q2 & 1, p = q2 >> 1;
    const int bt = (ND == 3) ? p / NK : 0;
    const int kt = (ND == 3) ? kt0 + p % NK : 0;
    if (ND == 3 && kt >= g.To) continue;
    const float2* row0 = reinterpret_cast<const float2*>(S2 + ((p * 2 + bh) * NH + kh) * FW);
    float2 v[HLW + 3];
#pragma unroll
    for (int i = 0; i < HLW + 3; ++i) {
      int idx = kw0 + i;
      if (PERIOD_ROWS) idx = idx >= Wo ? idx - Wo : idx;
      v[i] = row0[min(idx, rmax)];                             // (past the row only for the coefficients kw >= Wo of a ragged last group: not stored)
    }
    int band_lo, band_hi;
    dw_bands<ND>(bt, bh, band_lo, band_hi);
    float* o = ci + (int64_t)kt * g.cs0 + (int64_t)(kh0 + kh) * g.cs1 + kw0;
    float r_lo = 1.f, r_hi = 1.f;
    if (PACKED) { r_lo = rs[band_lo]; r_hi = rs[band_hi]; }
    float pl[4], ph[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float lo = 0.f, hi = 0.f;
#pragma unroll
      for (int i = 0; i < HLW; ++i) {
        lo = fmaf(t.lo[L - 1 - 2 * i], v[u + i].x, lo);
        hi = fmaf(t.hi[L - 1 - 2 * i], v[u + i].x, hi);
        lo = fmaf(t.lo[L - 2 - 2 * i], v[u + i].y, lo);
        hi = fmaf(t.hi[L - 2 - 2 * i], v[u + i].y, hi);
      }
      if (PACKED) {
        const bool in = kw0 + u < Wo;
        pl[u] = (in ? lo : 0.f) / r_lo; ph[u] = (in ? hi : 0.f) / r_hi;
        continue;
      }
      if (kw0 + u < Wo) {
        o[band_lo * g.cs_band + u] = lo;
        o[band_hi * g.cs_band + u] = hi;
      }
    }
    if (PACKED) {
      *reinterpret_cast<float4*>(o + band_lo * g.cs_band) = make_float4(pl[0], pl[1], pl[2], pl[3]);
      *reinterpret_cast<float4*>(o + band_hi * g.cs_band) = make_float4(ph[0], ph[1], ph[2], ph[3]);
    }
  }
}

// decide: the tile geometry and the kernel of an analysis, nothing launched. false = not covered by the fused kernel.
template <int ND, int L, int MODE>
static bool analysis_decide(const float* dst, const wdno_dwt_desc* d, bool odd_rule, const PackedStore* pk, FusedGeom& g, FusedChoice& c) {
  g = dw_geom(d, L, MODE);
  const bool odd = MODE == 0 && odd_rule;
  g.odd_t = odd && (g.T & 1); g.odd_h = odd && (g.H & 1); g.odd_w = odd && (g.W & 1);
  g.FW = (ND == 2 && MODE == 0) ? 2 * g.Wo : 2 * g.Wo + L - 2;        // 2-D periodization: one period per LDS row (see the kernel)
  if ((int64_t)g.T * g.H * g.W >= (1ll << 31)) return false;
  constexpr int NK = (ND == 3) ? 3 : 4;
  size_t lds;
  if (ND == 3) {
    // floats: 2 NK FW (FH + 2 NH) with FH = 2 NH + L - 2
    const size_t per_row = (size_t)2 * NK * g.FW * sizeof(float);
    const long nh_max = ((long)(dwt_fused_lds_budget(32) / per_row) - (L - 2)) / 4;
    if (nh_max < 1) return false;
    const int tiles = cdiv(g.Ho, (int)std::min<long>(nh_max, g.Ho));
    g.NH = cdiv(g.Ho, tiles);
    g.tiles_h = tiles;
    g.tiles_t = cdiv(g.To, NK);
    lds = per_row * (size_t)(4 * g.NH + L - 2);
  } else {
    const size_t per_row = (size_t)2 * g.FW * sizeof(float);
    long nh_max = (long)(dwt_fused_lds_budget(32) / per_row);
    nh_max = std::min<long>(nh_max / NK * NK, 2 * NK);        // two register groups per block: plenty of blocks for small images
    if (nh_max < NK) return false;
    g.NH = (int)nh_max;
    g.tiles_h = cdiv(g.Ho, g.NH);
    g.tiles_t = 1;
    lds = per_row * (size_t)g.NH;
  }
  const int64_t nb = (int64_t)g.n_img * g.tiles_t * g.tiles_h;
  if (nb > 0x7fffffff) return false;
  g.n_blocks = (int)nb;
  g.dFW = make_fastdiv(g.FW); g.dNH = make_fastdiv(g.NH); g.dWo = make_fastdiv(g.Wo); g.dQW4 = make_fastdiv((g.Wo + 3) / 4);
  if ((int64_t)2 * NK * 2 * g.NH * std::max(g.FW, g.Wo) * (int64_t)std::max(g.FW, g.NH) >= (1ll << 32)) return false;   // fd_div range
  c = FusedChoice{WDNO_DWT_ANALYSIS, 0, lds};
  if (pk) {
    if (!(ND == 3 && MODE == 1)) return false;   // the smoke pipeline's transform (zero mode, 3-D); other shapes: not instantiated
    g.img_inner = pk->img_inner; g.cs_outer = pk->cs_outer; g.resc = pk->resc; g.row_w = pk->row_w;
    g.dInner = make_fastdiv(g.img_inner);
    g.dQW4 = make_fastdiv(g.row_w / 4);
    if (g.row_w < g.Wo || (g.row_w & 3) || ((g.cs_img | g.cs_band | g.cs0 | g.cs1 | g.cs_outer) & 3) || ((uintptr_t)dst & 15)) return false;
    if ((int64_t)2 * NK * 2 * g.NH * g.row_w * (int64_t)std::max(g.FW, g.NH) >= (1ll << 32)) return false;   // fd_div range
    if ((int64_t)g.n_img * g.img_inner >= (1ll << 32)) return false;
    c.family = WDNO_DWT_ANALYSIS_PACKED;
  }
  return true;
}

// launch: what analysis_decide chose
template <int ND, int L, int MODE>
static void analysis_launch(const FusedChoice& c, const float* src, float* dst, const FusedGeom& g, const Taps& taps, hipStream_t st) {
  constexpr int NK = (ND == 3) ? 3 : 4;
  if (c.family == WDNO_DWT_ANALYSIS_PACKED) {
    if constexpr (ND == 3 && MODE == 1) dwt_analysis_fused_kernel<ND, L, MODE, NK, true><<<g.n_blocks, 256, c.lds, st>>>(src, dst, g, taps);
    return;
  }
  dwt_analysis_fused_kernel<ND, L, MODE, NK><<<g.n_blocks, 256, c.lds, st>>>(src, dst, g, taps);
}

template <int ND, int L, int MODE>
static bool fused_analysis(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, bool odd_rule, hipStream_t st, const PackedStore* pk,
                           wdno_dwt_plan* plan) {
  FusedGeom g;
  FusedChoice c;
  if (!analysis_decide<ND, L, MODE>(dst, d, odd_rule, pk, g, c)) return false;
  if (plan) dw_plan_of(g, c, plan);
  else analysis_launch<ND, L, MODE>(c, src, dst, g, taps, st);
  return true;
}

template <int ND, int L>
static bool fused_analysis_mode(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, bool odd_rule, hipStream_t st, const PackedStore* pk,
                                wdno_dwt_plan* plan) {
  return d->mode == 1 ? fused_analysis<ND, L, 1>(src, dst, d, taps, odd_rule, st, pk, plan) : fused_analysis<ND, L, 0>(src, dst, d, taps, odd_rule, st, pk, plan);
}
template <int ND>
static bool fused_analysis_nd(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, bool odd_rule, hipStream_t st, const PackedStore* pk,
                              wdno_dwt_plan* plan) {
  switch (d->L) {
    case 2: return fused_analysis_mode<ND, 2>(src, dst, d, taps, odd_rule, st, pk, plan);
    case 4: return fused_analysis_mode<ND, 4>(src, dst, d, taps, odd_rule, st, pk, plan);
    case 6: return fused_analysis_mode<ND, 6>(src, dst, d, taps, odd_rule, st, pk, plan);
    case 8: return fused_analysis_mode<ND, 8>(src, dst, d, taps, odd_rule, st, pk, plan);
    case 10: return fused_analysis_mode<ND, 10>(src, dst, d, taps, odd_rule, st, pk, plan);
    default: return false;
  }
}
bool dwt_fused_analysis(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, bool odd_rule, hipStream_t st, const PackedStore* pk,
                        wdno_dwt_plan* plan) {
  return d->nd == 3 ? fused_analysis_nd<3>(src, dst, d, taps, odd_rule, st, pk, plan) : fused_analysis_nd<2>(src, dst, d, taps, odd_rule, st, pk, plan);
}
