// dwt_synthesis.hip -- the fused single-launch synthesis kernels (packed coefficients -> 2-D / 3-D signal) and the choice among them; the
// scheme of the fused transforms and the steps the kernels share are in dwt_tiles.h, the per-axis reference in dwt.hip.
#include "dwt_tiles.h"
#include <algorithm>

// q = (n + off) >> 1, r = (n + off) & 1: x[n] = sum_i lo[q - i] g_lo[r + 2 i] + hi[q - i] g_hi[r + 2 i], i < L/2.
// ND = 3: register pass along T with NQ q-frames (2 NQ signal frames) per block. ND = 2: register pass along H, NQ q-rows per item.
template <int ND, int L, int MODE, int NQ>
__global__ __launch_bounds__(256) void dwt_synthesis_fused_kernel(const float* __restrict__ coef, float* __restrict__ x, FusedGeom g, Taps t) {
  extern __shared__ float lds[];
  constexpr int E = L / 2 - 1;
  constexpr int ET = NQ + E;
  int img, tt, th;
  dw_tile<ND>(blockIdx.x, g, img, tt, th);
  const int NW = g.FW, QW = NW >> 1, NQH = g.NH;
  const int EH = NQH + E;
  const int qh_start = g.qh0 + th * NQH;
  const int nqh = min(NQH, g.qh0 + g.QH - qh_start);       // valid q rows of this tile
  const int qt_start = (ND == 3) ? g.qt0 + tt * NQ : 0;
  const float* __restrict__ ci = coef + (int64_t)img * g.cs_img;
  float* __restrict__ xi = x + (int64_t)img * g.T * g.H * g.W;
  constexpr int NP = (ND == 3) ? 2 * ET : 1;
  float* S1 = lds;                                           // [NP][2][EH][NW]
  // pass W: packed coefficients -> S1
  const int eh_used = nqh + E;
  // Branch-free body: every load is issued unconditionally from a clamped (always valid) address and masked by a select, so that
  // the loads of several items are in flight together (with early-outs the loop was a chain of dependent L2 round trips: 22 of the
  // kernel's 42 us at [32, 8, 18, 34, 34]). A masked term contributes fmaf(0, tap, a) = a, i.e. the skipped fmaf of the per-axis kernel.
  // WB items per round: their WB * L loads are all requested before the first is used (a thread has 6 items at the Burgers shape; with the
  // compiler's 2-item unroll that was three dependent round trips to L2 / HBM per block).
  constexpr int WB = (ND == 2) ? 3 : 2;
  constexpr int HL = L / 2;
  const int n_w = NP * 2 * EH * QW;
  if (g.debug != WDNO_DBG_DWT_SKIP_W_PASS)
  for (int it0 = threadIdx.x; it0 < n_w; it0 += 256 * WB) {
    float cl[WB][HL], ch[WB][HL];
    unsigned okm[WB];
    int dst[WB];
#pragma unroll
    for (int u = 0; u < WB; ++u) {
      const bool live = it0 + 256 * u < n_w;
      const int it = live ? it0 + 256 * u : 0;                  // (a slot past the end decodes item 0: every address stays inside the image)
      int q = fd_div(it, g.dQW);
      const int ql = it - q * QW;
      const int q2 = fd_div(q, g.dEH), eh = q - q2 * EH;
      const int bh = q2 & 1, p = q2 >> 1;
      const int bt = (ND == 3) ? p / ET : 0;
      const int Kt = (ND == 3) ? smap<MODE>(qt_start - E + p % ET, g.To) : 0;
      const int Kh = smap<MODE>(qh_start - E + eh, g.Ho);
      const bool rowok = live && Kt >= 0 && Kh >= 0;
      int band_lo, band_hi;
      dw_bands<ND>(bt, bh, band_lo, band_hi);
      const int base = rowok ? (int)((int64_t)Kt * g.cs0 + (int64_t)Kh * g.cs1) : 0;        // (host: cs_img < 2^31)
      const float* rl = ci + band_lo * g.cs_band;
      const float* rh = ci + band_hi * g.cs_band;
      okm[u] = 0;
      dst[u] = (live && eh < eh_used) ? ((p * 2 + bh) * EH + eh) * NW + 2 * ql : -1;
#pragma unroll
      for (int i = 0; i < HL; ++i) {
        const int Kw = smap<MODE>(g.qw0 + ql - i, g.Wo);
        const int o = base + (Kw >= 0 ? Kw : 0);
        cl[u][i] = rl[o]; ch[u][i] = rh[o];
        okm[u] |= (rowok && Kw >= 0) ? (1u << i) : 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < WB; ++u) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int i = 0; i < HL; ++i) {
        const bool ok = (okm[u] >> i) & 1u;
        dw_pair_term(ok ? cl[u][i] : 0.f, ok ? ch[u][i] : 0.f, t, i, a0, a1);
      }
      if (dst[u] >= 0) *reinterpret_cast<float2*>(S1 + dst[u]) = make_float2(a0, a1);
    }
  }
  __syncthreads();
  if (ND == 3) {
    float* S2 = lds + NP * 2 * EH * NW;                      // [2 ET][2 NQH][NW] (sized by fused_synthesis; as a call to a layout function 6 of the 10 kernels change)
    if (g.debug != WDNO_DBG_DWT_SKIP_H_PASS)
#pragma unroll 2
    for (int it = threadIdx.x; it < NP * 2 * NQH * NW; it += 256) {
      int q = fd_div(it, g.dFW);
      const int pw = it - q * NW;
      const int p = fd_div(q, g.dNQH2), ph = q - p * 2 * NQH;
      if (ph >= 2 * nqh) continue;
      const int ql = ph >> 1, r = ph & 1;
      const float* cl = S1 + ((p * 2 + 0) * EH + ql + E) * NW + pw;
      const float* ch = S1 + ((p * 2 + 1) * EH + ql + E) * NW + pw;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < L / 2; ++i) {
        acc = fmaf(cl[-i * NW], r ? t.lo[2 * i + 1] : t.lo[2 * i], acc);
        acc = fmaf(ch[-i * NW], r ? t.hi[2 * i + 1] : t.hi[2 * i], acc);
      }
      S2[(p * 2 * NQH + ph) * NW + pw] = acc;
    }
    __syncthreads();
    if (g.debug != WDNO_DBG_DWT_SKIP_T_PASS)
    for (int it = threadIdx.x; it < 2 * nqh * NW; it += 256) {
      const int ph = fd_div(it, g.dFW), pw = it - ph * NW;
      const int nw = pw - (g.off & 1);                         // position pw <-> n_w = pw - (off & 1)
      const int nhh = 2 * (qh_start + (ph >> 1)) + (ph & 1) - g.off;
      if (nw < 0 || nw >= g.W || nhh < 0 || nhh >= g.H) continue;      // (these three lines also stand in the streaming kernel: as a function both kernels change)
      float cl[ET], ch[ET];
#pragma unroll
      for (int e = 0; e < ET; ++e) {
        cl[e] = S2[(e * 2 * NQH + ph) * NW + pw];
        ch[e] = S2[((ET + e) * 2 * NQH + ph) * NW + pw];
      }
      float* o = xi + (int64_t)nhh * g.W + nw;
#pragma unroll
      for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
        for (int r = 0; r < 2; ++r) dw_store_t(o, g, qt_start, qq, r, dw_column<L>(cl, ch, t, qq, r));
    }
  } else {
    // register pass along H: items (group of NQ q-rows, pw); EH rows of S1 hold the tile's coefficient rows (after the W pass). The same lines
    // close dwt_synthesis2_kernel (there with a 32-bit row offset in the store): as one function, with either form of the address, the L = 2
    // kernels of both come out shorter.
    const int wshift = g.off & 1;
    const int ngroups = (nqh + NQ - 1) / NQ;
    for (int it = threadIdx.x; it < ngroups * NW; it += 256) {
      const int gq = fd_div(it, g.dFW);
      const int pw = it - gq * NW, q0 = gq * NQ;
      const int nw = pw - wshift;
      if (nw < 0 || nw >= g.W) continue;
      float cl[ET], ch[ET];
#pragma unroll
      for (int e = 0; e < ET; ++e) {
        const bool ok = q0 + e < eh_used;
        cl[e] = ok ? S1[(q0 + e) * NW + pw] : 0.f;
        ch[e] = ok ? S1[(EH + q0 + e) * NW + pw] : 0.f;
      }
#pragma unroll
      for (int qq = 0; qq < NQ; ++qq) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const float acc = dw_column<L>(cl, ch, t, qq, r);
          const int nhh = 2 * (qh_start + q0 + qq) + r - g.off;
          if (q0 + qq < nqh && nhh >= 0 && nhh < g.H) xi[(int64_t)nhh * g.W + nw] = acc;
        }
      }
    }
  }
}


// Round 3: 2-D synthesis with the W pass fed from LDS. Ablation of the kernel above at the Burgers shape ([128, 4, 80, 64] -> [128, 160, 128],
// bior2.4, periodization; 14.8 us for 21 MB; tools/bench_dwt.py): without its loads 8.1 us, without the H pass 9.3, without the W pass 5.6.
// All 1280 blocks are resident at once (5 per CU) and the kernel lasts as long as ONE block's chain load -> W pass -> H pass -> store:
// what shortens it is fewer dependent round trips, not fewer instructions (a variant whose blocks walk several tiles with the next tile's
// rows prefetched into registers was slower for every tile count: 15.3 / 17.2 / 19.8 / 24.5 us at 1 / 2 / 3 / 5 tiles per block).
//   * staging: the tile's raw coefficient rows go to LDS -- row (band pair bh, coefficient row eh, lo / hi) holds the RW = 4 ceil(QW / 4)
//     + L / 2 - 1 coefficients K = qw0 - (L / 2 - 1) + p with the boundary rule applied (wrapped or zero). A wave takes whole rows (row
//     index and map are wave-uniform), a lane the same columns of every row; all loads of a thread are in flight together.
//   * W pass: an item is FOUR consecutive output pairs of one row: a window of L / 2 + 3 values per band from LDS instead of 4 * L / 2
//     global loads with a boundary map each.
//   * H pass: as above (register pass over NQ q-rows per item).
// Every sum keeps the order i = 0, 1, .. of the per-axis kernel: bit-identical (tests/test_gpu_dwt_fused.py).
template <int L, int MODE, int NQ, int PMAX>
__global__ __launch_bounds__(256) void dwt_synthesis2_kernel(const float* __restrict__ coef, float* __restrict__ x, FusedGeom g, Taps t) {
  extern __shared__ float lds[];
  constexpr int E = L / 2 - 1, ET = NQ + E, HL = L / 2, RMAX = 2 * NQ + E;       // rows per wave: 4 EH / 4, EH <= 2 NQ + E (host)
  const int NW = g.FW, QW = NW >> 1, NQH = g.NH;
  const int EH = NQH + E;
  const int QW4 = (QW + 3) >> 2, RW = 4 * QW4 + HL - 1;       // = dw_staged_row_width(QW4, L); inline: as a call, 4 of the 20 kernels change
  float* S1 = lds;                                            // [2 bh][EH][NW]
  float* R = lds + dw_synthesis2_lds<1>(NW, EH, RW);      // [2 bh][EH][lo, hi][RW]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // columns of this lane in a staged row (two per pass of 128; RW <= 128 PMAX by the host's choice): the same for every tile
  int kw[PMAX][2];
  bool colok[PMAX][2];
#pragma unroll
  for (int pp = 0; pp < PMAX; ++pp)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pidx = 128 * pp + 64 * h + lane;
      const int Kw = smap<MODE>(g.qw0 - (HL - 1) + min(pidx, RW - 1), g.Wo);
      colok[pp][h] = Kw >= 0 && pidx < RW;
      kw[pp][h] = Kw >= 0 ? Kw : 0;
    }
  constexpr int npp = PMAX;
  float v[PMAX][2][RMAX];
  auto tile_of = [&](int tile, int& img, int& qh_start) {
    int tt, th;
    dw_tile<2>(tile, g, img, tt, th);
    qh_start = g.qh0 + th * NQH;
  };
  auto fetch = [&](int tile) {
    int img, qh_start;
    tile_of(tile, img, qh_start);
    const float* __restrict__ ci = coef + (int64_t)img * g.cs_img;
#pragma unroll
    for (int pp = 0; pp < PMAX; ++pp) {
      if (pp >= npp) break;
#pragma unroll
      for (int rr = 0; rr < RMAX; ++rr) {
        const int r = wave + 4 * rr;                          // r = (bh * EH + eh) * 2 + band
        if (r >= 4 * EH) break;
        const int band = r & 1, q2 = r >> 1;
        const int bh = q2 >= EH ? 1 : 0, eh = q2 - bh * EH;
        const int Kh = smap<MODE>(qh_start - E + eh, g.Ho);
        const float* row = ci + (bh + 2 * band) * g.cs_band + (int64_t)(Kh >= 0 ? Kh : 0) * g.cs1;
        v[pp][0][rr] = row[kw[pp][0]];
        v[pp][1][rr] = row[kw[pp][1]];
      }
    }
  };
  const int tile = blockIdx.x;
  fetch(tile);
  {
    int img, qh_start;
    tile_of(tile, img, qh_start);
    const int nqh = min(NQH, g.qh0 + g.QH - qh_start);
    const int eh_used = nqh + E;
    float* __restrict__ xi = x + (int64_t)img * g.T * g.H * g.W;
    // registers -> R
#pragma unroll
    for (int pp = 0; pp < PMAX; ++pp) {
      if (pp >= npp) break;
#pragma unroll
      for (int rr = 0; rr < RMAX; ++rr) {
        const int r = wave + 4 * rr;
        if (r >= 4 * EH) break;
        const int q2 = r >> 1;
        const int eh = q2 >= EH ? q2 - EH : q2;
        const bool rowok = smap<MODE>(qh_start - E + eh, g.Ho) >= 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int pidx = 128 * pp + 64 * h + lane;
          if (pidx < RW) R[r * RW + pidx] = (colok[pp][h] && rowok) ? v[pp][h][rr] : 0.f;
        }
      }
    }
    __syncthreads();
    // pass W: R -> S1
    for (int it = threadIdx.x; it < 2 * EH * QW4; it += 256) {
      const int q2 = fd_div(it, g.dQW4), j = it - q2 * QW4;    // q2 = bh * EH + eh
      const int eh = q2 >= EH ? q2 - EH : q2;
      if (eh >= eh_used) continue;
      const float* wl = R + (q2 * 2) * RW + 4 * j;
      const float* wh = wl + RW;
      float cl[HL + 3], ch[HL + 3];
#pragma unroll
      for (int e = 0; e < HL + 3; ++e) { cl[e] = wl[e]; ch[e] = wh[e]; }
      float o8[8];
#pragma unroll
      for (int tq = 0; tq < 4; ++tq) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int i = 0; i < HL; ++i) dw_pair_term(cl[tq + HL - 1 - i], ch[tq + HL - 1 - i], t, i, a0, a1);
        o8[2 * tq] = a0; o8[2 * tq + 1] = a1;
      }
      float* d = S1 + q2 * NW + 8 * j;
      if (4 * j + 3 < QW && (NW & 3) == 0) {
        *reinterpret_cast<float4*>(d) = make_float4(o8[0], o8[1], o8[2], o8[3]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(o8[4], o8[5], o8[6], o8[7]);
      } else {
#pragma unroll
        for (int tq = 0; tq < 4; ++tq)
          if (4 * j + tq < QW) { d[2 * tq] = o8[2 * tq]; d[2 * tq + 1] = o8[2 * tq + 1]; }
      }
    }
    __syncthreads();
    // pass H (registers): items (group of NQ q-rows, pw), as in dwt_synthesis_fused_kernel<2, ..>
    const int wshift = g.off & 1;
    const int ngroups = (nqh + NQ - 1) / NQ;
    for (int it = threadIdx.x; it < ngroups * NW; it += 256) {
      const int gq = fd_div(it, g.dFW);
      const int pw = it - gq * NW, q0 = gq * NQ;
      const int nw = pw - wshift;
      if (nw < 0 || nw >= g.W) continue;
      float cl[ET], ch[ET];
#pragma unroll
      for (int e = 0; e < ET; ++e) {
        const bool ok = q0 + e < eh_used;
        cl[e] = ok ? S1[(q0 + e) * NW + pw] : 0.f;
        ch[e] = ok ? S1[(EH + q0 + e) * NW + pw] : 0.f;
      }
#pragma unroll
      for (int qq = 0; qq < NQ; ++qq) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const float acc = dw_column<L>(cl, ch, t, qq, r);
          const int nhh = 2 * (qh_start + q0 + qq) + r - g.off;
          if (q0 + qq < nqh && nhh >= 0 && nhh < g.H) xi[nhh * g.W + nw] = acc;
        }
      }
    }
  }
}

// Round 3: 3-D synthesis that STREAMS over the coefficient frames of its tile. The kernel above keeps the W-pass and H-pass results of
// all ET = NQ + E coefficient frames of a tile in LDS (12 planes for bior1.3), which leaves room for 2 q-rows per tile at 40 KB: 4896 blocks
// for [32, 8, 18, 34, 34], each coefficient read 3x through L2 and every W-pass item computed 3x (halo 6/4 in T times 4/2 in H). Here only ONE
// frame is in LDS at a time (W pass -> S1, H pass -> S2, 20 KB for 8 q-rows); the T pass is an accumulation in registers: a thread owns
// ITEMS output columns (ph, pw) and 2 NQ time samples of each, and every staged frame adds its lo / hi contribution to the <= L/2 q-frames it
// belongs to. Frames are walked in DESCENDING order so that each accumulator receives its terms in the order i = 0, 1, .. of the
// per-axis kernel (K = q - i): results stay BIT-IDENTICAL to it (tests/test_gpu_dwt_fused.py). WDNO_DBG_DWT3_SYNTH_LDS: the kernel above (A/B).
// The kernel is bound by VALU issue, not by memory (4 blocks per CU run concurrently; ~2.5 K wave instructions per wave at 4 cycles each were 19 of
// its 25 us): so (a) everything that does not depend on the frame -- the (band, row, column) decode of a thread's W- and H-pass items, the
// boundary maps, the LDS offsets -- is computed once before the frame loop, (b) an H-pass item produces BOTH rows 2 ql, 2 ql + 1 from one set
// of L reads, (c) the global loads of frame e - 1 are issued before the H / T passes of frame e. 30.0 -> 25.3 (c) -> 16.1 us (a, b) at
// [32,8,18,34,34]; 70.5 -> 56.4 -> 32.5 us at [10,8,34,66,66].
template <int L, int MODE, int NQ, int ITEMS, int WMAX>
__global__ __launch_bounds__(256) void dwt_synthesis3_stream_kernel(const float* __restrict__ coef, float* __restrict__ x, FusedGeom g, Taps t) {
  extern __shared__ float lds[];
  constexpr int E = L / 2 - 1;
  constexpr int ET = NQ + E;
  constexpr int HL = L / 2;
  int img, tt, th;
  dw_tile<3>(blockIdx.x, g, img, tt, th);
  const int NW = g.FW, QW = NW >> 1, NQH = g.NH;
  const int EH = NQH + E;
  const int qh_start = g.qh0 + th * NQH;
  const int nqh = min(NQH, g.qh0 + g.QH - qh_start);
  const int qt_start = g.qt0 + tt * NQ;
  const int eh_used = nqh + E;
  const float* __restrict__ ci = coef + (int64_t)img * g.cs_img;
  float* __restrict__ xi = x + (int64_t)img * g.T * g.H * g.W;
  float* S1 = lds;                              // [2 bt][2 bh][EH][NW]
  float* S2 = lds + dw_stream_lds<1>(NW, EH, NQH);      // [2 bt][2 NQH][NW]
  const int n_items = 2 * nqh * NW;             // output columns (ph, pw) of this tile
  // W-pass items of this thread: the same (band pair, coefficient row, column pair) in every frame, so the index work is done ONCE and a
  // frame is only its offset Kt * cs0 (the decode per frame was half of the pass's instructions). The loads of frame e - 1 are issued
  // before the H / T passes of frame e and wait in registers: a block's chain of six exposed global-load latencies (one per frame; the
  // blocks of a CU all run concurrently, so the kernel lasts as long as ONE block's chain) becomes one.
  int w_dst[WMAX], w_off[WMAX][HL];
  unsigned w_ok[WMAX];
  const int n_w = 4 * EH * QW;
#pragma unroll
  for (int k = 0; k < WMAX; ++k) {
    const int it = threadIdx.x + 256 * k;
    int q = fd_div(it, g.dQW);
    const int ql = it - q * QW;
    const int q2 = fd_div(q, g.dEH), eh = q - q2 * EH;
    const int bh = q2 & 1, bt = q2 >> 1;
    const int Kh = smap<MODE>(qh_start - E + eh, g.Ho);
    const bool rowok = Kh >= 0 && it < n_w;
    int band_lo, band_hi;
    dw_bands<3>(bt, bh, band_lo, band_hi);
    const int src = rowok ? (int)(band_lo * g.cs_band + (int64_t)Kh * g.cs1) : 0;      // (host: cs_img < 2^31)
    w_dst[k] = (it < n_w && eh < eh_used) ? (q2 * EH + eh) * NW + 2 * ql : -1;
    w_ok[k] = 0;
#pragma unroll
    for (int i = 0; i < HL; ++i) {
      const int Kw = smap<MODE>(g.qw0 + ql - i, g.Wo);
      w_off[k][i] = src + (rowok && Kw >= 0 ? Kw : 0);
      w_ok[k] |= (rowok && Kw >= 0) ? (1u << i) : 0u;
    }
  }
  float pl[WMAX][HL], ph_[WMAX][HL];
  auto fetch = [&](int e) {
    const int Kt = smap<MODE>(qt_start - E + e, g.To);
    const float* fl = ci + (int64_t)(Kt >= 0 ? Kt : 0) * g.cs0;          // block-uniform bases: the loads are saddr + 32-bit offset
    const float* fh = fl + g.cs_band;
#pragma unroll
    for (int k = 0; k < WMAX; ++k) {
      if (256 * k >= n_w) continue;             // block-uniform: item slots past the tile's count neither load nor compute
#pragma unroll
      for (int i = 0; i < HL; ++i) { pl[k][i] = fl[w_off[k][i]]; ph_[k][i] = fh[w_off[k][i]]; }
    }
  };
  // H-pass items of this thread: (bt, q-row, column) -> BOTH output rows 2 ql, 2 ql + 1 from the same L reads of S1 (each chain in the
  // order of the per-axis kernel); offsets fixed for all frames
  constexpr int HMAX = ITEMS;                   // 2 NQH NW <= 256 ITEMS by the host's choice of NQH
  int h_src[HMAX], h_dst[HMAX];
#pragma unroll
  for (int k = 0; k < HMAX; ++k) {
    const int it = threadIdx.x + 256 * k;
    const int q = fd_div(it, g.dFW);            // bt * NQH + ql
    const int pw = it - q * NW;
    const int bt = q >= NQH ? 1 : 0, ql = q - bt * NQH;
    const bool ok = it < 2 * NQH * NW && ql < nqh;
    h_src[k] = ok ? ((bt * 2) * EH + ql + E) * NW + pw : -1;
    h_dst[k] = (bt * 2 * NQH + 2 * ql) * NW + pw;
  }
  float acc[ITEMS][NQ][2];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j)
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) { acc[j][qq][0] = 0.f; acc[j][qq][1] = 0.f; }
  fetch(ET - 1);
#pragma unroll
  for (int e = ET - 1; e >= 0; --e) {
    const int Kt = smap<MODE>(qt_start - E + e, g.To);
    const bool live = Kt >= 0;                  // a frame outside the tensor contributes fmaf(0, tap, acc) = acc (block-uniform)
    if (live) {
      // pass W: the prefetched coefficients of frame Kt -> S1
#pragma unroll
      for (int k = 0; k < WMAX; ++k) {
        if (256 * k >= n_w) continue;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int i = 0; i < HL; ++i) {
          const bool ok = (w_ok[k] >> i) & 1u;
          dw_pair_term(ok ? pl[k][i] : 0.f, ok ? ph_[k][i] : 0.f, t, i, a0, a1);
        }
        if (w_dst[k] >= 0) *reinterpret_cast<float2*>(S1 + w_dst[k]) = make_float2(a0, a1);
      }
    }
    if (e > 0) fetch(e - 1);
    if (!live) continue;
    __syncthreads();
    // pass H: S1 -> S2
#pragma unroll
    for (int k = 0; k < HMAX; ++k) {
      if (h_src[k] < 0) continue;
      const float* cl = S1 + h_src[k];
      const float* ch = cl + EH * NW;
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int i = 0; i < HL; ++i) dw_pair_term(cl[-i * NW], ch[-i * NW], t, i, a0, a1);
      S2[h_dst[k]] = a0;
      S2[h_dst[k] + NW] = a1;
    }
    __syncthreads();
    // pass T: this frame's term of every q-frame it belongs to (i = qq + E - e in [0, E])
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const int it = threadIdx.x + 256 * j;
      if (it < n_items) {
        const float cl = S2[it], ch = S2[2 * NQH * NW + it];        // (ph, pw) = it / NW, it % NW: S2 rows are NW wide, so the item index is the offset
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq) {
          const int i = qq + E - e;
          if (i >= 0 && i <= E) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              acc[j][qq][r] = fmaf(cl, t.lo[r + 2 * i], acc[j][qq][r]);
              acc[j][qq][r] = fmaf(ch, t.hi[r + 2 * i], acc[j][qq][r]);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int it = threadIdx.x + 256 * j;
    if (it >= n_items) continue;
    const int ph = fd_div(it, g.dFW), pw = it - ph * NW;
    const int nw = pw - (g.off & 1);
    const int nhh = 2 * (qh_start + (ph >> 1)) + (ph & 1) - g.off;
    if (nw < 0 || nw >= g.W || nhh < 0 || nhh >= g.H) continue;        // (as in dwt_synthesis_fused_kernel<3, ..>)
    float* o = xi + (int64_t)nhh * g.W + nw;
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
      for (int r = 0; r < 2; ++r) dw_store_t(o, g, qt_start, qq, r, acc[j][qq][r]);
  }
}

// decide: the tile geometry and the kernel of a synthesis, nothing launched. false = not covered by a fused kernel.
template <int ND, int L, int MODE>
static bool synthesis_decide(const wdno_dwt_desc* d, FusedGeom& g, FusedChoice& c) {
  g = dw_geom(d, L, MODE);
  constexpr int E = L / 2 - 1;
  auto qcount = [&](int N) { return ((N - 1 + g.off) >> 1) - (g.off >> 1) + 1; };
  g.qt0 = g.qh0 = g.qw0 = g.off >> 1;
  g.QH = qcount(g.H);
  g.QT = qcount(g.T);
  g.FW = 2 * qcount(g.W);
  if (g.cs_img >= (1ll << 31) || (int64_t)g.T * g.H * g.W >= (1ll << 31)) return false;      // 32-bit offsets within an image
  constexpr int NQ = 4;
  size_t lds;
  if (ND == 3 && wdno_debug_mode != WDNO_DBG_DWT3_SYNTH_LDS) {
    // streaming kernel: q-rows per tile from the register budget (ITEMS columns of 2 NQ samples per thread) and a 32 KB LDS budget.
    // tile shape: 2 columns per thread, NQ = 4 q-frames per tile. Measured on [32,8,18,34,34] / [10,8,34,66,66] with this kernel (us):
    // 2 col NQ 4: 16.1 / 33.3; 3 col: 17.2 / 42.0; 4 col: 19.7 / 37.4; 2 col NQ 8: 17.8 / 31.8; 3 col NQ 8: 21.5 / 47.1
    auto stream = [&]() -> bool {
      constexpr int ITEMS = 2;
      const int NW = g.FW;
      int nqh = (ITEMS * 256) / (2 * NW);
      const int lds_rows = (int)(dwt_fused_lds_budget(32) / ((size_t)NW * sizeof(float)));      // 4 (NQH + E) + 4 NQH rows of NW floats
      nqh = std::min(nqh, (lds_rows - 4 * E) / 8);
      nqh = std::min(nqh, g.QH);
      if (nqh < 1 || g.cs_img >= (1ll << 31)) return false;
      const int tiles = cdiv(g.QH, nqh);
      g.NH = cdiv(g.QH, tiles);
      g.tiles_h = tiles;
      g.tiles_t = cdiv(g.QT, NQ);
      const size_t lds = (size_t)dw_stream_lds<2>(NW, g.NH + E, g.NH) * sizeof(float);
      const int64_t nbs = (int64_t)g.n_img * g.tiles_t * g.tiles_h;
      const int n_w = 4 * (g.NH + E) * (NW / 2);               // W-pass items of a frame: WMAX per thread, held in registers
      if (nbs > 0x7fffffff || n_w > 8 * 256 || (int64_t)4 * (g.NH + E) * NW * (int64_t)std::max(NW, 2 * (g.NH + E)) >= (1ll << 32)) return false;
      g.n_blocks = (int)nbs;
      g.dFW = make_fastdiv(NW); g.dQW = make_fastdiv(NW / 2); g.dEH = make_fastdiv(g.NH + E); g.dNQH2 = make_fastdiv(2 * g.NH);
      g.debug = 0;
      c = FusedChoice{WDNO_DWT_SYNTHESIS3_STREAM, n_w <= 4 * 256 ? 4 : 8, lds};
      return true;
    };
    if (stream()) return true;
  }
  const int RW = dw_staged_row_width((g.FW / 2 + 3) / 4, L);
  bool staged = false;
  if (ND == 3) {
    // floats: 2 ET NW (2 EH + 2 NQH), EH = NQH + E
    const size_t per_row = (size_t)2 * (NQ + E) * g.FW * sizeof(float);
    const long nq_max = ((long)(dwt_fused_lds_budget(40) / per_row) - 2 * E) / 4;
    if (nq_max < 1) return false;
    const int tiles = cdiv(g.QH, (int)std::min<long>(nq_max, g.QH));
    g.NH = cdiv(g.QH, tiles);
    g.tiles_h = tiles;
    g.tiles_t = cdiv(g.QT, NQ);
    lds = per_row * (size_t)(4 * g.NH + 2 * E);
  } else {
    const size_t per_row = (size_t)2 * g.FW * sizeof(float);
    long nq_max = (long)(dwt_fused_lds_budget(40) / per_row) - E;
    nq_max = std::min<long>(nq_max / NQ * NQ, 2 * NQ);
    if (nq_max < NQ) return false;
    g.NH = (int)nq_max;                                       // NH + E <= 2 NQ + E <= 16: the staged W pass keeps one register per row of a wave
    g.tiles_h = cdiv(g.QH, g.NH);
    g.tiles_t = 1;
    // dwt_synthesis2_kernel: S1 + its staged raw rows. Rows too wide to stage (RW > 256) go to dwt_synthesis_fused_kernel<2, ..>, which has
    // S1 alone (asking for the staged rows there as well went past 64 KB from W = 520 on, L = 10)
    staged = g.NH + E <= 2 * NQ + E && RW <= 256;
    lds = staged ? (size_t)dw_synthesis2_lds<2>(g.FW, g.NH + E, RW) * sizeof(float) : per_row * (size_t)(g.NH + E);
  }
  const int64_t nb = (int64_t)g.n_img * g.tiles_t * g.tiles_h;
  if (nb > 0x7fffffff) return false;
  g.n_blocks = (int)nb;
  g.dFW = make_fastdiv(g.FW); g.dQW = make_fastdiv(g.FW / 2); g.dEH = make_fastdiv(g.NH + E); g.dNQH2 = make_fastdiv(2 * g.NH);
  g.dQW4 = make_fastdiv((g.FW / 2 + 3) / 4); g.dRW = make_fastdiv(RW);
  g.debug = wdno_debug_mode;
  if (staged) {
    c = FusedChoice{WDNO_DWT_SYNTHESIS2, RW <= 128 ? 1 : 2, lds};
    return true;
  }
  if ((int64_t)2 * (NQ + E) * 2 * (g.NH + E) * g.FW * (int64_t)std::max(g.FW, 2 * (g.NH + E)) >= (1ll << 32)) return false;   // fd_div range
  c = FusedChoice{WDNO_DWT_SYNTHESIS_FUSED, 0, lds};
  return true;
}

// launch: what synthesis_decide chose
template <int ND, int L, int MODE>
static void synthesis_launch(const FusedChoice& c, const float* src, float* dst, const FusedGeom& g, const Taps& taps, hipStream_t st) {
  constexpr int NQ = 4;
  const int nb = g.n_blocks;
  if (c.family == WDNO_DWT_SYNTHESIS3_STREAM) {
    if (c.variant == 4) dwt_synthesis3_stream_kernel<L, MODE, NQ, 2, 4><<<nb, 256, c.lds, st>>>(src, dst, g, taps);
    else dwt_synthesis3_stream_kernel<L, MODE, NQ, 2, 8><<<nb, 256, c.lds, st>>>(src, dst, g, taps);
  } else if (c.family == WDNO_DWT_SYNTHESIS2) {
    if (c.variant == 1) dwt_synthesis2_kernel<L, MODE, NQ, 1><<<nb, 256, c.lds, st>>>(src, dst, g, taps);
    else dwt_synthesis2_kernel<L, MODE, NQ, 2><<<nb, 256, c.lds, st>>>(src, dst, g, taps);
  } else {
    dwt_synthesis_fused_kernel<ND, L, MODE, NQ><<<nb, 256, c.lds, st>>>(src, dst, g, taps);
  }
}

template <int ND, int L, int MODE>
static bool fused_synthesis(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, hipStream_t st, wdno_dwt_plan* plan) {
  FusedGeom g;
  FusedChoice c;
  if (!synthesis_decide<ND, L, MODE>(d, g, c)) return false;
  if (plan) dw_plan_of(g, c, plan);
  else synthesis_launch<ND, L, MODE>(c, src, dst, g, taps, st);
  return true;
}

template <int ND>
static bool fused_synthesis_nd(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, hipStream_t st, wdno_dwt_plan* plan) {
  const bool zero = d->mode == 1;
  switch (d->L) {
    case 2: return zero ? fused_synthesis<ND, 2, 1>(src, dst, d, taps, st, plan) : fused_synthesis<ND, 2, 0>(src, dst, d, taps, st, plan);
    case 4: return zero ? fused_synthesis<ND, 4, 1>(src, dst, d, taps, st, plan) : fused_synthesis<ND, 4, 0>(src, dst, d, taps, st, plan);
    case 6: return zero ? fused_synthesis<ND, 6, 1>(src, dst, d, taps, st, plan) : fused_synthesis<ND, 6, 0>(src, dst, d, taps, st, plan);
    case 8: return zero ? fused_synthesis<ND, 8, 1>(src, dst, d, taps, st, plan) : fused_synthesis<ND, 8, 0>(src, dst, d, taps, st, plan);
    case 10: return zero ? fused_synthesis<ND, 10, 1>(src, dst, d, taps, st, plan) : fused_synthesis<ND, 10, 0>(src, dst, d, taps, st, plan);
    default: return false;
  }
}
bool dwt_fused_synthesis(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, hipStream_t st, wdno_dwt_plan* plan) {
  return d->nd == 3 ? fused_synthesis_nd<3>(src, dst, d, taps, st, plan) : fused_synthesis_nd<2>(src, dst, d, taps, st, plan);
}
