// conv_wgrad_h3.hip -- weight gradient of the 16-bit convolutions (arithmetic: conv_h3.hip): the pixel table, the register-staged kernel, the
// ordered split reductions with their multi-tensor form, and THE choice between this kernel and the LDS-DMA ones of conv_wgrad_h3d.hip
// (plan query and entry points).
#include "conv_tiles.h"

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* ptr, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), (short)0, (int)bytes, 0x00020000);
}

// dwp[tap][k][r] = sum_p dy[p][k] * x[p shifted by tap][r]. The reduction index (pixels) is the SLOW index of both
// operands in memory, while v_mfma_f32_32x32x16_f16 wants 8 consecutive reduction elements per lane. The LDS tiles keep
// the natural [pixel][channel] layout (16-byte coalesced loads / stores) and the fragments are read with the gfx950
// transpose read ds_read_b64_tr_b16: inside a 16-lane group, lanes 4j..4j+3 point at the four 8-byte pieces of pixel
// row j (16 channels) and lane c receives channel c of rows 0..3 (verified by tools/probes/tr_probe.hip). Two reads
// give the 8 pixels of one MFMA operand. Rows are padded by 32 halves so the 4 pixel rows of a group fall on distinct
// 64-byte bank quarters.
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
#define WH_BKP 32
#define WH_PAD 32

// pixel table: one 16-byte record per output pixel, built once per geometry (host-cached):
//   x = physical output row (dy / y row index), y = element offset of input pixel (d0, h0, w0) (tap dz = dy = 0, may be
//   negative), z = d0 << 16 | (h0 & 0xffff), w = w0          with d0 = od*sd - pd etc.
__global__ __launch_bounds__(256) void pixel_table_kernel(int4v* __restrict__ tbl, wdno_conv_geom g, int P) {
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  int q = p;
  int ow = q % g.OW; q /= g.OW;
  int oh = q % g.OH; q /= g.OH;
  int od = q % g.OD;
  int n = q / g.OD;
  int d0 = od * g.sd - g.pd, h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
  int4v e;
  e.x = ((n * g.YD + (od * g.osd + g.ood)) * g.YH + (oh * g.osh + g.ooh)) * g.YW + (ow * g.osw + g.oow);
  e.y = (((n * g.D + d0) * g.H + h0) * g.W + w0) * g.C;
  e.z = (d0 << 16) | (h0 & 0xffff);
  e.w = w0;
  tbl[p] = e;
}
extern "C" int wdno_conv_pixel_table(void* table, const wdno_conv_geom* g, wdno_stream_t s) {
  int rc = check_geom(g);
  if (rc) return rc;
  int64_t P = (int64_t)g->N * g->OD * g->OH * g->OW;
  if (P >= 0x7fffffff || (int64_t)g->N * g->D * g->H * g->W * g->C >= 0x3fffffff) return WDNO_EUNSUPPORTED;
  pixel_table_kernel<<<(unsigned)cdiv64(P, 256), 256, 0, as_stream(s)>>>((int4v*)table, *g, (int)P);
  return wdno_check_launch();
}

struct WgradHP {
  ConvP c;
  int tiles_k, tiles_r, splits, bn;
  int64_t pix_per_split;
  int xcd_group;      // blocks renumbered so that each XCD owns a contiguous range of (split, tile) pairs
};

__device__ __forceinline__ half8 tr_frag(const _Float16* tile, int stride, int pix0, int ch0, int lane) {
  // operand fragment for channels ch0..ch0+31 (lane&31 mapping of the MFMA) and pixels pix0..pix0+15
  const int g = lane >> 4, xl = lane & 15;
  const _Float16* p0 = tile + (pix0 + 8 * (g >> 1) + (xl >> 2)) * stride + ch0 + 16 * (g & 1) + 4 * (xl & 3);
  typedef short short4v __attribute__((ext_vector_type(4)));
  typedef short4v __attribute__((address_space(3))) * lds_s4;
  short4v a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p0));
  short4v b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p0 + 4 * stride));
  typedef short short8v __attribute__((ext_vector_type(8)));
  short8v c = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(half8, c);
}

#define WH_RING 4
template <int BM, int BN, int WM, int WN, bool LP>
__global__ __launch_bounds__(256) void conv_wgrad_h3_kernel(const _Float16* __restrict__ xh, const _Float16* __restrict__ xl,
                                                             const _Float16* __restrict__ dyh, const _Float16* __restrict__ dyl,
                                                             const float* __restrict__ sx, const float* __restrict__ sdy,
                                                             const int4v* __restrict__ table, float* __restrict__ ws, WgradHP wpz,
                                                             unsigned x_bytes, unsigned dy_bytes) {
  constexpr int TM = BM / (WM * 32);
  constexpr int TN = BN / (WN * 32);
  constexpr int SA = BM + WH_PAD, SB = BN + WH_PAD;          // LDS row strides (halves)
  constexpr int A_C8 = BM / 8, B_C8 = BN / 8;                 // 16-byte pieces per pixel row
  constexpr int A_RPP = 256 / A_C8;                           // pixel rows per pass
  constexpr int A_PASSES = WH_BKP / A_RPP, B_PASSES = WH_BKP * B_C8 / 256;
  static_assert(256 % A_C8 == 0 && (WH_BKP * B_C8) % 256 == 0, "loader mapping");
  constexpr int NPL = LP ? 1 : 2;
  constexpr int STAGE = NPL * WH_BKP * (SA + SB);             // halves per stage: Ah, Al, Bh, Bl (LP: A, B)
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  int4v* pinfo = reinterpret_cast<int4v*>(hsm + 2 * STAGE);   // [WH_RING][WH_BKP]

  const ConvP& p = wpz.c;
  const wdno_conv_geom& g = p.g;
  const int tid = threadIdx.x;
  // (pixel split, k tile, tap row, r tile) from the block number, r tile fastest -- after xcd_swizzle, so that every XCD
  // (block b runs on XCD b % 8) works on one contiguous range of them: the tiles of a pixel split then pull that split's dy
  // and x rows through ONE L2. Unswizzled, the 27 tiles of a split of the 128 -> 64 level-0 layer sit on all eight XCDs and the
  // launch moves 4.6 GB over the fabric for 236 MB of operands.
  int b = wpz.xcd_group ? xcd_swizzle((int)(blockIdx.y * gridDim.x + blockIdx.x), (int)(gridDim.x * gridDim.y))
                        : (int)(blockIdx.y * gridDim.x + blockIdx.x);
  const int split = b / (int)gridDim.x;
  b -= split * (int)gridDim.x;
  const int tile_r = b % wpz.tiles_r; b /= wpz.tiles_r;
  const int tap = b % (g.kd * g.kh);
  const int tile_k = b / (g.kd * g.kh);
  const int dz = tap / g.kh, dyy = tap - dz * g.kh;
  const int k0 = tile_k * BM, r0 = tile_r * BN;
  const int pbeg = (int)((int64_t)split * wpz.pix_per_split);
  int pend = pbeg + (int)wpz.pix_per_split;
  if (pend > (int)p.P) pend = (int)p.P;
  const int nsteps = pbeg < pend ? (pend - pbeg + WH_BKP - 1) / WH_BKP : 0;
  const __amdgpu_buffer_rsrc_t rxh = make_rsrc(xh, x_bytes), rxl = make_rsrc(xl, x_bytes);
  const __amdgpu_buffer_rsrc_t rdh = make_rsrc(dyh, dy_bytes), rdl = make_rsrc(dyl, dy_bytes);
  const int tap_off = (dz * g.H + dyy) * g.W * g.C;          // uniform element offset of this block's tap row

  // pixel records travel table -> register -> LDS ring, several steps ahead of their use
  auto fetch_rec = [&](int step) -> int4v {
    int4v e;
    e.x = 0; e.y = 0; e.z = (int)0x80008000; e.w = 0;         // d0 = h0 = -32768: never valid
    int pm = pbeg + step * WH_BKP + tid;
    if (tid < WH_BKP && step < nsteps && pm < pend) e = table[pm];
    if (tid < WH_BKP && !(step < nsteps && pm < pend)) e.x = -1;
    return e;
  };
  auto put_rec = [&](int step, int4v e) {
    if (tid < WH_BKP) pinfo[(step & (WH_RING - 1)) * WH_BKP + tid] = e;
  };

  // B pieces: piece index tid + 256*i -> (pixel row, 8-channel group); BN need not divide 256 (192-wide tiles)
  int b_row[B_PASSES], b_c8[B_PASSES], r[B_PASSES], dx[B_PASSES];
  bool r_ok[B_PASSES];
#pragma unroll
  for (int i = 0; i < B_PASSES; ++i) {
    const int idx = tid + 256 * i;
    b_row[i] = idx / B_C8;
    b_c8[i] = (idx - b_row[i] * B_C8) * 8;
    r[i] = r0 + b_c8[i];
    r_ok[i] = r[i] < p.R;
    dx[i] = r[i] / g.C;
  }
  const int a_row = tid / A_C8, a_c8 = (tid % A_C8) * 8;
  const int ka = k0 + a_c8;
  const bool ka_ok = ka < g.K;

  int4v ah[A_PASSES], al[A_PASSES], bh[B_PASSES], bl[B_PASSES];
  auto load_tile = [&](int step) {
    const int4v* ps = pinfo + (step & (WH_RING - 1)) * WH_BKP;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      const int4v e = ps[a_row + i * A_RPP];
      const int off = (e.x >= 0 && ka_ok) ? (e.x * g.K + ka) * 2 : CV_OOB;
      ah[i] = __builtin_amdgcn_raw_buffer_load_b128(rdh, off, 0, 0);
      if (!LP) al[i] = __builtin_amdgcn_raw_buffer_load_b128(rdl, off, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) {
      const int4v e = ps[b_row[i]];
      const int d = (e.z >> 16) + dz, h = (int)(short)(e.z & 0xffff) + dyy, w = e.w + dx[i];
      const bool ok = e.x >= 0 && r_ok[i] && (unsigned)d < (unsigned)g.D && (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)g.W;
      const int off = ok ? (e.y + tap_off + r[i]) * 2 : CV_OOB;
      bh[i] = __builtin_amdgcn_raw_buffer_load_b128(rxh, off, 0, 0);
      if (!LP) bl[i] = __builtin_amdgcn_raw_buffer_load_b128(rxl, off, 0, 0);
    }
  };
  auto store_tile = [&](int buf) {
    _Float16* Ah = hsm + buf * STAGE;
    _Float16* Al = Ah + WH_BKP * SA;
    _Float16* Bh = Ah + NPL * WH_BKP * SA;
    _Float16* Bl = Bh + WH_BKP * SB;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
      *reinterpret_cast<int4v*>(&Ah[(a_row + i * A_RPP) * SA + a_c8]) = ah[i];
      if (!LP) *reinterpret_cast<int4v*>(&Al[(a_row + i * A_RPP) * SA + a_c8]) = al[i];
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) {
      *reinterpret_cast<int4v*>(&Bh[b_row[i] * SB + b_c8[i]]) = bh[i];
      if (!LP) *reinterpret_cast<int4v*>(&Bl[b_row[i] * SB + b_c8[i]]) = bl[i];
    }
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave - wm * WN;
  const int li = lane & 31, hh = lane >> 5;
  const int m_base = wm * (TM * 32), n_base = wn * (TN * 32);
  f32x16 acc[TM][TN];
  cv_zero_acc(acc);

  if (nsteps > 0) {
    put_rec(0, fetch_rec(0));
    put_rec(1, fetch_rec(1));
    put_rec(2, fetch_rec(2));
    int4v rec = fetch_rec(3);            // record of step s+3 is written to LDS during iteration s, loaded one iteration earlier
    __syncthreads();
    load_tile(0);
    store_tile(0);
    __syncthreads();
    if (nsteps > 1) load_tile(1);
    for (int step = 0; step < nsteps; ++step) {
      const _Float16* Ah = hsm + (step & 1) * STAGE;
      const _Float16* Al = Ah + WH_BKP * SA;
      const _Float16* Bh = Ah + NPL * WH_BKP * SA;
      const _Float16* Bl = Bh + WH_BKP * SB;
      put_rec(step + 3, rec);            // slot (step+3)&3 was last read by load_tile(step-1): two barriers ago
      rec = fetch_rec(step + 4);
#pragma unroll
      for (int ks = 0; ks < WH_BKP / 16; ++ks) {
        half8 fah[TM], fal[TM], fbh[TN], fbl[TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) {
          fah[a] = tr_frag(Ah, SA, ks * 16, m_base + a * 32, lane);
          if (!LP) fal[a] = tr_frag(Al, SA, ks * 16, m_base + a * 32, lane);
        }
#pragma unroll
        for (int bb = 0; bb < TN; ++bb) {
          fbh[bb] = tr_frag(Bh, SB, ks * 16, n_base + bb * 32, lane);
          if (!LP) fbl[bb] = tr_frag(Bl, SB, ks * 16, n_base + bb * 32, lane);
        }
        cv_mfma_set<LP, true>(acc, fah, fal, fbh, fbl);      // the dy fragment (k) is the row operand: acc is [k][r]
      }
      if (step + 1 < nsteps) store_tile((step + 1) & 1);
      __syncthreads();
      if (step + 2 < nsteps) load_tile(step + 2);
    }
  }

  const float inv = LP ? 1.0f : 1.0f / (sx[0] * sdy[0]);
  float* out = ws + ((int64_t)split * (g.kd * g.kh) + tap) * (int64_t)g.K * p.R;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      int kk = k0 + m_base + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (kk >= g.K) continue;
#pragma unroll
      for (int bb = 0; bb < TN; ++bb) {
        int rr = r0 + n_base + bb * 32 + li;
        if (rr < p.R) out[(int64_t)kk * p.R + rr] = acc[a][bb][e] * inv;
      }
    }
}

__global__ __launch_bounds__(256) void wgrad_h3_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t n, int splits) {
  // one float4 column per thread, four independent chains over the splits (a fixed order: the result is deterministic)
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = 0;
    for (; s + 3 < splits; s += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 v = *reinterpret_cast<const float4*>(ws + (int64_t)(s + u) * n + 4 * i);
        a[u].x += v.x; a[u].y += v.y; a[u].z += v.z; a[u].w += v.w;
      }
    }
    for (; s < splits; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(ws + (int64_t)s * n + 4 * i);
      a[0].x += v.x; a[0].y += v.y; a[0].z += v.z; a[0].w += v.w;
    }
    *reinterpret_cast<float4*>(out + 4 * i) = make_float4((a[0].x + a[1].x) + (a[2].x + a[3].x), (a[0].y + a[1].y) + (a[2].y + a[3].y),
                                                          (a[0].z + a[1].z) + (a[2].z + a[3].z), (a[0].w + a[1].w) + (a[2].w + a[3].w));
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      float acc = 0.f;
      for (int s = 0; s < splits; ++s) acc += ws[(int64_t)s * n + i];
      out[i] = acc;
    }
}

static void wgrad_h3_plan(WgradHP& w, const wdno_conv_geom* g) {
  fill_params(w.c, g);
  w.xcd_group = wdno_debug_mode != WDNO_DBG_WGRAD_NO_XCD_GROUPING;      // plain block order (the A/B)
  const int BM = g->K > 64 ? 128 : 64;
  w.tiles_k = cdiv(g->K, BM);
  // column tile of the kw*C run: 192 for the wide-K kernel (64 x 96 per wave beats 64 x 64), and for K <= 64 only when it
  // removes a half-empty tile (kw*C = 192: the 3-wide taps of the 64-channel layers)
  w.bn = (g->K > 64 || (w.c.R % 128 != 0 && w.c.R % 192 == 0)) ? 192 : 128;
  w.tiles_r = cdiv(w.c.R, w.bn);
  int64_t tiles = (int64_t)w.tiles_k * w.tiles_r * g->kd * g->kh;
  int64_t want = 512 / tiles;       // at most 512 blocks (floor): whole rounds of the 256 CUs, never a short extra round
  if (want < 1) want = 1;
  int64_t max_splits = cdiv64(w.c.P, 16 * WH_BKP);   // at least 16 steps per block
  if (want > max_splits) want = max_splits;
  if (want < 1) want = 1;
  if (want > 4096) want = 4096;
  int64_t pps = cdiv64(cdiv64(w.c.P, want), WH_BKP) * WH_BKP;
  w.pix_per_split = pps;
  w.splits = (int)cdiv64(w.c.P, pps);
}
extern "C" size_t wdno_conv_wgrad_f16x3_ws_bytes(const wdno_conv_geom* g) {
  if (check_geom(g) != WDNO_OK) return 0;
  WgradHP w;
  wgrad_h3_plan(w, g);
  int bm, bn, splits, pps, sp_mode;
  wdno_wgrad_h3d_plan(g, &bm, &bn, &splits, &pps, &sp_mode);       // the DMA kernel's plan may use a different split count
  if (splits > w.splits) w.splits = splits;
  return (size_t)w.splits * g->kd * g->kh * (size_t)g->K * w.c.R * sizeof(float);
}
template <int BM, int BN, int WM, int WN, bool LP>
static void launch_wgrad_h3(const void* xh, const void* xl, const void* dyh, const void* dyl, const float* sx, const float* sdy,
                            const void* table, float* wsf, const WgradHP& w, dim3 grid, hipStream_t st) {
  const wdno_conv_geom& g = w.c.g;
  const unsigned x_bytes = (unsigned)((int64_t)g.N * g.D * g.H * g.W * g.C * 2);
  const unsigned dy_bytes = (unsigned)((int64_t)g.N * g.YD * g.YH * g.YW * g.K * 2);
  size_t lds = (size_t)2 * (LP ? 1 : 2) * WH_BKP * (BM + WH_PAD + BN + WH_PAD) * sizeof(_Float16) + WH_RING * WH_BKP * sizeof(int4v);
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)conv_wgrad_h3_kernel<BM, BN, WM, WN, LP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_done = true;
  }
  conv_wgrad_h3_kernel<BM, BN, WM, WN, LP><<<grid, 256, lds, st>>>((const _Float16*)xh, (const _Float16*)xl, (const _Float16*)dyh,
                                                            (const _Float16*)dyl, sx, sdy, (const int4v*)table, wsf, w, x_bytes, dy_bytes);
}
// THE choice of the weight-gradient kernel: the persistent LDS-DMA kernels for everything they take (WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV = never),
// the register-staged kernels below otherwise. wgrad_h3_partials launches what this says and wdno_conv_wgrad_plan() reports it (reduce_tiled is
// filled there: it depends on the parameter's extents).
static int wgrad_h3_choose(const wdno_conv_geom* g, WgradHP& w, wdno_wgrad_plan& pl) {
  wgrad_h3_plan(w, g);
  pl.reduce_tiled = 0;
  if (wdno_debug_mode != WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV) {
    int rc = wdno_wgrad_h3d_describe(g, &pl);
    if (rc != WDNO_EUNSUPPORTED) return rc;
  }
  if (w.splits > 65535) return WDNO_EUNSUPPORTED;
  pl.family = WDNO_WGRAD_REG_H3;
  pl.bm = g->K > 64 ? 128 : 64;
  pl.bn = w.bn;
  pl.splits = w.splits; pl.pix_per_split = (int)w.pix_per_split; pl.splitpair = 0;
  pl.items = w.tiles_k * g->kd * g->kh * w.tiles_r;
  pl.grid = pl.items;
  return WDNO_OK;
}
// Runs the weight-gradient kernels; the per-split partial results go to `ws` ([splits][ntap][K][R]; with one split `single`
// may name the final packed destination instead). Returns the split count through *splits_out.
static int wgrad_h3_partials(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                             const void* pixel_table, float* single, void* ws, size_t ws_bytes, const wdno_conv_geom* g, hipStream_t st,
                             int* splits_out) {
  int rc = check_geom(g);
  if (rc) return rc;
  if ((g->C & 7) || (g->K & 7) || !pixel_table) return WDNO_EUNSUPPORTED;
  if ((int64_t)g->N * g->D * g->H * g->W * g->C * 2 >= CV_OOB || (int64_t)g->N * g->YD * g->YH * g->YW * g->K * 2 >= CV_OOB)
    return WDNO_EUNSUPPORTED;        // 32-bit buffer offsets
  WgradHP w;
  wdno_wgrad_plan pl;
  rc = wgrad_h3_choose(g, w, pl);
  if (rc) return rc;
  if (pl.family != WDNO_WGRAD_REG_H3) {
    const int splits = pl.splits;
    size_t need_d = (size_t)splits * g->kd * g->kh * (size_t)g->K * w.c.R * sizeof(float);
    float* dst = (splits == 1 && single) ? single : (float*)ws;
    if (dst == (float*)ws && ws_bytes < need_d) return WDNO_EWORKSPACE;
    rc = wdno_conv_wgrad_h3_dma(xh, xl, dyh, dyl, sx, sdy, pixel_table, dst, g, st);
    if (rc == WDNO_OK) *splits_out = splits;
    return rc;
  }
  size_t need = (size_t)w.splits * g->kd * g->kh * (size_t)g->K * w.c.R * sizeof(float);
  float* wsf = (w.splits == 1 && single) ? single : (float*)ws;
  if (wsf == (float*)ws && ws_bytes < need) return WDNO_EWORKSPACE;
  if (w.splits > 65535) return WDNO_EUNSUPPORTED;
  dim3 grid((unsigned)(w.tiles_k * g->kd * g->kh * w.tiles_r), (unsigned)w.splits);
  if (xl == nullptr) {          // single bf16 plane per operand
    if (pl.bm == 128) launch_wgrad_h3<128, 192, 2, 2, true>(xh, xh, dyh, dyh, sx, sdy, pixel_table, wsf, w, grid, st);
    else if (w.bn == 192) launch_wgrad_h3<64, 192, 2, 2, true>(xh, xh, dyh, dyh, sx, sdy, pixel_table, wsf, w, grid, st);
    else launch_wgrad_h3<64, 128, 1, 4, true>(xh, xh, dyh, dyh, sx, sdy, pixel_table, wsf, w, grid, st);
  } else if (pl.bm == 128) launch_wgrad_h3<128, 192, 2, 2, false>(xh, xl, dyh, dyl, sx, sdy, pixel_table, wsf, w, grid, st);
  else if (w.bn == 192) launch_wgrad_h3<64, 192, 2, 2, false>(xh, xl, dyh, dyl, sx, sdy, pixel_table, wsf, w, grid, st);
  else launch_wgrad_h3<64, 128, 1, 4, false>(xh, xl, dyh, dyl, sx, sdy, pixel_table, wsf, w, grid, st);
  *splits_out = w.splits;
  return WDNO_OK;
}
extern "C" int wdno_conv_wgrad_f16x3(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                                     const void* pixel_table, float* dwp, void* ws, size_t ws_bytes, const wdno_conv_geom* g, wdno_stream_t s) {
  hipStream_t st = as_stream(s);
  int splits = 0;
  int rc = wgrad_h3_partials(xh, xl, sx, dyh, dyl, sdy, pixel_table, dwp, ws, ws_bytes, g, st, &splits);
  if (rc) return rc;
  if (splits > 1) {
    int64_t n = (int64_t)g->kd * g->kh * g->K * (int64_t)g->kw * g->C;
    wgrad_h3_reduce_kernel<<<stream_grid(n / 4 + 1, 256), 256, 0, st>>>((const float*)ws, dwp, n, splits);
  }
  return wdno_check_launch();
}
// Same, but the gradient is delivered in the layout of the parameter, dw[Kn][Cn][kd][kh][kw] (Kn <= g->K, Cn <= g->C: the
// channel padding is dropped), by the split reduction itself -- no packed intermediate, no permute / slice copy afterwards.
// A block = 32 groups of four consecutive elements x 8 slices of the split list: with ~56 splits of a few hundred KB each, one
// thread per element walking all splits is a chain of 14 dependent loads on a few hundred blocks (14.5 us per launch, 72
// launches per train step); here a thread adds 7 float4 and the eight slices meet in LDS.
// (bid of nb blocks: the kernel's own grid, or the blocks one item owns inside a multi-tensor launch)
__device__ __forceinline__ void wgrad_h3_reduce_nat_body(const float* __restrict__ ws, float* __restrict__ dw, int64_t n, int splits,
                                                         int K8, int C8, int kw, int ntap, int Kn, int Cn, float4 (*part)[33], int bid, int nb) {
  const int R = kw * C8;
  const int j = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int64_t n4 = n >> 2;
  for (int64_t i4 = (int64_t)bid * 32 + j; i4 - j < n4; i4 += (int64_t)nb * 32) {      // block-uniform trip count
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (i4 < n4) {
      const float4* src = reinterpret_cast<const float4*>(ws) + i4;
      int sidx = q;
      for (; sidx + 8 < splits; sidx += 16) {
        const float4 u = src[(int64_t)sidx * n4], v = src[(int64_t)(sidx + 8) * n4];
        a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
        b.x += v.x; b.y += v.y; b.z += v.z; b.w += v.w;
      }
      if (sidx < splits) {
        const float4 u = src[(int64_t)sidx * n4];
        a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
      }
    }
    part[q][j] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    __syncthreads();
    // thread (q, j), q < 4: component q of group j
    if (q < 4 && i4 < n4) {
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float4 v = part[g][j];
        t += q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
      }
      const int64_t i = i4 * 4 + q;
      const int r = (int)(i % R);
      int64_t tt = i / R;
      const int k = (int)(tt % K8);
      const int tap = (int)(tt / K8);
      const int dx = r / C8, c = r - dx * C8;
      if (k < Kn && c < Cn) dw[(((int64_t)k * Cn + c) * ntap + tap) * kw + dx] = t;
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void wgrad_h3_reduce_nat_kernel(const float* __restrict__ ws, float* __restrict__ dw, int64_t n, int splits,
                                                                   int K8, int C8, int kw, int ntap, int Kn, int Cn) {
  __shared__ float4 part[8][33];
  wgrad_h3_reduce_nat_body(ws, dw, n, splits, K8, C8, kw, ntap, Kn, Cn, part, (int)blockIdx.x, (int)gridDim.x);
}
// The same reduction with coalesced stores. Above, consecutive threads hold consecutive (dx, c) of one (tap row, k) and scatter them
// ntap * kw floats apart in the parameter layout [K][C][taps]. Here a block owns one k and 64 input channels: it reads its T = ntap * kw
// segments of 64 contiguous floats per split (one wave per segment, lane = channel), sums the splits in order, turns the [T][64] tile
// through LDS and writes 64 * T contiguous floats of dw. T <= 64 (everything but the 7 x 7 x 7 stem).
__device__ __forceinline__ void wgrad_h3_reduce_tile_body(const float* __restrict__ ws, float* __restrict__ dw, int64_t n, int splits,
                                                          int K8, int C8, int kw, int ntap, int Kn, int Cn, float (*tile)[65], int bx, int by) {
  const int T = ntap * kw, R = kw * C8;
  const int k = by, c0 = bx * 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int sgm = wave; sgm < T; sgm += 4) {
    const int t = sgm / kw, dx = sgm - t * kw;
    float a = 0.f, b = 0.f;
    if (c0 + lane < C8) {
      const float* src = ws + ((int64_t)t * K8 + k) * R + dx * C8 + c0 + lane;
      int sp = 0;
      for (; sp + 1 < splits; sp += 2) { a += src[(int64_t)sp * n]; b += src[(int64_t)(sp + 1) * n]; }
      if (sp < splits) a += src[(int64_t)sp * n];
    }
    tile[lane][sgm] = a + b;
  }
  __syncthreads();
  const int cn = min(64, Cn - c0);                    // channels of this tile that exist in the parameter
  float* out = dw + ((int64_t)k * Cn + c0) * T;
  for (int e = threadIdx.x; e < cn * T; e += 256) {
    const int c = e / T, sgm = e - c * T;
    out[e] = tile[c][sgm];
  }
}
__global__ __launch_bounds__(256) void wgrad_h3_reduce_tile_kernel(const float* __restrict__ ws, float* __restrict__ dw, int64_t n, int splits,
                                                                    int K8, int C8, int kw, int ntap, int Kn, int Cn) {
  __shared__ float tile[64][65];
  wgrad_h3_reduce_tile_body(ws, dw, n, splits, K8, C8, kw, ntap, Kn, Cn, tile, (int)blockIdx.x, (int)blockIdx.y);
}
// which of the two reductions a layer takes, and with how many blocks (shared by the per-layer launch and the multi-tensor one)
static bool wgrad_h3_reduce_tiled(int splits, const wdno_conv_geom* g, int Kn, int Cn) {
  const int T = g->kd * g->kh * g->kw;
  const bool big = (int64_t)Kn * cdiv(Cn, 64) >= 512 && splits <= 8;
  return T <= 64 && (splits <= 2 || big);
}
extern "C" int wdno_conv_wgrad_plan(const wdno_conv_geom* g, int lowp, int Kn, int Cn, wdno_wgrad_plan* out) {
  (void)lowp;                // (both plane forms share one plan)
  WDNO_REQUIRE(out);
  int rc = check_geom(g);
  if (rc) return rc;
  if ((g->C & 7) || (g->K & 7)) return WDNO_EUNSUPPORTED;
  WgradHP w;
  rc = wgrad_h3_choose(g, w, *out);
  if (rc) return rc;
  out->reduce_tiled = wgrad_h3_reduce_tiled(out->splits, g, Kn > 0 ? Kn : g->K, Cn > 0 ? Cn : g->C) ? 1 : 0;
  return WDNO_OK;
}

// ---- every pending split reduction of a backward pass in ONE launch (round 6). A training step ran 58 of these reductions, 5-10 us each, one behind
// every weight-gradient kernel (0.43 ms per smoke step, profiles/r05_smoke_kernel_stats.md); only the optimiser reads their results. The callers
// now run the partial-sum kernels alone (wdno_conv_wgrad_*_partials: the workspace stays alive) and hand the list of reductions over at the end of
// the backward: the items travel BY VALUE in the kernel arguments (<= WDNO_WGRAD_REDUCE_MAX per launch: 2.4 KB of arguments, well inside the 4 KB a launch takes together with the implicit ones), so the launch needs no table upload and
// replays unchanged from a captured graph. A block finds its item by its first-block number and runs the same body as the per-layer kernels in
// the same order of additions: results are bit-identical to them.
struct WgradReduceArgs {
  wdno_wgrad_reduce_item it[WDNO_WGRAD_REDUCE_MAX];
  int first[WDNO_WGRAD_REDUCE_MAX + 1];          // first block of item i; first[n] = grid
  int n;
};
__global__ __launch_bounds__(256) void wgrad_h3_reduce_multi_kernel(const WgradReduceArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[64 * 65];                // tile[64][65] of the tiled body / part[8][33] float4 of the scatter body
  int lo = 0, hi = a.n - 1;                      // last item whose first block is <= blockIdx.x (block-uniform: scalar loads of the arguments)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const wdno_wgrad_reduce_item& w = a.it[lo];
  const int bid = (int)blockIdx.x - a.first[lo], nb = a.first[lo + 1] - a.first[lo];
  if (w.tiled) {
    const int bxn = (w.Cn + 63) >> 6;
    wgrad_h3_reduce_tile_body(w.ws, w.dw, w.n, w.splits, w.K8, w.C8, w.kw, w.ntap, w.Kn, w.Cn, reinterpret_cast<float (*)[65]>(smem), bid % bxn, bid / bxn);
  } else {
    wgrad_h3_reduce_nat_body(w.ws, w.dw, w.n, w.splits, w.K8, w.C8, w.kw, w.ntap, w.Kn, w.Cn, reinterpret_cast<float4 (*)[33]>(smem), bid, nb);
  }
}
extern "C" int wdno_wgrad_reduce_multi(const wdno_wgrad_reduce_item* items, int n_items, wdno_stream_t s) {
  WDNO_REQUIRE(items && n_items >= 0);
  hipStream_t st = as_stream(s);
  for (int base = 0; base < n_items; base += WDNO_WGRAD_REDUCE_MAX) {
    WgradReduceArgs a;
    a.n = n_items - base < WDNO_WGRAD_REDUCE_MAX ? n_items - base : WDNO_WGRAD_REDUCE_MAX;
    int grid = 0;
    for (int i = 0; i < a.n; ++i) {
      a.it[i] = items[base + i];
      const wdno_wgrad_reduce_item& w = a.it[i];
      WDNO_REQUIRE(w.ws && w.dw && w.n > 0 && w.splits >= 1 && w.Kn > 0 && w.Cn > 0 && w.Kn <= w.K8 && w.Cn <= w.C8);
      a.first[i] = grid;
      grid += w.tiled ? cdiv(w.Cn, 64) * w.Kn : stream_grid(w.n / 4, 32);      // the per-layer launches' grids
    }
    a.first[a.n] = grid;
    if (grid > 0) wgrad_h3_reduce_multi_kernel<<<grid, 256, 0, st>>>(a);
  }
  return wdno_check_launch();
}

static void wgrad_h3_reduce_launch(const float* ws, float* dw, int64_t n, int splits, const wdno_conv_geom* g, int Kn, int Cn, hipStream_t st) {
  // (layers with many splits are the small ones: K * C / 64 blocks that each walk T x splits segments are too few and too serial there --
  // 64 -> 64 channels with 18 splits took 2x the scatter kernel's time, +1.1 ms per smoke step when used everywhere)
  // ... but a layer with >= 512 (k, 64-channel) blocks and a handful of splits (256 -> 256 at level 2: 1024 blocks, 3 splits) has enough of them, and
  // the scatter kernel's 4-byte stores 27 floats apart are what it pays for (31-33 us per launch, 7 launches per smoke step)
  if (wgrad_h3_reduce_tiled(splits, g, Kn, Cn)) {
    wgrad_h3_reduce_tile_kernel<<<dim3(cdiv(Cn, 64), Kn), 256, 0, st>>>(ws, dw, n, splits, g->K, g->C, g->kw, g->kd * g->kh, Kn, Cn);
    return;
  }
  wgrad_h3_reduce_nat_kernel<<<stream_grid(n / 4, 32), 256, 0, st>>>(ws, dw, n, splits, g->K, g->C, g->kw, g->kd * g->kh, Kn, Cn);
}
extern "C" int wdno_conv_wgrad_f16x3_param(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                                           const void* pixel_table, float* dw, int Kn, int Cn, void* ws, size_t ws_bytes,
                                           const wdno_conv_geom* g, wdno_stream_t s) {
  WDNO_REQUIRE(g && Kn > 0 && Cn > 0 && Kn <= g->K && Cn <= g->C);
  hipStream_t st = as_stream(s);
  int splits = 0;
  int rc = wgrad_h3_partials(xh, xl, sx, dyh, dyl, sdy, pixel_table, nullptr, ws, ws_bytes, g, st, &splits);
  if (rc) return rc;
  const int64_t n = (int64_t)g->kd * g->kh * g->K * (int64_t)g->kw * g->C;
  wgrad_h3_reduce_launch((const float*)ws, dw, n, splits, g, Kn, Cn, st);
  return wdno_check_launch();
}

// The partial-sum kernels alone: `item` comes back filled for wdno_wgrad_reduce_multi (ws must stay alive and unmodified until that launch).
extern "C" int wdno_conv_wgrad_partials(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                                        const void* pixel_table, float* dw, int Kn, int Cn, void* ws, size_t ws_bytes,
                                        const wdno_conv_geom* g, wdno_wgrad_reduce_item* item, wdno_stream_t s) {
  WDNO_REQUIRE(g && item && dw && Kn > 0 && Cn > 0 && Kn <= g->K && Cn <= g->C);
  int splits = 0;
  int rc = wgrad_h3_partials(xh, xl, sx, dyh, dyl, sdy, pixel_table, nullptr, ws, ws_bytes, g, as_stream(s), &splits);      // xl == NULL: one bf16 plane per operand
  if (rc) return rc;
  const int64_t n = (int64_t)g->kd * g->kh * g->K * (int64_t)g->kw * g->C;
  if (n >= 0x7fffffff) return WDNO_EUNSUPPORTED;
  item->ws = (const float*)ws; item->dw = dw; item->n = (int)n; item->splits = splits; item->K8 = g->K; item->C8 = g->C; item->kw = g->kw;
  item->ntap = g->kd * g->kh; item->Kn = Kn; item->Cn = Cn; item->tiled = wgrad_h3_reduce_tiled(splits, g, Kn, Cn) ? 1 : 0;
  return wdno_check_launch();
}

extern "C" int wdno_conv_wgrad_bf16_param(const void* x16, const void* dy16, const void* pixel_table, float* dw, int Kn, int Cn, void* ws,
                                          size_t ws_bytes, const wdno_conv_geom* g, wdno_stream_t s) {
  WDNO_REQUIRE(g && Kn > 0 && Cn > 0 && Kn <= g->K && Cn <= g->C);
  hipStream_t st = as_stream(s);
  int splits = 0;
  int rc = wgrad_h3_partials(x16, nullptr, nullptr, dy16, nullptr, nullptr, pixel_table, nullptr, ws, ws_bytes, g, st, &splits);
  if (rc) return rc;
  const int64_t n = (int64_t)g->kd * g->kh * g->K * (int64_t)g->kw * g->C;
  wgrad_h3_reduce_launch((const float*)ws, dw, n, splits, g, Kn, Cn, st);
  return wdno_check_launch();
}
