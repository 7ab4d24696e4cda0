// dwt.hip -- single-level separable wavelet filter banks on gfx950 (HBM-bound stencil passes).
//
// Every transform on the WDNO path is a tensor product of two 1-axis primitives:
//   analysis : y_b[k] = sum_m f_b[L-1-m] * X(2k + m - off)            (b = lo, hi; stride-2 correlation)
//   synthesis: x[n]   = sum_{m : (n+off-m) even} lo[K] g_lo[m] + hi[K] g_hi[m],  K = (n+off-m)/2
// with off = L-2 and zero extension (mode 'zero'), or off = L/2-1 and periodic extension (mode
// 'periodization', odd lengths extended by repeating the last sample). The adjoints needed for guidance
// back-propagation are the same two primitives with reversed taps.
//
// One launch per axis; the band index and the (possibly padded) coefficient packing of coef_to_tensor are
// folded into the store/load addressing of the pass that touches the coefficient tensor, so no separate
// packing kernel exists. Taps travel as kernel arguments (<= 16 per filter).
//
// This unit holds the per-axis kernels, the choice between them and the fused single-launch transforms (fused_try), and the entry points;
// the fused kernels are dwt_analysis.hip and dwt_synthesis.hip, the steps they share dwt_tiles.h.
#include "dwt_tiles.h"
#include <cstdlib>

#define WDNO_MAXCOMP 5

// mixed-radix outer index -> two linear addresses
struct OuterMap {
  int ncomp;
  int n[WDNO_MAXCOMP];
  int64_t sa[WDNO_MAXCOMP];  // strides on the "signal side" tensor
  int64_t sc[WDNO_MAXCOMP];  // strides on the "coefficient side" tensor
};

struct AxisPass {
  OuterMap om;
  int64_t outer;        // product of om.n
  int N;                // signal length along the axis (logical, before odd extension)
  int M;                // coefficient length along the axis
  int inner;            // contiguous trailing extent shared by both sides
  int64_t sig_stride;   // stride of the axis on the signal side (elements)
  int64_t coef_stride;  // stride of the axis on the coefficient side
  int64_t band_stride;  // stride between lo and hi on the coefficient side
  int mode, L, off;
  int odd;              // periodization with odd N: extended length N+1
};

__device__ __forceinline__ void outer_addr(const OuterMap& om, int64_t o, int64_t& a, int64_t& c) {
  a = 0; c = 0;
#pragma unroll
  for (int i = WDNO_MAXCOMP - 1; i >= 0; --i) {
    if (i < om.ncomp) {
      int64_t q = o / om.n[i];
      int r = (int)(o - q * om.n[i]);
      a += r * om.sa[i];
      c += r * om.sc[i];
      o = q;
    }
  }
}

// signal -> (lo, hi)
__global__ __launch_bounds__(256) void analysis_kernel(const float* __restrict__ sig, float* __restrict__ coef, AxisPass p, Taps t) {
  int64_t total = p.outer * p.M * p.inner;
  int64_t stride = (int64_t)gridDim.x * 256;
  int Next = p.N + p.odd;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    int i = (int)(idx % p.inner);
    int64_t r = idx / p.inner;
    int k = (int)(r % p.M);
    int64_t o = r / p.M;
    int64_t a, c;
    outer_addr(p.om, o, a, c);
    const float* sp = sig + a + i;
    float lo = 0.f, hi = 0.f;
    int j0 = 2 * k - p.off;
    for (int m = 0; m < p.L; ++m) {
      int j = j0 + m;
      float v;
      if (p.mode == 1) {
        v = (j >= 0 && j < p.N) ? sp[(int64_t)j * p.sig_stride] : 0.f;
      } else {
        j %= Next;
        if (j < 0) j += Next;
        if (j > p.N - 1) j = p.N - 1;
        v = sp[(int64_t)j * p.sig_stride];
      }
      lo = fmaf(t.lo[p.L - 1 - m], v, lo);
      hi = fmaf(t.hi[p.L - 1 - m], v, hi);
    }
    float* cp = coef + c + (int64_t)k * p.coef_stride + i;
    cp[0] = lo;
    cp[p.band_stride] = hi;
  }
}

// (lo, hi) -> signal. For the adjoint of a periodized analysis of odd length (odd = 1) the sample of the
// repeated position N is folded back onto N-1.
__device__ __forceinline__ float synth_point(const float* __restrict__ cp, const AxisPass& p, const Taps& t, int n) {
  float acc = 0.f;
  int base = n + p.off;
  int Next = p.N + p.odd;   // periodization period on the signal side
  for (int m = (base & 1); m < p.L; m += 2) {
    int kk = base - m;      // even
    if (p.mode == 1) {
      kk >>= 1;             // arithmetic shift; negative stays negative
      if (kk < 0 || kk >= p.M) continue;
    } else {
      kk %= Next;
      if (kk < 0) kk += Next;
      kk >>= 1;
    }
    const float* q = cp + (int64_t)kk * p.coef_stride;
    acc = fmaf(q[0], t.lo[m], acc);
    acc = fmaf(q[p.band_stride], t.hi[m], acc);
  }
  return acc;
}
__global__ __launch_bounds__(256) void synthesis_kernel(const float* __restrict__ coef, float* __restrict__ sig, AxisPass p, Taps t) {
  int64_t total = p.outer * p.N * p.inner;
  int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
    int i = (int)(idx % p.inner);
    int64_t r = idx / p.inner;
    int n = (int)(r % p.N);
    int64_t o = r / p.N;
    int64_t a, c;
    outer_addr(p.om, o, a, c);
    const float* cp = coef + c + i;
    float v = synth_point(cp, p, t, n);
    if (p.odd && n == p.N - 1) v += synth_point(cp, p, t, p.N);
    sig[a + (int64_t)n * p.sig_stride + i] = v;
  }
}

// LDS budget per block of the fused kernels (dwt_tiles.h)
size_t dwt_fused_lds_budget(long default_kb) {
  static long env_kb = -1;
  if (env_kb < 0) {
    const char* e = getenv("WDNO_DWT_LDS_KB");        // A/B switch (tools/bench_dwt.py)
    env_kb = e ? atol(e) : 0;
  }
  long kb = env_kb > 0 ? env_kb : default_kb;
  if (kb < 8) kb = 8;
  if (kb > 64) kb = 64;
  return (size_t)kb * 1024;
}

// true = the transform was launched as ONE fused kernel; false = not covered (1-D, long filters, rows that do not fit LDS, the
// odd-length synthesis-shaped adjoint), the caller falls back to the per-axis passes. With `plan` (wdno_dwt_plan_query) the same decision is
// only reported: the units' "decide" step runs, their "launch" step does not.
static bool fused_try(bool analysis_dir, const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, bool odd_rule, hipStream_t st,
                      const PackedStore* pk = nullptr, wdno_dwt_plan* plan = nullptr) {
  if ((wdno_debug_mode == WDNO_DBG_PER_AXIS_DWT_AND_WGRAD_WINDOW_K64 && !pk) || d->nd < 2) return false;
  if (!analysis_dir && d->mode == 0 && odd_rule)
    for (int a = 3 - d->nd; a < 3; ++a)
      if (d->in_dims[a] & 1) return false;
  if (!analysis_dir && d->mode == 0)
    for (int a = 3 - d->nd; a < 3; ++a)
      if (d->in_dims[a] != 2 * d->out_dims[a]) return false;
  return analysis_dir ? dwt_fused_analysis(src, dst, d, taps, odd_rule, st, pk, plan) : dwt_fused_synthesis(src, dst, d, taps, st, plan);
}

// ------------------------------------------------------------------------------------------------ host side
static int validate(const wdno_dwt_desc* d) {
  if (!d || d->nd < 1 || d->nd > 3 || (d->mode != 0 && d->mode != 1)) return WDNO_EINVAL;
  if (d->L < 2 || d->L > WDNO_MAXL || (d->L & 1) || d->n_img <= 0) return WDNO_EINVAL;
  for (int a = 3 - d->nd; a < 3; ++a) {
    int N = d->in_dims[a], M = d->out_dims[a];
    if (N <= 0 || M <= 0) return WDNO_EINVAL;
    if (d->mode == 0) {
      if (M != (N + 1) / 2 || N + (N & 1) < d->L) return WDNO_EUNSUPPORTED;
    }
    // mode zero: forward has M == (N+L-1)/2 ; inverse/adjoints may be called with the natural N = 2M-L+2
  }
  return WDNO_OK;
}

// What each entry point (WDNO_DWT_ENTRY_*) runs with -- the filter pair (decomposition or reconstruction), its tap order, the direction of the
// data and whether an odd periodized length follows the repeated-sample rule -- and what it asks of the descriptor beyond validate(): ONE
// table and ONE check, for the entry points and for wdno_dwt_plan_query.
//   inv_adjoint: d(coef) from d(x) for x = inv(coef): analysis-shaped with reversed reconstruction taps
//   fwd_adjoint: d(x) from d(coef) for coef = fwd(x): synthesis-shaped with reversed decomposition taps
struct EntrySpec { bool rec_taps, reverse_taps, analysis_dir, odd_rule; };
static const EntrySpec ENTRIES[5] = {
  {false, false, true, true},      // WDNO_DWT_ENTRY_FWD
  {true, false, false, false},     // WDNO_DWT_ENTRY_INV
  {true, true, true, false},       // WDNO_DWT_ENTRY_INV_ADJOINT
  {false, true, false, true},      // WDNO_DWT_ENTRY_FWD_ADJOINT
  {false, false, true, true},      // WDNO_DWT_ENTRY_FWD_PACKED
};
static int entry_check(const wdno_dwt_desc* d, int entry) {
  int rc = validate(d);
  if (rc) return rc;
  if (entry == WDNO_DWT_ENTRY_FWD_PACKED && (d->nd != 3 || d->mode != 1)) return WDNO_EUNSUPPORTED;
  for (int a = 3 - d->nd; a < 3; ++a) {
    if (entry == WDNO_DWT_ENTRY_INV || entry == WDNO_DWT_ENTRY_INV_ADJOINT) {
      int want = d->mode == 1 ? 2 * d->out_dims[a] - d->L + 2 : 2 * d->out_dims[a];
      if (d->in_dims[a] != want) return WDNO_EINVAL;   // the inverse always produces the natural (even) length
    } else if (d->mode == 1 && d->out_dims[a] != (d->in_dims[a] + d->L - 1) / 2) {
      return WDNO_EINVAL;
    }
  }
  return WDNO_OK;
}

// Intermediate layouts (forward order T, H, W; nb = number of bands produced so far):
//   after pass T : [img][bt][To][H][W]
//   after pass H : [img][bt][To][bh][Ho][W]
//   after pass W : the coefficient tensor (strided), band = bt*4 + bh*2 + bw (missing axes contribute 0 bits)
static size_t ws_elems(const wdno_dwt_desc* d) {
  int T = d->in_dims[0], H = d->in_dims[1], W = d->in_dims[2];
  int To = d->out_dims[0], Ho = d->out_dims[1];
  if (d->nd == 1) return 0;
  if (d->nd == 2) return (size_t)d->n_img * 2 * Ho * W;
  size_t t1 = (size_t)d->n_img * 2 * To * H * W;
  size_t t2 = (size_t)d->n_img * 2 * To * 2 * Ho * W;
  return t1 + t2;
}
extern "C" size_t wdno_dwt_ws_bytes(const wdno_dwt_desc* d) {
  if (validate(d) != WDNO_OK) return 0;
  return ws_elems(d) * sizeof(float) + 256;
}

static void fill_taps(Taps& t, const float* lo, const float* hi, int L, bool reverse) {
  for (int i = 0; i < WDNO_MAXL; ++i) { t.lo[i] = 0.f; t.hi[i] = 0.f; }
  for (int i = 0; i < L; ++i) {
    t.lo[i] = reverse ? lo[L - 1 - i] : lo[i];
    t.hi[i] = reverse ? hi[L - 1 - i] : hi[i];
  }
}

static void set_outer(OuterMap& om, int ncomp, const int* n, const int64_t* sa, const int64_t* sc, int64_t& outer) {
  om.ncomp = ncomp;
  outer = 1;
  for (int i = 0; i < WDNO_MAXCOMP; ++i) {
    om.n[i] = i < ncomp ? n[i] : 1;
    om.sa[i] = i < ncomp ? sa[i] : 0;
    om.sc[i] = i < ncomp ? sc[i] : 0;
    if (i < ncomp) outer *= n[i];
  }
}

// Build the pass descriptors shared by all four entry points. `analysis_dir`: true when data flows
// signal -> coefficients (dwt_fwd, dwt_inv_adjoint), false for the reverse direction.
// sig = the signal-side tensor of the whole transform, coef = the packed coefficient tensor.
static int run(const float* src, float* dst, const wdno_dwt_desc* d, int entry, const float* f, void* ws, size_t ws_bytes, hipStream_t st) {
  int rc = entry_check(d, entry);
  if (rc) return rc;
  const EntrySpec& e = ENTRIES[entry];
  const bool analysis_dir = e.analysis_dir, odd_rule = e.odd_rule;
  const float* fl = f + (e.rec_taps ? 2 * d->L : 0);
  Taps taps;
  fill_taps(taps, fl, fl + d->L, d->L, e.reverse_taps);
  if (fused_try(analysis_dir, src, dst, d, taps, odd_rule, st)) return wdno_check_launch();
  if (ws_elems(d) * sizeof(float) > ws_bytes) return WDNO_EWORKSPACE;
  const int T = d->in_dims[0], H = d->in_dims[1], W = d->in_dims[2];
  const int To = d->out_dims[0], Ho = d->out_dims[1], Wo = d->out_dims[2];
  const int img = d->n_img;
  const int off = d->mode == 1 ? d->L - 2 : d->L / 2 - 1;
  float* t1 = (float*)ws;                                   // [img][2][To][H][W]      (nd == 3)
  float* t2 = d->nd == 3 ? t1 + (size_t)img * 2 * To * H * W : t1;  // [img][bt][To][2][Ho][W]
  auto base = [&](int N, int M) {
    AxisPass p;
    p.N = N; p.M = M; p.mode = d->mode; p.L = d->L; p.off = off;
    p.odd = (d->mode == 0 && odd_rule && (N & 1)) ? 1 : 0;
    return p;
  };
  // contiguous signal strides
  const int64_t xs1 = W, xs0 = (int64_t)H * W, xsi = (int64_t)T * H * W;
  auto launch = [&](bool ana, const float* a_in, float* a_out, const AxisPass& p) {
    int64_t items = p.outer * (int64_t)(ana ? p.M : p.N) * p.inner;
    int grid = stream_grid(items, 256);
    if (ana) analysis_kernel<<<grid, 256, 0, st>>>(a_in, a_out, p, taps);
    else synthesis_kernel<<<grid, 256, 0, st>>>(a_in, a_out, p, taps);
  };

  // --- describe the three possible passes; "signal side" (sa) is the input of the analysis direction
  AxisPass pT, pH, pW;
  bool hasT = d->nd == 3, hasH = d->nd >= 2;
  if (hasT) {  // signal [img][T][H*W] <-> t1 [img][2][To][H*W]
    pT = base(T, To);
    int n[1] = {img};
    int64_t sa[1] = {xsi};
    int64_t sc[1] = {(int64_t)2 * To * H * W};
    set_outer(pT.om, 1, n, sa, sc, pT.outer);
    pT.inner = H * W; pT.sig_stride = xs0; pT.coef_stride = (int64_t)H * W; pT.band_stride = (int64_t)To * H * W;
  }
  const int nbt = hasT ? 2 : 1;            // bands already present before the H pass
  const int Tcur = hasT ? To : 1;
  if (hasH) {  // signal-side [img*nbt*Tcur][H][W] <-> t2 [img*nbt*Tcur][2][Ho][W]
    pH = base(H, Ho);
    int n[1] = {img * nbt * Tcur};
    int64_t sa[1] = {(int64_t)H * W};
    int64_t sc[1] = {(int64_t)2 * Ho * W};
    set_outer(pH.om, 1, n, sa, sc, pH.outer);
    pH.inner = W; pH.sig_stride = W; pH.coef_stride = W; pH.band_stride = (int64_t)Ho * W;
  }
  {  // W pass: signal-side rows (img, bt, to, bh, ho) of length W  <->  packed coefficient tensor
    pW = base(W, Wo);
    const int nbh = hasH ? 2 : 1;
    const int Hcur = hasH ? Ho : 1;
    int n[5] = {img, nbt, Tcur, nbh, Hcur};
    // signal side = t2 layout [img][bt][To][bh][Ho][W] (or the raw signal when nd == 1)
    int64_t sa[5] = {(int64_t)nbt * Tcur * nbh * Hcur * W, (int64_t)Tcur * nbh * Hcur * W, (int64_t)nbh * Hcur * W, (int64_t)Hcur * W, (int64_t)W};
    // band index: 3-D = bt*4 + bh*2 + bw ('aaa'..'ddd'); 2-D = bw*2 + bh (pywt dwt2 order LL,'da','ad','dd'); 1-D = bw
    const int64_t bsH = (d->nd == 2) ? d->cs_band : 2 * d->cs_band;
    const int64_t bsW = (d->nd == 2) ? 2 * d->cs_band : d->cs_band;
    int64_t sc[5] = {d->cs_img, 4 * d->cs_band, d->cs0, bsH, d->cs1};
    if (!hasT) { sc[1] = 0; sc[2] = 0; }
    if (!hasH) { sc[3] = 0; sc[4] = 0; }
    set_outer(pW.om, 5, n, sa, sc, pW.outer);
    pW.inner = 1; pW.sig_stride = 1; pW.coef_stride = 1; pW.band_stride = bsW;
  }

  if (analysis_dir) {
    const float* cur = src;
    if (hasT) { launch(true, cur, t1, pT); cur = t1; }
    if (hasH) { launch(true, cur, t2, pH); cur = t2; }
    launch(true, cur, dst, pW);
  } else {
    // coefficients -> signal: W, then H, then T
    float* wout = hasH ? t2 : dst;
    launch(false, src, wout, pW);
    if (hasH) {
      float* hout = hasT ? t1 : dst;
      launch(false, t2, hout, pH);
      if (hasT) launch(false, t1, dst, pT);
    }
  }
  return wdno_check_launch();
}

extern "C" int wdno_dwt_fwd(const float* x, float* coef, const wdno_dwt_desc* d, const float* f, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return run(x, coef, d, WDNO_DWT_ENTRY_FWD, f, ws, ws_bytes, as_stream(s));
}
// Analysis with the coefficients stored straight into a larger, differently ordered tensor and divided by a per-channel constant: image
// i = (outer, inner) = (i / img_inner, i % img_inner) writes at outer * cs_outer + inner * d->cs_img (+ band * cs_band + k0 * cs0 + k1 * cs1 + k2),
// value / rescaler[inner * 8 + band] (IEEE division); rows are written row_w (>= the coefficient count, % 4 == 0) columns wide, 0 / rescaler beyond
// the coefficients (whole 16-byte stores: strides and `state` 16-byte aligned). The smoke task's state [B][pad_t][8 F + 2][pad_x][pad_x] takes the F fields of a sample
// with cs_outer = pad_t C pad_x^2, cs_img = 8 pad_x^2, cs_band = pad_x^2, cs0 = C pad_x^2, cs1 = pad_x (data_2d.py:156-221: cat, pad, permute,
// / RESCALER -- the padding and the two condition channels are wdno_pack_smoke_fill's). ONE fused launch, 3-D zero mode only: anything the fused
// kernel does not take is WDNO_EUNSUPPORTED (the caller then transforms into a coefficient tensor and packs, wdno_pack_smoke_fields).
extern "C" int wdno_dwt_fwd_packed(const float* x, float* state, const wdno_dwt_desc* d, const float* f, int img_inner, int64_t cs_outer, int row_w,
                                   const float* rescaler, wdno_stream_t s) {
  if (!d) return WDNO_EINVAL;
  WDNO_REQUIRE(x && state && f && rescaler && img_inner > 0 && d->n_img % img_inner == 0);
  int rc = entry_check(d, WDNO_DWT_ENTRY_FWD_PACKED);            // validate() and what this entry asks beyond it
  if (rc) return rc;
  const EntrySpec& e = ENTRIES[WDNO_DWT_ENTRY_FWD_PACKED];
  Taps taps;
  fill_taps(taps, f, f + d->L, d->L, e.reverse_taps);
  PackedStore ps = {img_inner, row_w, cs_outer, rescaler};
  if (!fused_try(e.analysis_dir, x, state, d, taps, e.odd_rule, as_stream(s), &ps)) return WDNO_EUNSUPPORTED;
  return wdno_check_launch();
}
extern "C" int wdno_dwt_inv(const float* coef, float* x, const wdno_dwt_desc* d, const float* f, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return run(coef, x, d, WDNO_DWT_ENTRY_INV, f, ws, ws_bytes, as_stream(s));
}
extern "C" int wdno_dwt_inv_adjoint(const float* dx, float* dcoef, const wdno_dwt_desc* d, const float* f, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return run(dx, dcoef, d, WDNO_DWT_ENTRY_INV_ADJOINT, f, ws, ws_bytes, as_stream(s));
}
extern "C" int wdno_dwt_fwd_adjoint(const float* dcoef, float* dx, const wdno_dwt_desc* d, const float* f, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return run(dcoef, dx, d, WDNO_DWT_ENTRY_FWD_ADJOINT, f, ws, ws_bytes, as_stream(s));
}
// What the entry point would launch (include/wdno_hip.h): entry_check and fused_try as the entry points call them, with `plan` set
extern "C" int wdno_dwt_plan_query(const wdno_dwt_desc* d, int entry, wdno_dwt_plan* out) {
  if (!out || entry < WDNO_DWT_ENTRY_FWD || entry > WDNO_DWT_ENTRY_FWD_PACKED) return WDNO_EINVAL;
  *out = wdno_dwt_plan{-1, 0, 0, 0, 0, 0, 0, WDNO_OK};
  if ((out->rc = entry_check(d, entry))) return WDNO_OK;
  const EntrySpec& e = ENTRIES[entry];
  Taps taps = {};
  const bool packed = entry == WDNO_DWT_ENTRY_FWD_PACKED;
  PackedStore ps = {1, (d->out_dims[2] + 3) & ~3, 0, nullptr};
  wdno_dwt_plan pl;
  if (fused_try(e.analysis_dir, nullptr, nullptr, d, taps, e.odd_rule, nullptr, packed ? &ps : nullptr, &pl)) *out = pl;
  else if (packed) out->rc = WDNO_EUNSUPPORTED;
  else out->family = WDNO_DWT_PER_AXIS;
  return WDNO_OK;
}
