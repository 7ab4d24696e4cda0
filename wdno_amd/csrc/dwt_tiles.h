// dwt_tiles.h -- what the fused wavelet kernels share, each step written once (prefix dw_): dwt_analysis_fused_kernel (dwt_analysis.hip) and
// dwt_synthesis_fused_kernel, dwt_synthesis2_kernel, dwt_synthesis3_stream_kernel (dwt_synthesis.hip). The per-axis kernels of dwt.hip are the
// reference all of them are compared against bit for bit (tests/test_gpu_dwt_fused.py) and use nothing from here but Taps. Every function is
// __forceinline__ and replaces an inline site only where the kernel compiles to the same code (profiles/dwt_tiles_header.md); a site that
// did not come out that way keeps its inline form and says so. The LDS layout of a kernel is ONE function that its chooser calls to size
// the launch and the kernel calls to carve lds[].
//
// One launch per 2-D / 3-D transform, no workspace round trip ("fuse all axes in LDS").
// A block owns a tile of coefficients (analysis) / signal samples (synthesis) of one image and runs the per-axis passes back to
// back: the pass along the SLOWEST transformed axis lives in registers (it needs no neighbours across lanes: a thread owns one
// column, its loads / stores are coalesced over the contiguous axis and touch global memory), the other passes go through LDS.
//     analysis : global --T (regs)--> S1 --H--> S2 --W--> packed coefficients          (2-D: global --H (regs)--> S2 --W--> coef)
//     synthesis: packed coefficients --W--> S1 --H--> S2 --T (regs)--> global          (2-D: coef --W--> S1 --H (regs)--> global)
// Boundary rules (zero extension / periodization / repeated last sample of an odd length) are applied where a pass reads its
// operand from global memory, so the LDS passes are unconditional. Pass order and the order of every fmaf chain are those of the
// per-axis kernels of dwt.hip, hence the results are BIT-IDENTICAL to them (tests compare with torch.equal).
// Halo rows/frames of neighbouring tiles are re-read through L2: logical tile ids are laid out so that one XCD (= one L2) owns a
// contiguous range of tiles, i.e. whole images.
#pragma once
#include "common.h"
#include "debug_modes.h"
#include "fastdiv.h"

#define WDNO_MAXL 16

struct Taps { float lo[WDNO_MAXL]; float hi[WDNO_MAXL]; };

struct FusedGeom {
  FastDiv dFW, dNH, dWo, dQW, dEH, dNQH2, dRW, dQW4;      // (dRW, dQW4: the staged W pass of the 2-D synthesis)
  int n_img, T, H, W, To, Ho, Wo;
  int64_t cs_img, cs_band, cs0, cs1;
  int off, odd_t, odd_h, odd_w;
  int NH;                 // analysis: coefficient rows per tile; synthesis: q rows per tile (q = (n + off) >> 1)
  int tiles_t, tiles_h, n_blocks;
  int FW;                 // analysis: columns incl. boundary extension (2 Wo + L - 2); synthesis: 2 * QW
  int qt0, qh0, qw0;      // synthesis: first q along each axis (off >> 1)
  int QH, QT;             // synthesis: number of q rows / frames in total
  int debug;              // tools only: 12 / 13 / 14 skip the W / H / T pass of the synthesis kernel (timing breakdown, wrong results)
  // PACKED analysis (wdno_dwt_fwd_packed): image = (outer, inner) = (img / img_inner, img % img_inner), coefficient base = outer * cs_outer +
  // inner * cs_img, every coefficient divided (IEEE) by resc[inner * 2^ND + band] on its way out
  // Rows are written in full: row_w (a multiple of 4, >= Wo) columns, zeros (/ resc) beyond the coefficients, as aligned 16-byte stores.
  FastDiv dInner;
  int img_inner, row_w;
  int64_t cs_outer;
  const float* resc;
};

struct PackedStore { int img_inner, row_w; int64_t cs_outer; const float* resc; };     // wdno_dwt_fwd_packed

// What a chooser decided: the kernel (WDNO_DWT_* of wdno_hip.h), its variant (PMAX of dwt_synthesis2_kernel, WMAX of the stream kernel, 0
// otherwise) and the dynamic LDS of the launch; the tile geometry is the FusedGeom next to it. Each unit has ONE "decide" function, which
// fills both and launches nothing, and one "launch" function, which only reads them.
struct FusedChoice { int family, variant; size_t lds; };
static inline void dw_plan_of(const FusedGeom& g, const FusedChoice& c, wdno_dwt_plan* out) {
  *out = wdno_dwt_plan{c.family, c.variant, g.NH, g.tiles_h, g.tiles_t, g.n_blocks, (int)c.lds, WDNO_OK};
}

// The two fused units, one entry each (fused_try of dwt.hip): true = the transform is covered by ONE fused kernel, false = not covered.
// plan == nullptr: decide and launch. plan != nullptr (wdno_dwt_plan_query): decide only -- *plan receives the decision, nothing is launched
// and src / dst are not touched.
bool dwt_fused_analysis(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, bool odd_rule, hipStream_t st, const PackedStore* pk,
                        wdno_dwt_plan* plan);
bool dwt_fused_synthesis(const float* src, float* dst, const wdno_dwt_desc* d, const Taps& taps, hipStream_t st, wdno_dwt_plan* plan);
// LDS budget per block (dwt.hip; <= 64 KB: the default dynamic-LDS limit, no function attribute needed -> graph-capture safe). Smaller
// tiles = more blocks per CU to hide the latency of the global reads, at the price of more halo re-reads through L2.
size_t dwt_fused_lds_budget(long default_kb);

// the part of the geometry both choosers fill alike
static inline FusedGeom dw_geom(const wdno_dwt_desc* d, int L, int mode) {
  FusedGeom g = {};
  g.n_img = d->n_img;
  g.T = d->in_dims[0]; g.H = d->in_dims[1]; g.W = d->in_dims[2];
  g.To = d->out_dims[0]; g.Ho = d->out_dims[1]; g.Wo = d->out_dims[2];
  g.cs_img = d->cs_img; g.cs_band = d->cs_band; g.cs0 = d->cs0; g.cs1 = d->cs1;
  g.off = mode == 1 ? L - 2 : L / 2 - 1;
  return g;
}

// ------------------------------------------------------------------------------------------------ LDS layouts (floats)
// A kernel's regions lie end to end from lds[0]; dw_*_lds<R> is the offset of region R, and with R = the number of regions the size of the
// request. The arguments are the extents as the kernel names them (a function that adds a constant to one of them itself is folded
// differently from the kernel's own sum and costs the no-wrap flags of the offset: profiles/dwt_tiles_header.md). The 3-D analysis and the
// fused synthesis kernel changed with such a call: their carve and their chooser's formula stay in dwt_analysis.hip / dwt_synthesis.hip.
// floats of a staged raw coefficient row of dwt_synthesis2_kernel: QW4 groups of four output pairs, plus the window's reach
__host__ __device__ __forceinline__ int dw_staged_row_width(int QW4, int L) { return 4 * QW4 + L / 2 - 1; }
// dwt_synthesis2_kernel: S1 [2 bh][EH][NW], then the staged raw rows R [2 bh][EH][lo, hi][RW]
template <int R>
__host__ __device__ __forceinline__ int dw_synthesis2_lds(int NW, int EH, int RW) {
  if constexpr (R == 1) return 2 * EH * NW;
  else return 2 * EH * NW + 4 * EH * RW;
}
// dwt_synthesis3_stream_kernel: S1 [2 bt][2 bh][EH][NW], then S2 [2 bt][2 NQH][NW]
template <int R>
__host__ __device__ __forceinline__ int dw_stream_lds(int NW, int EH, int NQH) {
  if constexpr (R == 1) return 4 * EH * NW;
  else return 4 * EH * NW + 4 * NQH * NW;
}

#ifdef __HIPCC__
__device__ __forceinline__ int xcd_tile(int bid, int nb) {
  return (nb & 7) ? bid : (bid & 7) * (nb >> 3) + (bid >> 3);
}
// Periodic wrap without an integer division: every index a valid item asks for lies within one period of [0, P) (|j| < 2 P is
// guaranteed by L <= P, checked on the host); items of a ragged last tile may ask for more and are clamped (their results are
// never stored), so that no read leaves the tensor.
__device__ __forceinline__ int wrap_period(int j, int P) {
  j = j < 0 ? j + P : j;
  j = j >= P ? j - P : j;
  j = j >= P ? j - P : j;
  return min(max(j, 0), P - 1);
}
template <int MODE>
__device__ __forceinline__ int amap(int j, int N, int odd) {      // signal index read by an analysis pass: [0, N) or -1 (= zero)
  if (MODE == 1) return (j >= 0 && j < N) ? j : -1;
  j = wrap_period(j, N + odd);
  return j > N - 1 ? N - 1 : j;
}
template <int MODE>
__device__ __forceinline__ int smap(int K, int M) {               // coefficient index read by a synthesis pass
  if (MODE == 1) return (K >= 0 && K < M) ? K : -1;
  return wrap_period(K, M);
}

// block id -> (image, T tile, H tile): logical tile ids are laid out so that one XCD (= one L2) owns whole images
template <int ND>
__device__ __forceinline__ void dw_tile(int bid, const FusedGeom& g, int& img, int& tt, int& th) {
  int b = xcd_tile(bid, g.n_blocks);
  th = b % g.tiles_h;
  b /= g.tiles_h;
  tt = (ND == 3) ? b % g.tiles_t : 0;
  img = (ND == 3) ? b / g.tiles_t : b;
}
// sub-bands a W pass reads or writes for (T band bt, H band bh): 3-D band = bt 4 + bh 2 + bw, 2-D band = bw 2 + bh
template <int ND>
__device__ __forceinline__ void dw_bands(int bt, int bh, int& band_lo, int& band_hi) {
  band_lo = (ND == 3) ? bt * 4 + bh * 2 : bh;
  band_hi = (ND == 3) ? band_lo + 1 : bh + 2;
}

// One sample v at window position jj of an analysis register pass -> the NK sliding accumulators it belongs to (m = jj - 2 k)
template <int L, int NK>
__device__ __forceinline__ void dw_scatter(float v, int jj, const Taps& t, float* lo, float* hi) {
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int m = jj - 2 * k;
    if (m >= 0 && m < L) {
      lo[k] = fmaf(t.lo[L - 1 - m], v, lo[k]);
      hi[k] = fmaf(t.hi[L - 1 - m], v, hi[k]);
    }
  }
}
// The L-term analysis sums of a full window, m = 0 .. L - 1 as in analysis_kernel
template <int L>
__device__ __forceinline__ void dw_dot(const float* w, const Taps& t, float& lo, float& hi) {
  lo = 0.f; hi = 0.f;
#pragma unroll
  for (int m = 0; m < L; ++m) {
    lo = fmaf(t.lo[L - 1 - m], w[m], lo);
    hi = fmaf(t.hi[L - 1 - m], w[m], hi);
  }
}

// Term i of a synthesis pass that produces BOTH outputs n = 2 q - off, 2 q - off + 1 of one q from the coefficients K = q - i:
// a0 (r = 0) and a1 (r = 1), each in the order i = 0, 1, .. of synth_point
__device__ __forceinline__ void dw_pair_term(float vl, float vh, const Taps& t, int i, float& a0, float& a1) {
  a0 = fmaf(vl, t.lo[2 * i], a0);
  a0 = fmaf(vh, t.hi[2 * i], a0);
  a1 = fmaf(vl, t.lo[2 * i + 1], a1);
  a1 = fmaf(vh, t.hi[2 * i + 1], a1);
}
// Output (qq, r) of a synthesis register pass from the column's ET = NQ + E coefficients cl / ch (entry e <-> q = q0 - E + e)
template <int L>
__device__ __forceinline__ float dw_column(const float* cl, const float* ch, const Taps& t, int qq, int r) {
  constexpr int E = L / 2 - 1;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < L / 2; ++i) {
    acc = fmaf(cl[qq - i + E], t.lo[r + 2 * i], acc);
    acc = fmaf(ch[qq - i + E], t.hi[r + 2 * i], acc);
  }
  return acc;
}

// 3-D synthesis: the store of time sample (qq, r) of the output column o (its sample in frame 0)
__device__ __forceinline__ void dw_store_t(float* o, const FusedGeom& g, int qt_start, int qq, int r, float acc) {
  const int nt = 2 * (qt_start + qq) + r - g.off;
  if (nt >= 0 && nt < g.T) o[nt * ((int64_t)g.H * g.W)] = acc;
}
#endif
