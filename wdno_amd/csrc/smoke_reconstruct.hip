// smoke_reconstruct.hip -- the wavelet branch of InferencePipeline.run_base_model (smoke/inference_2d.py:137-152) as ONE launch: the sampled
// state x [B][F][C][H][W] in network units becomes pred [B][to][6][ho][wo], channels 0..4 = IDWT3(x RESCALER) of fields 0..4, cropped, channel 5
// = IDWT1(the two half-means of the last channel) in every cell. include/wdno_hip.h states the contract; wdno_amd/smoke/reconstruct.py: plan()
// chooses the tile.
//
// Zero-mode synthesis of L = 6 taps on one axis, as csrc/smoke_guidance.hip:  x[n] = sum_j lo[kb - j] g_lo[par + 2 j] + hi[kb - j] g_hi[par + 2 j]
// with par = n & 1, kb = (n + 4 - par) / 2, j = 0, 1, 2 (N = 2 M - 4, so kb - j is always inside [0, M) for n < N). band = 4 bt + 2 bh + bw, the
// channel of field f being 8 f + band.
//
// Tile blocks: one workgroup of 256 threads per (sample, field, tile of tn frames x hn rows, full width), passes in the order T, H, W:
//   T pass  reads the coefficients in place from global memory (the frame pair n, n + 1 shares its three coefficient frames: six loads give two
//           values) and writes A1 [4 (bh, bw)][tn][KH][wc], KH = hn / 2 + 2 coefficient rows;
//   H pass  A1 -> A2 [2 (bw)][tn][hn][wc];   W pass  A2 -> registers -> pred.
// Putting the W pass last keeps both buffers wc (not wo) wide and the T pass first needs no staging buffer: (tn, hn) = (4, 8) on the 34 x 34
// block is 21 760 B of LDS where the guidance kernel's order needs 47 488 B, the frame axis has no halo in LDS at all and the row halo costs
// KH / (hn / 2) = 1.5 x of the cheapest pass only. Flat indices are split into (column, row, frame) once per pass and advanced by adds
// (Idx3): no integer division per element.
// Smoke-out blocks: cdiv(to, tn) more workgroups per sample. Each forms the fp64 sums of x[b, k, C - 1] RESCALER[C - 1] (the product in fp32, as
// the reference forms it) over rows < half and rows >= half of the tn / 2 + 2 coefficient frames its frames read -- per-thread strided sums,
// then a tree over the 256 threads --, rounds the means to fp32, synthesises its tn frames and stores each value to the ho wo cells.
// Nothing is atomic and every sum has a fixed order: a sample's bits do not depend on the batch size or on its index.
// wdno_smoke_reconstruct_at: the coefficient block starts at row and column `off` of the tensor (the space super-resolution level,
// smoke/inference_2d.py:219: off = 1); the smoke-out blocks do not move.
#include "common.h"
#include "idx3.h"

namespace {

constexpr int L = 6;
constexpr int NT = 256;

struct RTaps { float lo[L], hi[L]; };      // rec_lo, rec_hi

struct SRecP {
  const float* x; const float* resc; float* pred;
  int F, C, H, W;
  int64_t ss; int fs, cs, rs;                // strides of sample, frame, channel, row (elements)
  int tc, hc, wc, to, ho, wo;
  int half, tn, hn;
  int ntiles;                                // tile blocks per sample; the blocks after them are smoke-out blocks
  int off;                                   // row and column at which the coefficient block starts (wdno_smoke_reconstruct_at)
};

__device__ __forceinline__ void tile_block(const SRecP& p, const RTaps& g, float* smem, int blk, int b) {
  const int tid = threadIdx.x;
  const int tn = p.tn, hn = p.hn, KH = hn / 2 + 2, wc = p.wc, wo = p.wo;
  const int nrt = (p.ho + hn - 1) / hn, nft = (p.to + tn - 1) / tn;
  const int field = blk / (nft * nrt);
  blk -= field * nft * nrt;
  const int n0 = (blk / nrt) * tn, h0 = (blk % nrt) * hn, k0h = h0 / 2;
  float* const A1 = smem;                         // [4][tn][KH][wc]
  float* const A2 = A1 + 4 * tn * KH * wc;        // [2][tn][hn][wc]
  const float* const xb = p.x + (size_t)b * p.ss + (size_t)p.off * p.rs + p.off;      // the block's first row and column
  // T pass
  for (int q = 0; q < 4; ++q) {
    const int ch = 8 * field + q;
    const float rl = p.resc[ch], rh = p.resc[ch + 4];
    const float* const xl = xb + (size_t)ch * p.cs;
    const float* const xh = xl + (size_t)4 * p.cs;
    float* const dst = A1 + q * tn * KH * wc;
    for (Idx3<NT> i(tid, wc, KH); i.c < tn / 2; i.next()) {
      const int n = n0 + 2 * i.c, kr = k0h + i.b, kb = (n + 4) >> 1;      // frames n and n + 1 read coefficient frames kb, kb - 1, kb - 2
      float e = 0.f, o = 0.f;
      if (n < p.to && kr < p.hc) {
        const size_t at = (size_t)kr * p.rs + i.a;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const size_t off = (size_t)(kb - j) * p.fs + at;
          const float lo = __fmul_rn(xl[off], rl), hi = __fmul_rn(xh[off], rh);
          e = fmaf(lo, g.lo[2 * j], e);     e = fmaf(hi, g.hi[2 * j], e);
          o = fmaf(lo, g.lo[2 * j + 1], o); o = fmaf(hi, g.hi[2 * j + 1], o);
        }
      }
      float* const d = dst + ((2 * i.c) * KH + i.b) * wc + i.a;
      d[0] = e;
      d[KH * wc] = o;
    }
  }
  __syncthreads();
  // H pass
  for (int bw = 0; bw < 2; ++bw) {
    const float* const lo = A1 + bw * tn * KH * wc;
    const float* const hi = lo + 2 * tn * KH * wc;
    float* const dst = A2 + bw * tn * hn * wc;
    for (Idx3<NT> i(tid, wc, hn); i.c < tn; i.next()) {
      const int row = h0 + i.b, par = row & 1, kb = ((row + 4 - par) >> 1) - k0h;
      const int src = (i.c * KH + kb) * wc + i.a;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        acc = fmaf(lo[src - j * wc], par ? g.lo[2 * j + 1] : g.lo[2 * j], acc);
        acc = fmaf(hi[src - j * wc], par ? g.hi[2 * j + 1] : g.hi[2 * j], acc);
      }
      dst[(i.c * hn + i.b) * wc + i.a] = acc;
    }
  }
  __syncthreads();
  // W pass
  float* const pb = p.pred + ((size_t)b * p.to * 6 + field) * p.ho * wo;
  const float* const hi0 = A2 + tn * hn * wc;
  for (Idx3<NT> i(tid, wo, hn); i.c < tn; i.next()) {
    const int fr = n0 + i.c, row = h0 + i.b;
    if (fr >= p.to || row >= p.ho) continue;
    const int par = i.a & 1, kb = (i.a + 4 - par) >> 1;
    const int src = (i.c * hn + i.b) * wc + kb;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc = fmaf(A2[src - j], par ? g.lo[2 * j + 1] : g.lo[2 * j], acc);
      acc = fmaf(hi0[src - j], par ? g.hi[2 * j + 1] : g.hi[2 * j], acc);
    }
    pb[((size_t)fr * 6 * p.ho + row) * wo + i.a] = acc;
  }
}

__device__ __forceinline__ void smoke_out_block(const SRecP& p, const RTaps& g, float* smem, int blk, int b) {
  const int tid = threadIdx.x;
  const int KT = p.tn / 2 + 2, n0 = blk * p.tn, k0 = n0 / 2;
  double* const red = reinterpret_cast<double*>(smem);           // [NT]
  float* const mean = reinterpret_cast<float*>(red + NT);        // [2][KT]: lo, hi
  const float r = p.resc[p.C - 1];
  const float* const xb = p.x + (size_t)b * p.ss + (size_t)(p.C - 1) * p.cs;
  for (int s = 0; s < 2 * KT; ++s) {
    const int kf = k0 + (s % KT), upper = s / KT;
    const int r0 = upper ? p.half : 0, nr = upper ? p.H - p.half : p.half;
    double acc = 0.0;
    if (kf < p.tc) {
      const float* const src = xb + (size_t)kf * p.fs + (size_t)r0 * p.rs;
      for (Idx3<NT> i(tid, p.W, nr); i.c < 1; i.next()) acc += (double)__fmul_rn(src[(size_t)i.b * p.rs + i.a], r);
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) mean[s] = (float)(red[0] / (double)(nr * p.W));
    __syncthreads();
  }
  float* const pb = p.pred + ((size_t)b * p.to * 6 + 5) * p.ho * p.wo;
  const int cells = p.ho * p.wo;
  for (int dn = 0; dn < p.tn && n0 + dn < p.to; ++dn) {
    const int fr = n0 + dn, par = fr & 1, kb = ((fr + 4 - par) >> 1) - k0;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc = fmaf(mean[kb - j], par ? g.lo[2 * j + 1] : g.lo[2 * j], acc);
      acc = fmaf(mean[KT + kb - j], par ? g.hi[2 * j + 1] : g.hi[2 * j], acc);
    }
    float* const dst = pb + (size_t)fr * 6 * cells;
    for (int idx = tid; idx < cells; idx += NT) dst[idx] = acc;
  }
}

__global__ __launch_bounds__(NT) void smoke_reconstruct_kernel(SRecP p, RTaps g) {
  extern __shared__ __align__(16) float smem[];
  const int blk = blockIdx.x, b = blockIdx.y;
  if (blk < p.ntiles) tile_block(p, g, smem, blk, b);
  else smoke_out_block(p, g, smem, blk - p.ntiles, b);
}

// bytes of LDS a workgroup needs (wdno_amd/smoke/reconstruct.py: lds_bytes states the same)
int64_t lds_need(const wdno_smoke_reconstruct_desc* d) {
  const int64_t KH = d->hn / 2 + 2, KT = d->tn / 2 + 2;
  const int64_t tile = 4 * (4 * (int64_t)d->tn * KH * d->wc + 2 * (int64_t)d->tn * d->hn * d->wc), so = 8 * NT + 4 * 2 * KT;
  return tile > so ? tile : so;
}

int validate(const wdno_smoke_reconstruct_desc* d) {
  if (!d) return WDNO_EINVAL;
  if (d->mode != 1 || d->L != L) return WDNO_EUNSUPPORTED;
  WDNO_REQUIRE(d->B > 0 && d->B <= 65535 && d->F > 0 && d->C >= 42 && d->H > 1 && d->W > 0);
  WDNO_REQUIRE(d->row_stride >= d->W && (int64_t)d->chan_stride >= (int64_t)d->H * d->row_stride &&
               (int64_t)d->frame_stride >= (int64_t)d->C * d->chan_stride && d->sample_stride >= (int64_t)d->F * d->frame_stride);
  WDNO_REQUIRE((int64_t)d->F * d->C * d->H * d->W < ((int64_t)1 << 31) && (int64_t)d->B * d->sample_stride < ((int64_t)1 << 40));
  WDNO_REQUIRE(d->tc >= 3 && d->tc <= d->F && d->hc >= 3 && d->hc <= d->H && d->wc >= 3 && d->wc <= d->W);      // a block larger than the tensor
  WDNO_REQUIRE(d->to >= 1 && d->to <= 2 * d->tc - L + 2 && d->ho >= 1 && d->ho <= 2 * d->hc - L + 2 && d->wo >= 1 && d->wo <= 2 * d->wc - L + 2);      // a crop larger than the reconstruction
  WDNO_REQUIRE((int64_t)d->to * 6 * d->ho * d->wo < ((int64_t)1 << 31));
  WDNO_REQUIRE(d->half >= 1 && d->half < d->H);
  WDNO_REQUIRE(d->tn >= 2 && d->hn >= 2 && !(d->tn & 1) && !(d->hn & 1) && d->tn <= 64 && d->hn <= 64);
  WDNO_REQUIRE(d->lds_bytes >= lds_need(d) && d->lds_bytes <= 65536);
  return WDNO_OK;
}

}  // namespace

extern "C" int wdno_smoke_reconstruct_at(const float* x, const float* rescaler, float* pred, const wdno_smoke_reconstruct_desc* d, int off,
                                         const float* filt, wdno_stream_t s) {
  WDNO_REQUIRE(x && rescaler && pred && d && filt && x != pred);
  const int rc = validate(d);
  if (rc) return rc;
  WDNO_REQUIRE(off >= 0 && d->hc + off <= d->H && d->wc + off <= d->W);
  SRecP p;
  p.x = x; p.resc = rescaler; p.pred = pred;
  p.F = d->F; p.C = d->C; p.H = d->H; p.W = d->W;
  p.ss = d->sample_stride; p.fs = d->frame_stride; p.cs = d->chan_stride; p.rs = d->row_stride;
  p.tc = d->tc; p.hc = d->hc; p.wc = d->wc; p.to = d->to; p.ho = d->ho; p.wo = d->wo;
  p.half = d->half; p.tn = d->tn; p.hn = d->hn; p.off = off;
  const int nft = cdiv(d->to, d->tn);
  p.ntiles = 5 * nft * cdiv(d->ho, d->hn);
  RTaps g;
  for (int m = 0; m < L; ++m) { g.lo[m] = filt[2 * L + m]; g.hi[m] = filt[3 * L + m]; }
  smoke_reconstruct_kernel<<<dim3(p.ntiles + nft, d->B), NT, (size_t)d->lds_bytes, as_stream(s)>>>(p, g);
  return wdno_check_launch();
}

extern "C" int wdno_smoke_reconstruct(const float* x, const float* rescaler, float* pred, const wdno_smoke_reconstruct_desc* d, const float* filt,
                                      wdno_stream_t s) {
  return wdno_smoke_reconstruct_at(x, rescaler, pred, d, 0, filt, s);
}
