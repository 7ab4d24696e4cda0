// smoke_cascade.hip -- the conditions of the space super-resolution level (InferencePipeline.run_super_model, smoke/inference_2d.py:176-196) as
// ONE launch that writes the sampler's whole condition source src [B][pad_t][82][pad_x][pad_x] in network units:
//   channels 40..79  low: the base sample's channels 0..39 inside its coefficient block (t0, h0, w0), read in place through the sample's
//                    strides, nearest x2 on rows and columns (upsample_coef type 'space'), zero beyond; copied, never rescaled
//   channels 24..39  control: the coefficient tensor coef [B][2][8][t1][h1][w1] of the fine controls (fields 3 and 4), replicate-padded by one
//                    cell on the four spatial sides (the block sits at row and column 1), zero beyond, / RESCALER[c] (IEEE division)
//   channel 80       init: sub-band f % 4 of the zero-mode 2-D analysis of rho(t = 0) on the fine grid in frame f -- the reference's
//                    super-level frame order (l.181), not the base level's f / (pad_t / 4) -- zero beyond (h1, w1), / RESCALER[80]
//   everything else  zero
// include/wdno_hip.h states the contract; wdno_amd/smoke/cascade.py: plan() checks the integers.
//
// grid = (B pad_t, 82): a workgroup of 256 threads owns one (sample, frame, channel) plane, so the branch on the channel is uniform and a
// thread decodes (row, float4 column) from its index with one multiply-high. The four sub-bands of the initial density are transformed by the
// workgroups of frames 0..3, which store the plane to the frames f, f + 4, ... that show it; the W pass runs first and the sums are those of
// csrc/pack.hip. HBM-bound on the store: 82 pad_t pad_x^2 floats per sample written once.
#include "common.h"
#include "fastdiv.h"

namespace {

constexpr int L = 6;
constexpr int NT = 256;
constexpr int C = 82;

struct CasP {
  const float* prev; const float* coef; const float* rho; const float* resc; float* out;
  int64_t pss, rss;                       // sample strides of prev and rho (elements)
  int pfs, pcs, prs, rrs;                 // frame, channel, row strides of prev; row stride of rho
  int t0, h0, w0, t1, h1, w1, Hf, Wf;
  int pad_t, pad_x;
  FastDiv dW4;
  float flo[L], fhi[L];                   // the FLIPPED decomposition filters: flo[m] = dec_lo[L - 1 - m]
};

__global__ __launch_bounds__(NT) void cascade_conditions_kernel(CasP p) {
  __shared__ float tp[2][L];
  const int tid = threadIdx.x, c = blockIdx.y;
  const int W4 = p.pad_x >> 2, n4 = p.pad_x * W4;
  const int b = (int)(blockIdx.x / (unsigned)p.pad_t), f = (int)(blockIdx.x - (unsigned)b * (unsigned)p.pad_t);
  const size_t plane = (size_t)p.pad_x * p.pad_x;
  float4* const out = reinterpret_cast<float4*>(p.out + ((size_t)blockIdx.x * C + c) * plane);
  if (c >= 24 && c < 40) {                 // control
    const float r = p.resc[c];
    const bool in_t = f < p.t1;
    const float* const src = p.coef + (((size_t)b * 16 + (c - 24)) * p.t1 + (in_t ? f : 0)) * p.h1 * p.w1;
    for (int i = tid; i < n4; i += NT) {
      const int h = fd_div(i, p.dW4), w = (i - h * W4) * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (in_t && h < p.h1 + 2) {
        const float* const row = src + (size_t)min(max(h - 1, 0), p.h1 - 1) * p.w1;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (w + e < p.w1 + 2) v[e] = row[min(max(w + e - 1, 0), p.w1 - 1)];
      }
      out[i] = make_float4(v[0] / r, v[1] / r, v[2] / r, v[3] / r);
    }
  } else if (c >= 40 && c < 80) {          // low
    const bool in_t = f < p.t0;
    const float* const src = p.prev + (size_t)b * p.pss + (size_t)(in_t ? f : 0) * p.pfs + (size_t)(c - 40) * p.pcs;
    for (int i = tid; i < n4; i += NT) {
      const int h = fd_div(i, p.dW4), w = (i - h * W4) * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (in_t && h < 2 * p.h0) {
        const float* const row = src + (size_t)(h >> 1) * p.prs;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (w + e < 2 * p.w0) v[e] = row[(w + e) >> 1];
      }
      out[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else if (c == C - 2) {                 // init: frames 0..3 transform, and store for every frame that shows their sub-band
    if (f >= 4) return;
    if (tid < 2 * L) tp[tid / L][tid % L] = tid < L ? p.flo[tid] : p.fhi[tid - L];
    __syncthreads();
    const float r = p.resc[c];
    const float* const fh = tp[f & 1];
    const float* const fw = tp[f >> 1];
    const float* const img = p.rho + (size_t)b * p.rss;
    const int rep = p.pad_t >> 2;
    const size_t fstride4 = (size_t)4 * C * (plane >> 2);      // float4s between frames f and f + 4
    for (int i = tid; i < n4; i += NT) {
      const int h = fd_div(i, p.dW4), w = (i - h * W4) * 4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (h < p.h1 && w < p.w1) {
        const int r0 = 2 * h - (L - 2), j0 = 2 * w - (L - 2);
#pragma unroll
        for (int m = 0; m < L; ++m) {
          const int rr = r0 + m;
          if (rr < 0 || rr >= p.Hf) continue;
          const float* const row = img + (size_t)rr * p.rrs;
          float xs[6 + L];
#pragma unroll
          for (int t = 0; t < 6 + L; ++t) { const int jj = j0 + t; xs[t] = (jj >= 0 && jj < p.Wf) ? row[jj] : 0.f; }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float a = 0.f;
#pragma unroll
            for (int t = 0; t < L; ++t) a = fmaf(fw[t], xs[2 * e + t], a);
            v[e] = fmaf(fh[m], a, v[e]);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) if (w + e >= p.w1) v[e] = 0.f;
      }
      const float4 o = make_float4(v[0] / r, v[1] / r, v[2] / r, v[3] / r);
      for (int k = 0; k < rep; ++k) out[i + (size_t)k * fstride4] = o;
    }
  } else {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = tid; i < n4; i += NT) out[i] = z;
  }
}

int validate(const wdno_smoke_cascade_desc* d) {
  if (!d) return WDNO_EINVAL;
  if (d->mode != 1 || d->L != L || d->C != C) return WDNO_EUNSUPPORTED;
  WDNO_REQUIRE(d->B > 0 && d->B <= 65535 && d->F0 > 0 && d->C0 >= 40 && d->H0 > 0 && d->W0 > 0);
  WDNO_REQUIRE(d->pad_t > 0 && d->pad_x > 0 && !(d->pad_t & 3) && !(d->pad_x & 3));
  WDNO_REQUIRE((int64_t)d->B * d->pad_t < ((int64_t)1 << 31) && (int64_t)d->pad_x * d->pad_x < ((int64_t)1 << 24));      // grid; fd_div range
  WDNO_REQUIRE(d->t0 >= 1 && d->t0 <= d->F0 && d->h0 >= 1 && d->h0 <= d->H0 && d->w0 >= 1 && d->w0 <= d->W0 && d->t0 <= d->pad_t);
  WDNO_REQUIRE(d->t1 >= 1 && d->t1 <= d->pad_t && d->h1 >= 1 && d->w1 >= 1);
  WDNO_REQUIRE(2 * d->h0 == d->h1 + 2 && 2 * d->w0 == d->w1 + 2 && d->h1 + 2 <= d->pad_x && d->w1 + 2 <= d->pad_x);
  WDNO_REQUIRE(d->Hf > 0 && d->Wf > 0 && d->h1 == (d->Hf + L - 1) / 2 && d->w1 == (d->Wf + L - 1) / 2);
  WDNO_REQUIRE(d->prev_row_stride >= d->W0 && (int64_t)d->prev_chan_stride >= (int64_t)d->H0 * d->prev_row_stride &&
               (int64_t)d->prev_frame_stride >= (int64_t)d->C0 * d->prev_chan_stride &&
               d->prev_sample_stride >= (int64_t)d->F0 * d->prev_frame_stride && d->prev_sample_stride < ((int64_t)1 << 31));
  WDNO_REQUIRE(d->rho_row_stride >= d->Wf && d->rho_sample_stride >= (int64_t)d->Hf * d->rho_row_stride && d->rho_sample_stride < ((int64_t)1 << 31));
  return WDNO_OK;
}

}  // namespace

extern "C" int wdno_smoke_cascade_conditions(const float* prev, const float* coef, const float* rho0, const float* rescaler, float* src,
                                             const wdno_smoke_cascade_desc* d, const float* filt, wdno_stream_t s) {
  WDNO_REQUIRE(prev && coef && rho0 && rescaler && src && d && filt);
  const int rc = validate(d);
  if (rc) return rc;
  WDNO_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0);
  CasP p;
  p.prev = prev; p.coef = coef; p.rho = rho0; p.resc = rescaler; p.out = src;
  p.pss = d->prev_sample_stride; p.rss = d->rho_sample_stride;
  p.pfs = d->prev_frame_stride; p.pcs = d->prev_chan_stride; p.prs = d->prev_row_stride; p.rrs = d->rho_row_stride;
  p.t0 = d->t0; p.h0 = d->h0; p.w0 = d->w0; p.t1 = d->t1; p.h1 = d->h1; p.w1 = d->w1; p.Hf = d->Hf; p.Wf = d->Wf;
  p.pad_t = d->pad_t; p.pad_x = d->pad_x;
  p.dW4 = make_fastdiv(d->pad_x >> 2);
  for (int m = 0; m < L; ++m) { p.flo[m] = filt[L - 1 - m]; p.fhi[m] = filt[L + L - 1 - m]; }
  cascade_conditions_kernel<<<dim3((unsigned)(d->B * d->pad_t), C), NT, 0, as_stream(s)>>>(p);
  return wdno_check_launch();
}
