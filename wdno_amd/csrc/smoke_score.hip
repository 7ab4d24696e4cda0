// smoke_score.hip -- the arithmetic of InferencePipeline.multi_evaluate (smoke/inference_2d.py:426-439) for one (pred, data) pair as ONE launch
// that reads only what the metrics read: pred [B][T][6][h][w] fp32 and, per channel, a strided (possibly broadcast) view of the data, fp32 or
// fp64. include/wdno_hip.h states the contract; wdno_amd/smoke/score.py builds the channel table.
//
// One workgroup of 1024 threads per sample. Channel by channel (so the element type is uniform), every thread walks the (frame, row, column)
// cells tid, tid + 1024, ... and adds (double)pred - (double)data squared, and data squared, to its fp64 partial sums; the partial sums are
// combined by a wave butterfly, then the 16 wave sums by thread 0 in wave order. Nothing is atomic: a sample's five numbers depend on
// neither the batch size nor its index.
#include "common.h"
#include "idx3.h"

namespace {

constexpr int NT = 1024;

struct ScoreP {
  const float* pred; double* out;
  wdno_smoke_score_channel ch[6];
  int T, h, w;
};

template <typename D>
__device__ __forceinline__ void channel_sums(const ScoreP& p, int c, int b, double& err, double& sq) {
  const wdno_smoke_score_channel& k = p.ch[c];
  const D* const data = static_cast<const D*>(k.ptr) + (int64_t)b * k.sample_stride;
  const float* const pred = p.pred + ((size_t)b * p.T * 6 + c) * p.h * p.w;
  const int t0 = c == 0 ? 1 : 0;               // mask[:, 0, 0] = False: frame 0 of channel 0 is in no sum
  for (Idx3<NT> i((int)threadIdx.x, p.w, p.h); i.c < p.T; i.next()) {
    if (i.c < t0) continue;
    const double d = (double)data[(int64_t)i.c * k.frame_stride + (int64_t)i.b * k.row_stride + (int64_t)i.a * k.col_stride];
    const double e = (double)pred[((size_t)i.c * 6 * p.h + i.b) * p.w + i.a] - d;
    err += e * e;
    sq += d * d;
  }
}

__global__ __launch_bounds__(NT) void smoke_score_kernel(ScoreP p) {
  __shared__ double red[NT / 64][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};          // err of channels 0..2, err of channel 5, data^2 of channels 0..2, data^2 of channels 3..4
  for (int c = 0; c < 6; ++c) {
    double err = 0.0, sq = 0.0;
    if (p.ch[c].is_double) channel_sums<double>(p, c, b, err, sq);
    else channel_sums<float>(p, c, b, err, sq);
    if (c < 3) { s[0] += err; s[2] += sq; }
    else if (c < 5) s[3] += sq;
    else s[1] += err;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum_d(s[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < 4) {
    double v = 0.0;
    for (int wv = 0; wv < NT / 64; ++wv) v += red[wv][tid];
    p.out[(size_t)b * 5 + tid] = v;
  }
  if (tid == 4) {
    const wdno_smoke_score_channel& k = p.ch[5];
    const int64_t at = (int64_t)b * k.sample_stride + (int64_t)(p.T - 1) * k.frame_stride;
    p.out[(size_t)b * 5 + 4] = k.is_double ? static_cast<const double*>(k.ptr)[at] : (double)static_cast<const float*>(k.ptr)[at];
  }
}

// ---- the four comparisons of the super-resolution branch (smoke/inference_2d.py:405-456, simulation mode): a workgroup per (sample, comparison).
// A comparison is a grid of g x g cells; the data cell is (row ds, column ds) of the full-resolution data, the pred value is
//   PM_STRIDE   pred[row ps, column ps]                 (base, current; linear and nearest when the grids are equal)
//   PM_NEAREST  pred[row / 2, column / 2]               (F.interpolate(mode='nearest') to twice the side)
//   PM_LINEAR   the bilinear value at twice the side, align_corners = False: source coordinate y / 2 - 0.25 clamped at 0, so an even row 2 k
//               is 0.25 pred[k - 1] + 0.75 pred[k] (k - 1 clamped to 0), an odd row 2 k + 1 is 0.75 pred[k] + 0.25 pred[k + 1] (k + 1 clamped to
//               n - 1); weights and products are exact in fp64, the four-term sum is formed rows first.
enum { PM_STRIDE = 0, PM_NEAREST = 1, PM_LINEAR = 2 };

struct ScoreSuperP {
  const float* pred; double* out;
  wdno_smoke_score_channel ch[6];
  int T, n, N;
};

__device__ __forceinline__ void lin_taps(int y, int n, int& y0, int& y1, double& w0) {
  const int k = y >> 1;
  if (y & 1) { y0 = k; y1 = min(k + 1, n - 1); w0 = 0.75; }
  else { y0 = max(k - 1, 0); y1 = k; w0 = 0.25; }
}

template <typename D, int PM>
__device__ __forceinline__ void super_channel_sums(const ScoreSuperP& p, int c, int b, int g, int ps, int ds, double& err, double& sq) {
  const wdno_smoke_score_channel& k = p.ch[c];
  const D* const data = static_cast<const D*>(k.ptr) + (int64_t)b * k.sample_stride;
  const int n = p.n;
  const float* const pred = p.pred + ((size_t)b * p.T * 6 + c) * n * n;
  const int t0 = c == 0 ? 1 : 0;
  for (Idx3<NT> i((int)threadIdx.x, g, g); i.c < p.T; i.next()) {
    if (i.c < t0) continue;
    const double d = (double)data[(int64_t)i.c * k.frame_stride + (int64_t)(i.b * ds) * k.row_stride + (int64_t)(i.a * ds) * k.col_stride];
    const float* const pf = pred + (size_t)i.c * 6 * n * n;
    double v;
    if (PM == PM_STRIDE) v = (double)pf[(i.b * ps) * n + i.a * ps];
    else if (PM == PM_NEAREST) v = (double)pf[(i.b >> 1) * n + (i.a >> 1)];
    else {
      int y0, y1, x0, x1;
      double wy, wx;
      lin_taps(i.b, n, y0, y1, wy);
      lin_taps(i.a, n, x0, x1, wx);
      const double r0 = wx * (double)pf[y0 * n + x0] + (1.0 - wx) * (double)pf[y0 * n + x1];
      const double r1 = wx * (double)pf[y1 * n + x0] + (1.0 - wx) * (double)pf[y1 * n + x1];
      v = wy * r0 + (1.0 - wy) * r1;
    }
    const double e = v - d;
    err += e * e;
    sq += d * d;
  }
}

template <int PM>
__device__ __forceinline__ void super_sums(const ScoreSuperP& p, int b, int g, int ps, int ds, double* s) {
  for (int c = 0; c < 6; ++c) {
    double err = 0.0, sq = 0.0;
    if (p.ch[c].is_double) super_channel_sums<double, PM>(p, c, b, g, ps, ds, err, sq);
    else super_channel_sums<float, PM>(p, c, b, g, ps, ds, err, sq);
    if (c < 3) { s[0] += err; s[2] += sq; }
    else if (c < 5) s[3] += sq;
    else s[1] += err;
  }
}

__global__ __launch_bounds__(NT) void smoke_score_super_kernel(ScoreSuperP p) {
  __shared__ double red[NT / 64][4];
  const int b = blockIdx.x, cmp = blockIdx.y, tid = threadIdx.x;
  const int f = p.N / p.n, hn = p.N >> 1;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (cmp == 0) super_sums<PM_STRIDE>(p, b, hn, p.n / hn, 2, s);
  else if (cmp == 1) super_sums<PM_STRIDE>(p, b, p.n, 1, f, s);
  else if (f == 1) super_sums<PM_STRIDE>(p, b, p.N, 1, 1, s);
  else if (cmp == 2) super_sums<PM_LINEAR>(p, b, p.N, 1, 1, s);
  else super_sums<PM_NEAREST>(p, b, p.N, 1, 1, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum_d(s[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  double* const out = p.out + ((size_t)b * 4 + cmp) * 5;
  if (tid < 4) {
    double v = 0.0;
    for (int wv = 0; wv < NT / 64; ++wv) v += red[wv][tid];
    out[tid] = v;
  }
  if (tid == 4) {
    const wdno_smoke_score_channel& k = p.ch[5];
    const int64_t at = (int64_t)b * k.sample_stride + (int64_t)(p.T - 1) * k.frame_stride;
    out[4] = k.is_double ? static_cast<const double*>(k.ptr)[at] : (double)static_cast<const float*>(k.ptr)[at];
  }
}

}  // namespace

extern "C" int wdno_smoke_score_super(const float* pred, const wdno_smoke_score_channel* data, double* out, int B, int T, int n, int N, wdno_stream_t s) {
  WDNO_REQUIRE(pred && data && out);
  WDNO_REQUIRE(B > 0 && B <= 65535 && T > 0 && n > 0 && N > 1 && !(N & 1) && (n == N || 2 * n == N));
  WDNO_REQUIRE((int64_t)T * 6 * N * N < ((int64_t)1 << 31));
  WDNO_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0);
  ScoreSuperP p;
  p.pred = pred; p.out = out; p.T = T; p.n = n; p.N = N;
  for (int c = 0; c < 6; ++c) {
    const wdno_smoke_score_channel& k = data[c];
    WDNO_REQUIRE(k.ptr && k.sample_stride >= 0 && k.frame_stride >= 0 && k.row_stride >= 0 && k.col_stride >= 0);
    WDNO_REQUIRE((reinterpret_cast<uintptr_t>(k.ptr) & (k.is_double ? 7 : 3)) == 0);
    p.ch[c] = k;
  }
  smoke_score_super_kernel<<<dim3(B, 4), NT, 0, as_stream(s)>>>(p);
  return wdno_check_launch();
}

extern "C" int wdno_smoke_score(const float* pred, const wdno_smoke_score_channel* data, double* out, int B, int T, int h, int w, wdno_stream_t s) {
  WDNO_REQUIRE(pred && data && out);
  WDNO_REQUIRE(B > 0 && T > 0 && h > 0 && w > 0 && (int64_t)T * 6 * h * w < ((int64_t)1 << 31));
  WDNO_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0);
  ScoreP p;
  p.pred = pred; p.out = out; p.T = T; p.h = h; p.w = w;
  for (int c = 0; c < 6; ++c) {
    const wdno_smoke_score_channel& k = data[c];
    WDNO_REQUIRE(k.ptr && k.sample_stride >= 0 && k.frame_stride >= 0 && k.row_stride >= 0 && k.col_stride >= 0);
    WDNO_REQUIRE((reinterpret_cast<uintptr_t>(k.ptr) & (k.is_double ? 7 : 3)) == 0);
    p.ch[c] = k;
  }
  smoke_score_kernel<<<dim3(B), NT, 0, as_stream(s)>>>(p);
  return wdno_check_launch();
}
