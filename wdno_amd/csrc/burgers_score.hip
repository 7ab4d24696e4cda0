// burgers_score.hip -- the sums and order statistics behind mse_deviation and the two metric(..., evaluate=True) calls of diffuse_2dconv
// (eval_ddpm_burgers.py:220-230, test_util.py:79-98) for one batch as ONE launch. include/wdno_hip.h states the contract and the 14 columns
// of out; wdno_amd/burgers/score.py applies the metric formulas to them.
//
// One workgroup of 1024 threads per sample. Every difference is (double)a - (double)b of the fp32 values and is squared and accumulated
// in fp64: per-thread strided partial sums, a wave butterfly, then the 16 wave sums added by one thread in wave order.
// The medians. torch's median of a row of n values is the element of rank (n - 1) / 2 of the sorted row. |c - t| of both candidates is
// staged in LDS as fp64 (2 x 8 n_w bytes) and the element of that rank is found by exact rank counting: element i has rank
// #{j : v_j < v_i or (v_j == v_i and j < i)}, a bijection onto 0 .. n - 1 whatever the ties, so exactly one thread finds its count equal to
// the wanted rank and stores its value. Squaring is monotone on non-negative fp64 values (one rounding), so the median of (c - t)^2 is
// the square of the median of |c - t|: one selection per candidate gives both. n_w^2 / 1024 comparisons per thread: 14 at the evaluation's
// 120 columns, 3 600 at 1 920.
// Nothing is atomic and every sum has a fixed order: a sample's row of out depends on neither the batch size nor its index.
#include "common.h"

namespace {

constexpr int NT = 1024;
constexpr int NS = 10;      // ddpm | candidate u_repeat: strided sq, sq, abs | candidate x_gt: strided sq, sq, abs | f^2 | t^2 | |t|

struct BScoreP {
  const float* u; const float* f; const float* gt; const float* ut; double* out;
  int64_t gs, gr, gc, ts, tr, tc;            // strides of x_gt and u_target: sample, row, column (elements)
  int n_t, n_x, sub, nw;
};

__global__ __launch_bounds__(NT) void burgers_score_kernel(BScoreP p) {
  extern __shared__ __align__(16) double absd[];          // [2][nw]: |c - t| of the two candidates
  __shared__ double red[NT / 64][NS];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n_t = p.n_t, n_x = p.n_x, sub = p.sub, nw = p.nw;
  const float* const u = p.u + (size_t)b * n_t * n_x;
  const float* const f = p.f + (size_t)b * (n_t - 1) * n_x;
  const float* const gt = p.gt + (int64_t)b * p.gs;
  const float* const tl = p.ut + (int64_t)b * p.ts + (int64_t)(n_t - 1) * p.tr;      // the last row of u_target
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  // rows 1 .. n_t - 1 of u against x_gt[:, ::sub]; f^2 over the same index range ([n_t - 1][n_x])
  for (int idx = tid; idx < (n_t - 1) * n_x; idx += NT) {
    const int r = idx / n_x, j = idx - r * n_x;
    const double e = (double)u[idx + n_x] - (double)gt[(int64_t)(r + 1) * p.gr + (int64_t)j * sub * p.gc];
    s[0] += e * e;
    const double fv = (double)f[idx];
    s[7] += fv * fv;
  }
  // the last row: both candidates against t
  const float* const ul = u + (size_t)(n_t - 1) * n_x;
  const float* const gl = gt + (int64_t)(n_t - 1) * p.gr;
  for (int col = tid; col < nw; col += NT) {
    const int j = col / sub;
    const double t = (double)tl[(int64_t)col * p.tc];
    const double e0 = (double)ul[j] - t, e1 = (double)gl[(int64_t)col * p.gc] - t;
    const double a0 = fabs(e0), a1 = fabs(e1), q0 = e0 * e0, q1 = e1 * e1;
    absd[col] = a0;
    absd[nw + col] = a1;
    if (col - j * sub == 0) { s[1] += q0; s[4] += q1; }
    s[2] += q0; s[3] += a0;
    s[5] += q1; s[6] += a1;
    s[8] += t * t; s[9] += fabs(t);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double v = wave_sum_d(s[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();                                         // (also: absd is complete)
  double* const o = p.out + (size_t)b * 14;
  if (tid < NS) {
    double v = 0.0;
    for (int wv = 0; wv < NT / 64; ++wv) v += red[wv][tid];
    // out columns: 0 ddpm | 1 2 3 (4 5) u_repeat | 6 7 8 (9 10) x_gt | 11 f^2 | 12 t^2 | 13 |t|
    const int at = tid == 0 ? 0 : (tid <= 3 ? tid : (tid <= 6 ? tid + 2 : tid + 4));
    o[at] = v;
  }
  // the medians: rank (nw - 1) / 2 of |c - t|, by rank counting
  const int want = (nw - 1) / 2;
  for (int item = tid; item < 2 * nw; item += NT) {
    const int cand = item / nw, i = item - cand * nw;
    const double* const v = absd + cand * nw;
    const double vi = v[i];
    int rank = 0;
    for (int j = 0; j < nw; ++j) {
      const double vj = v[j];
      rank += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
    }
    if (rank == want) {
      o[4 + 5 * cand] = vi * vi;
      o[5 + 5 * cand] = vi;
    }
  }
}

}  // namespace

extern "C" int wdno_burgers_score(const float* u, const float* f, const float* x_gt, const float* u_target, double* out,
                                  const wdno_burgers_score_desc* d, wdno_stream_t s) {
  WDNO_REQUIRE(u && f && x_gt && u_target && out && d);
  WDNO_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0);
  WDNO_REQUIRE(((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(x_gt) | reinterpret_cast<uintptr_t>(u_target)) & 3) == 0);
  WDNO_REQUIRE(d->B > 0 && d->n_t >= 2 && d->n_x >= 1 && d->sub >= 1);
  WDNO_REQUIRE((int64_t)d->n_t * d->n_x < ((int64_t)1 << 31) && (int64_t)d->n_x * d->sub <= 3840);      // the two fp64 rows fit 64 KiB of LDS
  WDNO_REQUIRE(d->gt_sample_stride >= 0 && d->gt_row_stride >= 0 && d->gt_col_stride >= 0);
  WDNO_REQUIRE(d->ut_sample_stride >= 0 && d->ut_row_stride >= 0 && d->ut_col_stride >= 0);
  const int nw = d->n_x * d->sub;
  WDNO_REQUIRE(d->lds_bytes == 16 * nw);
  BScoreP p;
  p.u = u; p.f = f; p.gt = x_gt; p.ut = u_target; p.out = out;
  p.gs = d->gt_sample_stride; p.gr = d->gt_row_stride; p.gc = d->gt_col_stride;
  p.ts = d->ut_sample_stride; p.tr = d->ut_row_stride; p.tc = d->ut_col_stride;
  p.n_t = d->n_t; p.n_x = d->n_x; p.sub = d->sub; p.nw = nw;
  burgers_score_kernel<<<dim3(d->B), NT, (size_t)d->lds_bytes, as_stream(s)>>>(p);
  return wdno_check_launch();
}
