// burgers_datagen.hip -- the Burgers data-set generator (make_data_varying_f + burgers_numeric_solve_free + the two slices of
// generate_data_burgers_equation, burgers/ddpm_burgers/generate_burgers.py:207-368) as ONE persistent launch per batch. The integration is the
// solver's (burgers_step.h: the same point update, DPP / LDS halo and record rule as burgers.hip, one workgroup of W waves per trajectory, P
// contiguous points per lane); what differs is where the forcing comes from and what is recorded.
//
// Forcing. The reference's f [N][t][s] is a sum of 8 separable terms, f[n][iv][g] = sum_j (amp_j X_j[g]) T_j[iv]. The kernel reads the two small
// tables AX [N][8][s] = amp_j X_j and TT [N][t][8] = T_j and forms a control interval's forcing in registers at the interval's start:
// fc = AX[0][g] TT[iv][0]; fc = fc + AX[j][g] TT[iv][j], j = 1..7, every operation a separate IEEE fp32 one -- the reference's own order
// (amp * exp_space * exp_time, the terms added one after another), hence its bits. With clamp set (alpha != 1) fc = clamp(fc alpha, -10, 10)
// (l.272-273). TT[n][iv][0..7] is wave-uniform and read through the scalar cache; the AX rows are coalesced and read in chunks of 8 points,
// 64 loads in flight and one wait per chunk. Nothing is prefetched across the step loop (it would hold 8 P registers through it). u0 [N][s] is dense: the reference's interpolation of it to s points is the identity.
//
// Records, already subsampled: u_rec [N][num_t + 1][cols] holds the columns g % sx == 0 of u0 and of every recorded row, f_rec [N][f_rows][cols]
// the forcing of the intervals iv % st == 0 at those columns (the reference's trajectory[:, :, ::sx] and f[:, ::st, ::sx]).
#include "burgers_step.h"

namespace {

typedef __attribute__((address_space(4))) float bg_const_float;      // constant address space: a wave-uniform address loads through the scalar cache

// x, as a value that exists only once y does: orders the loads addressed by x after the computation of y
__device__ __forceinline__ int bg_after(int x, float y) {
  asm volatile("" : "+v"(x) : "v"(y));
  return x;
}

struct BurgersGenP {
  const float* u0; const float* ax; const float* tt; float* u_rec; float* f_rec;
  int s, t;
  int steps, record_time, f_time, num_t, sub_s, st, f_rows, cols;      // sub_s = sx: the name burgers_step.h reads
  int clamp;
  float h, d, dm, dt, alpha;      // h = c / 2 with c = fp32(1 / (2 dx)); d, dm = fp32(visc / dx^2), fp32(-2 visc / dx^2); dt, alpha as fp32
};

template <int W, int P>
__global__ __launch_bounds__(W * 64) void burgers_generate_kernel(BurgersGenP p) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform: scalar branches below
  const int g0 = (w * 64 + lane) * P;
  const bool wave_full = (w + 1) * 64 * P <= p.s;        // no point of this wave is past the grid: nothing to re-zero
  const size_t n = blockIdx.x;
  __shared__ float halo[2][2][W + 1];
  bg_halo_init<W>(halo);

  float u[P], fc[P];
  const float* __restrict__ u0 = p.u0 + n * p.s;
#pragma unroll
  for (int k = 0; k < P; ++k) u[k] = g0 + k < p.s ? u0[g0 + k] : 0.f;
  float* __restrict__ out = p.u_rec + n * (size_t)(p.num_t + 1) * p.cols;
  bg_record<P>(u, g0, out, p);

  const float* __restrict__ ax = p.ax + n * 8 * (size_t)p.s;
  const float* __restrict__ tt = p.tt + n * (size_t)p.t * 8;
  float* __restrict__ f_out = p.f_rec + n * (size_t)p.f_rows * p.cols;
  int rec_left = p.record_time, row = 1, par = 0;
  int f_left = 1, f_row = 0;                               // intervals until the next recorded one; its row
  for (int iv = 0; iv < p.t; ++iv) {                       // t intervals cover the steps (checked on the host); with no steps only f is recorded
    {
      // the interval change costs memory latency, not work: the eight TT values come through the scalar cache, the 8 x C AX values of a chunk
      // of C points are all in flight before the first is used (indices clamped into the row, so no load sits in a branch). C = 8 keeps 64
      // values in flight: max(P / 8, 1) round trips per interval, no configuration spills, and those with P >= 16 need fewer registers than the solver's
      const bg_const_float* tk = (const bg_const_float*)(tt + (size_t)iv * 8);
      int gq = bg_opaque(g0);
      constexpr int C = P < 8 ? P : 8;
#pragma unroll
      for (int k0 = 0; k0 < P; k0 += C) {
        float a[8][C];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int c = 0; c < C; ++c) a[j][c] = ax[(size_t)j * p.s + min(gq + k0 + c, p.s - 1)];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float v = __fmul_rn(a[0][c], tk[0]);
#pragma unroll
          for (int j = 1; j < 8; ++j) v = __fadd_rn(v, __fmul_rn(a[j][c], tk[j]));
          if (p.clamp) v = fminf(fmaxf(__fmul_rn(v, p.alpha), -10.f), 10.f);
          fc[k0 + c] = gq + k0 + c < p.s ? v : 0.f;
        }
        gq = bg_after(gq, fc[k0 + C - 1]);          // the next chunk's loads are issued after this chunk's values are used, not all P x 8 at once
      }
    }
    if (--f_left == 0) {
      bg_record<P>(fc, g0, f_out + (size_t)f_row * p.cols, p);
      ++f_row;
      f_left = p.st;
    }
    const int j_end = min(p.steps, (iv + 1) * p.f_time);
    for (int j = iv * p.f_time; j < j_end; ++j) {
      BG_STEP();
      if (--rec_left == 0) {
        bg_record<P>(u, g0, out + (size_t)row * p.cols, p);
        ++row;
        rec_left = p.record_time;
      }
    }
  }
}

template <int W, int P>
int bgd_launch(const BurgersGenP& p, int N, hipStream_t st) {
  burgers_generate_kernel<W, P><<<N, W * 64, 0, st>>>(p);
  return wdno_check_launch();
}

template <int W>
int bgd_launch_w(const BurgersGenP& p, int N, int P, hipStream_t st) {
  switch (P) {
    case 2: return bgd_launch<W, 2>(p, N, st);
    case 4: return bgd_launch<W, 4>(p, N, st);
    case 8: return bgd_launch<W, 8>(p, N, st);
    case 16: return bgd_launch<W, 16>(p, N, st);
    case 32:
      if constexpr (W <= 8) return bgd_launch<W, 32>(p, N, st);      // the solver's configurations, no others
      break;
  }
  return WDNO_EUNSUPPORTED;
}

}  // namespace

extern "C" int wdno_burgers_generate(const float* u0, const float* ax, const float* tt, float* u_rec, float* f_rec,
                                     const wdno_burgers_generate_desc* d, wdno_stream_t s) {
  WDNO_REQUIRE(u0 && ax && tt && u_rec && f_rec && d && d->N > 0 && d->s > 0 && d->t > 0 && d->num_t >= 0 && d->st > 0 && d->sx > 0);
  WDNO_REQUIRE(d->cols == (d->s + d->sx - 1) / d->sx && d->f_rows == (d->t + d->st - 1) / d->st && d->steps >= 0);
  const int W = d->waves, P = d->points;
  if ((int64_t)W * 64 * P < d->s) return WDNO_EINVAL;
  if (d->steps > 0) {          // the host raises the reference's exceptions first; the kernel relies on these
    WDNO_REQUIRE(d->f_time > 0 && d->record_time > 0);
    WDNO_REQUIRE((d->steps - 1) / d->f_time < d->t && d->steps / d->record_time == d->num_t);
    WDNO_REQUIRE((int64_t)d->t * d->f_time < ((int64_t)1 << 31));
  }
  BurgersGenP p;
  p.u0 = u0; p.ax = ax; p.tt = tt; p.u_rec = u_rec; p.f_rec = f_rec;
  p.s = d->s; p.t = d->t;
  p.steps = d->steps; p.record_time = d->steps > 0 ? d->record_time : 1; p.f_time = d->steps > 0 ? d->f_time : 1;
  p.num_t = d->num_t; p.sub_s = d->sx; p.st = d->st; p.f_rows = d->f_rows; p.cols = d->cols;
  p.clamp = d->clamp != 0;
  p.h = 0.5f * d->c; p.d = d->d; p.dm = d->dm; p.dt = d->dt; p.alpha = d->alpha;
  hipStream_t st = as_stream(s);
  switch (W) {
    case 1: return bgd_launch_w<1>(p, d->N, P, st);
    case 2: return bgd_launch_w<2>(p, d->N, P, st);
    case 4: return bgd_launch_w<4>(p, d->N, P, st);
    case 8: return bgd_launch_w<8>(p, d->N, P, st);
    case 16: return bgd_launch_w<16>(p, d->N, P, st);
  }
  return WDNO_EUNSUPPORTED;
}
