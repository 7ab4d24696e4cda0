// burgers.hip -- the Burgers control-evaluation solver (burgers_numeric_solve_free, burgers/ddpm_burgers/generate_burgers.py:104-204) as ONE
// persistent launch: the whole explicit-Euler integration (614 400 steps at T = 8) of a trajectory runs inside one workgroup, with its state in
// registers. The reference runs the same loop as ~15 torch ops per step.
//
// Layout. One workgroup of W waves per trajectory; lane l of wave w holds the P contiguous interior points g = (64 w + l) P + k, k < P
// (64 W P >= s). Points g >= s are kept at 0 every step: the first of them is the right Dirichlet ghost, the left ghost is the 0 that lane 0 of
// wave 0 reads. Neighbours across lanes come through DPP wave shifts (no LDS); across waves through a small LDS array, double-buffered by the
// step's parity, so that one barrier per step suffices (a wave that has passed barrier j + 1 writes buffer (j + 2) & 1 only after every wave has
// read buffer j & 1). W = 1: no LDS, no barrier.
//
// Arithmetic. Every point's update is the same fixed sequence of IEEE fp32 operations (no contraction), so a trajectory's result does not depend
// on W, P, the batch or its position in it. It is the reference's own order (generate_burgers.py:179-186: einsum over the [-1, 1] / 2dx and
// [1, -2, 1] visc / dx^2 stencil rows, then u + dt (-(1/2) transport + diffusion + f)) with one exact rewrite: -(1/2)(-c a^2 + c e^2) is
// computed as (c/2) a^2 + (-c/2) e^2 (scaling by a power of two commutes with rounding outside the subnormal range).
//
// Forcing. f [N][Nt_f][nxf] is interpolated to s points inside the kernel (torch's linear, align_corners = False: src = max((i + 0.5) nxf / s
// - 0.5, 0)), once per control interval; the coarse values of the next interval are loaded while the current one runs. u0 likewise.
// Records go straight into out [N][num_t + 1][out_cols] (only the columns g % sub_s == 0).
//
// The step itself (point update, halo, record rule) is in burgers_step.h, shared with burgers_datagen.hip.
#include "burgers_step.h"

namespace {

struct BurgersP {
  const float* u0; const float* f; float* out;
  int s, nx0, nt_f, nxf;
  int steps, record_time, f_time, num_t, sub_s, out_cols;
  float h, d, dm, dt;             // h = c / 2 with c = fp32(1 / (2 dx)); d, dm = fp32(visc / dx^2), fp32(-2 visc / dx^2); dt as fp32
  float scale_u, scale_f;         // fp32(nx0) / fp32(s), fp32(nxf) / fp32(s): torch's area_pixel_compute_scale
};

// torch's linear interpolation (align_corners = False) of point g of a line x of n values resampled to s points
__device__ __forceinline__ void bg_src(int g, int n, float scale, int& i0, int& i1, float& lam) {
  float src = __fadd_rn(__fmul_rn(scale, __fadd_rn((float)g, 0.5f)), -0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = min((int)floorf(src), n - 1);
  lam = fminf(fmaxf(__fadd_rn(src, -(float)i0), 0.f), 1.f);
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
}
__device__ __forceinline__ float bg_mix(float x0, float x1, float lam) {
  return __fadd_rn(__fmul_rn(x0, __fadd_rn(1.f, -lam)), __fmul_rn(x1, lam));
}

template <int W, int P>
__global__ __launch_bounds__(W * 64) void burgers_solve_kernel(BurgersP p) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform: scalar branches below
  const int g0 = (w * 64 + lane) * P;
  const bool wave_full = (w + 1) * 64 * P <= p.s;        // no point of this wave is past the grid: nothing to re-zero
  const size_t n = blockIdx.x;
  __shared__ float halo[2][2][W + 1];
  bg_halo_init<W>(halo);

  float u[P], fc[P], x0n[P], x1n[P];
  const float* __restrict__ u0 = p.u0 + n * p.nx0;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    int i0, i1; float lam;
    bg_src(g0 + k, p.nx0, p.scale_u, i0, i1, lam);
    u[k] = g0 + k < p.s ? bg_mix(u0[i0], u0[i1], lam) : 0.f;
  }
  float* __restrict__ out = p.out + n * (size_t)(p.num_t + 1) * p.out_cols;
  bg_record<P>(u, g0, out, p);

  const float* __restrict__ fn = p.f + n * (size_t)p.nt_f * p.nxf;
  const int n_iv = p.steps > 0 ? (p.steps + p.f_time - 1) / p.f_time : 0;          // control intervals used (<= Nt_f: checked on the host)
#pragma unroll
  for (int k = 0; k < P; ++k) {                                                    // interval 0
    int i0, i1; float lam;
    bg_src(g0 + k, p.nxf, p.scale_f, i0, i1, lam);
    fc[k] = g0 + k < p.s ? bg_mix(fn[i0], fn[i1], lam) : 0.f;
  }
  int rec_left = p.record_time, row = 1, par = 0;
  for (int iv = 0; iv < n_iv; ++iv) {
    const bool more = iv + 1 < n_iv;
    if (more) {                                                                    // the next interval's coarse values, in flight meanwhile
      const float* __restrict__ fr = fn + (size_t)(iv + 1) * p.nxf;
      const int gq = bg_opaque(g0);
#pragma unroll
      for (int k = 0; k < P; ++k) {
        int i0, i1; float lam;
        bg_src(gq + k, p.nxf, p.scale_f, i0, i1, lam);
        x0n[k] = fr[i0];
        x1n[k] = fr[i1];
      }
    }
    const int j_end = min(p.steps, (iv + 1) * p.f_time);
    for (int j = iv * p.f_time; j < j_end; ++j) {
      BG_STEP();
      if (--rec_left == 0) {
        bg_record<P>(u, g0, out + (size_t)row * p.out_cols, p);
        ++row;
        rec_left = p.record_time;
      }
    }
    if (more) {
      const int gq = bg_opaque(g0);
#pragma unroll
      for (int k = 0; k < P; ++k) {
        int i0, i1; float lam;
        bg_src(gq + k, p.nxf, p.scale_f, i0, i1, lam);
        fc[k] = gq + k < p.s ? bg_mix(x0n[k], x1n[k], lam) : 0.f;
      }
    }
  }
}

template <int W, int P>
int bg_launch(const BurgersP& p, int N, hipStream_t st) {
  burgers_solve_kernel<W, P><<<N, W * 64, 0, st>>>(p);
  return wdno_check_launch();
}

template <int W>
int bg_launch_w(const BurgersP& p, int N, int P, hipStream_t st) {
  switch (P) {
    case 2: return bg_launch<W, 2>(p, N, st);
    case 4: return bg_launch<W, 4>(p, N, st);
    case 8: return bg_launch<W, 8>(p, N, st);
    case 16: return bg_launch<W, 16>(p, N, st);
    case 32:
      if constexpr (W <= 8) return bg_launch<W, 32>(p, N, st);      // 16 waves x 32 points would need more than 128 VGPRs a lane
      break;
  }
  return WDNO_EUNSUPPORTED;
}

}  // namespace

extern "C" int wdno_burgers_solve(const float* u0, const float* f, float* out, const wdno_burgers_desc* d, wdno_stream_t s) {
  WDNO_REQUIRE(u0 && f && out && d && d->N > 0 && d->s > 0 && d->nx0 > 0 && d->nt_f > 0 && d->nxf > 0 && d->num_t >= 0 && d->sub_s > 0);
  WDNO_REQUIRE(d->out_cols == (d->s + d->sub_s - 1) / d->sub_s && d->steps >= 0);
  const int W = d->waves, P = d->points;
  if ((int64_t)W * 64 * P < d->s) return WDNO_EINVAL;
  if (d->steps > 0) {          // the host raises the reference's exceptions first; the kernel relies on these
    WDNO_REQUIRE(d->f_time > 0 && d->record_time > 0);
    WDNO_REQUIRE((d->steps - 1) / d->f_time < d->nt_f && d->steps / d->record_time == d->num_t);
  }
  BurgersP p;
  p.u0 = u0; p.f = f; p.out = out;
  p.s = d->s; p.nx0 = d->nx0; p.nt_f = d->nt_f; p.nxf = d->nxf;
  p.steps = d->steps; p.record_time = d->steps > 0 ? d->record_time : 1; p.f_time = d->steps > 0 ? d->f_time : 1;
  p.num_t = d->num_t; p.sub_s = d->sub_s; p.out_cols = d->out_cols;
  p.h = 0.5f * d->c; p.d = d->d; p.dm = d->dm; p.dt = d->dt;
  p.scale_u = (float)d->nx0 / (float)d->s;
  p.scale_f = (float)d->nxf / (float)d->s;
  hipStream_t st = as_stream(s);
  switch (W) {
    case 1: return bg_launch_w<1>(p, d->N, P, st);
    case 2: return bg_launch_w<2>(p, d->N, P, st);
    case 4: return bg_launch_w<4>(p, d->N, P, st);
    case 8: return bg_launch_w<8>(p, d->N, P, st);
    case 16: return bg_launch_w<16>(p, d->N, P, st);
  }
  return WDNO_EUNSUPPORTED;
}
