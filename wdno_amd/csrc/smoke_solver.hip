// smoke_solver.hip -- the smoke control-evaluation solver (solver(), smoke/dataset/evaluate_solver.py:135-196, with the PhiFlow pieces it calls)
// as ONE persistent launch: one workgroup per simulation runs all 256 frames, each with its conjugate-gradient pressure solve (up to 500
// iterations on the 127 x 127 cell grid), the velocity projection, the advection of the two densities and the bucket sums. The reference runs
// one process per simulation, ~30 s each on a CPU.
//
// The steps it shares with the data-set generator (smoke_datagen.hip) -- the thread layout, the reductions, the stencil, the divergence, the CG
// pressure solve with its fp64 accumulation, the projection and the advection of a cell -- are in smoke_flow.h, where the layout is described.
// The loop bounds are the descriptor's frame and iteration counts (256 and 500): nothing in the kernel waits on another workgroup or spins.
// Interpolation weights and the bucket sums are fp64 (the reference interpolates in fp64 through scipy and sums the buckets in fp64).
#include "smoke_flow.h"

namespace {

using namespace smoke;

constexpr int NQ = 10;                // per-frame sums: 7 buckets, the union, the set-zero density before / after the bucket mask

struct SmokeP {
  const float* d0; const float* c1; const float* c2; const float* v0;
  const float* fluid; const float* active; const float* vmask; const float* buckets;
  const int* slot;
  float* dens; float* zdens; float* vel; double* ratio; float* ws;
  int nt, nx, ti, si, num_t, max_iter, n_out;
  float accuracy;
};

template <int NT>
__global__ __launch_bounds__(NT) void smoke_solve_kernel(SmokeP P) {
  constexpr int NW = NT / 64;          // waves
  constexpr int RR = SG / NW;          // rows per wave: 8 or 16
  constexpr int NGW = RR / 8;          // reduction groups per wave
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = w * RR, col0 = 2 * lane;
  const size_t n = blockIdx.x;

  __shared__ SmShared<NW, NQ> sh;
  if (threadIdx.x < 7) sh.outs[threadIdx.x] = 0.0;

  const SmWorkspace W = sm_workspace(P.ws, n);
  float2* __restrict__ velws = W.vel;
  const float* __restrict__ c1 = P.c1 + n * (size_t)P.nt * P.nx * P.nx;
  const float* __restrict__ c2 = P.c2 + n * (size_t)P.nt * P.nx * P.nx;
  const float2* __restrict__ vmask = reinterpret_cast<const float2*>(P.vmask);

  float dg[RR][2];
  bool act[RR][2];
  sm_stencil<RR>(P.fluid, P.active, row0, col0, dg, act);

  // initial state: velocity, the tiled density in both planes of buffer 0 (row / column 127 are zero in every buffer)
  {
    const float* __restrict__ d0 = P.d0 + n * (size_t)P.nx * P.nx;
    const float2* __restrict__ v0 = reinterpret_cast<const float2*>(P.v0);
#pragma unroll 1
    for (int k = 0; k < RR; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = row0 + k, j = col0 + e, c = i * SG + j;
        velws[c] = v0[c];
        const float d = (i < SN && j < SN) ? d0[(i / P.si) * P.nx + j / P.si] : 0.f;
        W.dbuf0[c] = d; W.dbuf0[SCELLS + c] = d;
        W.dbuf1[c] = 0.f; W.dbuf1[SCELLS + c] = 0.f;
      }
  }
  __syncthreads();

#pragma unroll 1
  for (int frame = 0; frame < P.num_t; ++frame) {
    // ---- the frame's velocity: interior from the previous frame, rim from the control; masked (evaluate_solver.py:89-101, flow.py:297)
    {
      const float* __restrict__ c1f = c1 + (size_t)(frame / P.ti) * P.nx * P.nx;
      const float* __restrict__ c2f = c2 + (size_t)(frame / P.ti) * P.nx * P.nx;
#pragma unroll 1
      for (int k = 0; k < RR; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int i = row0 + k, j = col0 + e, c = i * SG + j;
          float2 v;
          if (sm_interior(i, j)) {
            v = velws[c];
          } else {
            const int ci = (i / P.si) * P.nx + j / P.si;
            v = make_float2(c1f[ci], c2f[ci]);
          }
          const float2 m = vmask[c];
          velws[c] = make_float2(__fmul_rn(v.x, m.x), __fmul_rn(v.y, m.y));
        }
    }
    __syncthreads();

    // ---- divergence, CG, pressure to the workspace, then the projection
    sm_divergence<RR>(W, row0, col0);
    sm_pressure_solve<NT, NQ>(sh, dg, act, W, P.max_iter, P.accuracy, lane, w, row0, col0);
    __syncthreads();
    int oslot = P.slot[frame];
    oslot = oslot < P.n_out ? oslot : -1;
    const size_t obase = oslot >= 0 ? (n * P.n_out + oslot) * (size_t)SCELLS : 0;
    sm_project<RR>(W, vmask, row0, col0, [&](int, int, int c, float2 v) {
      if (oslot >= 0) reinterpret_cast<float2*>(P.vel)[obase + c] = v;
    });
    __syncthreads();

    // ---- advection of both densities and the per-frame sums
    const float* __restrict__ src = W.buffer(frame & 1);
    float* __restrict__ dst = W.buffer((frame & 1) ^ 1);
#pragma unroll 1
    for (int g = 0; g < NGW; ++g) {
      double s[NQ];
#pragma unroll
      for (int qn = 0; qn < NQ; ++qn) s[qn] = 0.0;
#pragma unroll 1
      for (int kk = 0; kk < 8; ++kk)
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
          const int i = row0 + g * 8 + kk, j = col0 + e, c = i * SG + j;
          float d, z;
          sm_advect_cell<false>(velws, src, i, j, c, d, z);
          dst[c] = d;
          dst[SCELLS + c] = z;
          if (oslot >= 0) P.dens[obase + c] = d;
          bool any = false;
#pragma unroll
          for (int b = 0; b < 7; ++b) {
            const float bm = P.buckets[b * SCELLS + c];
            s[b] += (double)d * (double)bm;
            any = any || bm != 0.f;
          }
          s[7] += any ? (double)d : 0.0;
          s[8] += (double)z;
          s[9] += (double)z * (double)P.buckets[7 * SCELLS + c];
        }
      sm_group_sums<NQ, NW>(sh, s, lane, w * NGW + g);
    }
    __syncthreads();
    double in_buckets = 0.0;
#pragma unroll
    for (int g = 0; g < NGROUP; ++g) in_buckets += sh.fred[7][g];
    const bool hit = in_buckets > 0.0;                        // evaluate_solver.py:173
#pragma unroll 1
    for (int k = 0; k < RR; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = (row0 + k) * SG + col0 + e;             // own cells: written above by this thread
        float z = dst[SCELLS + c];
        if (hit) z = __fmul_rn(z, P.buckets[7 * SCELLS + c]);  // evaluate_solver.py:176
        if (hit) dst[SCELLS + c] = z;
        if (oslot >= 0) P.zdens[obase + c] = z;
      }
    if (threadIdx.x == 0) {
      double tot = 0.0, zsum = 0.0;
      for (int b = 0; b < 7; ++b) {
        if (hit) {
          double sb = 0.0;
          for (int g = 0; g < NGROUP; ++g) sb += sh.fred[b][g];
          sh.outs[b] += sb;
        }
        tot += sh.outs[b];
      }
      for (int g = 0; g < NGROUP; ++g) zsum += sh.fred[hit ? 9 : 8][g];
      P.ratio[n * (size_t)P.num_t + frame] = sh.outs[1] / (tot + zsum);
    }
    __syncthreads();
  }
}

template <int NT>
int sm_launch(const SmokeP& p, int B, hipStream_t st) {
  smoke_solve_kernel<NT><<<B, NT, 0, st>>>(p);
  return wdno_check_launch();
}

}  // namespace

extern "C" int wdno_smoke_solve(const float* init_density, const float* c1, const float* c2, const float* init_velocity, const float* fluid_ext,
                                const float* active_ext, const float* velocity_mask, const float* buckets, const int* frame_slot, float* density,
                                float* zero_density, float* velocity, double* ratio, float* ws, const wdno_smoke_solve_desc* d, wdno_stream_t s) {
  WDNO_REQUIRE(init_density && c1 && c2 && init_velocity && fluid_ext && active_ext && velocity_mask && buckets && frame_slot && ratio && ws && d);
  WDNO_REQUIRE(d->B > 0 && d->nt > 0 && d->nx > 0 && d->time_interval > 0 && d->space_interval > 0);
  WDNO_REQUIRE(d->num_t > 0 && d->num_t <= 256 && d->max_iter >= 0 && d->max_iter <= 500 && d->n_out >= 0 && d->n_out <= d->num_t);
  WDNO_REQUIRE(d->nx * d->space_interval == SG && d->nt * d->time_interval >= d->num_t);          // every control index stays inside c1 / c2
  WDNO_REQUIRE(d->n_out == 0 || (density && zero_density && velocity));
  SmokeP p;
  p.d0 = init_density; p.c1 = c1; p.c2 = c2; p.v0 = init_velocity;
  p.fluid = fluid_ext; p.active = active_ext; p.vmask = velocity_mask; p.buckets = buckets; p.slot = frame_slot;
  p.dens = density; p.zdens = zero_density; p.vel = velocity; p.ratio = ratio; p.ws = ws;
  p.nt = d->nt; p.nx = d->nx; p.ti = d->time_interval; p.si = d->space_interval;
  p.num_t = d->num_t; p.max_iter = d->max_iter; p.n_out = d->n_out; p.accuracy = d->accuracy;
  hipStream_t st = as_stream(s);
  switch (d->threads) {
    case 1024: return sm_launch<1024>(p, d->B, st);
    case 512: return sm_launch<512>(p, d->B, st);
  }
  return WDNO_EUNSUPPORTED;
}
