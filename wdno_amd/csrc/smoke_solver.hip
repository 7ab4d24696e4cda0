// smoke_solver.hip -- the smoke control-evaluation solver (solver(), smoke/dataset/evaluate_solver.py:135-196, with the PhiFlow pieces it calls)
// as ONE persistent launch: one workgroup per simulation runs all 256 frames, each with its conjugate-gradient pressure solve (up to 500
// iterations on the 127 x 127 cell grid), the velocity projection, the advection of the two densities and the bucket sums. The reference runs
// one process per simulation, ~30 s each on a CPU.
//
// Layout. The cell grid is padded to 128 x 128. A workgroup of NT threads (1024 or 512) is NT / 64 waves; wave w owns the RR = 128 / (NT / 64)
// rows [w RR, (w + 1) RR) and lane l owns the two columns 2 l, 2 l + 1 of them: 2 RR cells a thread (16 or 32). During the CG loop x, r, p and
// A p of those cells stay in registers. A cell's left / right neighbours are in the thread itself or one lane away (DPP wave shifts, no LDS:
// a wave spans the whole row, so what lies beyond its end lanes is the inactive padding of the domain), its upper / lower neighbours are in the thread except
// for the first and last row of the wave, which come through a two-row LDS halo per wave. The stencil is data: per cell the diagonal
// min(-(fluid neighbours), -1) and one `active` bit (the coupling to a neighbour is active[self] * active[neighbour],
// phi/solver/sparse.py:51-53), derived once from the two extended masks the host passes. No obstacle layout is compiled in.
//
// One CG iteration is three barrier rounds: the halo of the masked direction vector; the reduction that delivers sum(p Ap), sum(p r) and
// max|r| together (the stopping test of the reference's loop condition and its step length); the reduction of sum(r Ap). Every reduction is a
// thread's sequential fp32 sum over an 8-row group of its cells, an fp32 butterfly over the wave (DPP), and an fp64 sum of the sixteen
// (group) results in index order by every thread from LDS -- the same order for both workgroup sizes, so a simulation's bits depend on
// neither the configuration, the batch nor its position in it, and every wave takes the same stopping decision. The loop bounds are the
// descriptor's frame and iteration counts (256 and 500): nothing in the kernel waits on another workgroup or spins.
//
// The per-frame steps around the CG loop run once per 500 iterations and go through a per-simulation workspace in global memory (L2):
// velocity [128][128][2], pressure [128][128], two buffers of the two densities, and the fp64 accumulator of the pressure (the sum of the CG
// steps a p is kept in fp32 registers for 16 iterations at a time and added to it: the reference's fp32 `pressure += a * momentum` loses
// most of its accuracy in exactly that sum). Interpolation weights and the bucket sums are fp64 (the
// reference interpolates in fp64 through scipy and sums the buckets in fp64).
#include "common.h"

namespace {

constexpr int SG = 128;               // staggered grid / padded cell grid
constexpr int SN = 127;               // cells per side
constexpr int SE = 129;               // extended masks
constexpr int SCELLS = SG * SG;
constexpr int NGROUP = 16;            // 8-row reduction groups
constexpr int WS_PLANES = 9;          // velocity (2), pressure, two buffers of two densities (4), the fp64 pressure accumulator (2)
constexpr int XFLUSH = 16;            // CG iterations between two flushes of the fp32 pressure increments into the fp64 accumulator
constexpr int NQ = 10;                // per-frame sums: 7 buckets, the union, the set-zero density before / after the bucket mask

struct SmokeP {
  const float* d0; const float* c1; const float* c2; const float* v0;
  const float* fluid; const float* active; const float* vmask; const float* buckets;
  const int* slot;
  float* dens; float* zdens; float* vel; double* ratio; float* ws;
  int nt, nx, ti, si, num_t, max_iter, n_out;
  float accuracy;
};

template <int CTRL>
__device__ __forceinline__ float sm_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// the value of lane l - 1 / l + 1 (wave_shr:1 / wave_shl:1), 0 where there is none
__device__ __forceinline__ float sm_prev_lane(float v) { return sm_dpp<0x138>(v); }
__device__ __forceinline__ float sm_next_lane(float v) { return sm_dpp<0x130>(v); }

__device__ __forceinline__ float sm_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// fp32 butterfly over the 64 lanes in a fixed order: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror, then the four rows
__device__ __forceinline__ float sm_wave_sum(float v) {
  v = __fadd_rn(v, sm_dpp<0xB1>(v));
  v = __fadd_rn(v, sm_dpp<0x4E>(v));
  v = __fadd_rn(v, sm_dpp<0x141>(v));
  v = __fadd_rn(v, sm_dpp<0x140>(v));
  const float a = sm_lane(v, 0), b = sm_lane(v, 16), c = sm_lane(v, 32), d = sm_lane(v, 48);
  return __fadd_rn(__fadd_rn(a, b), __fadd_rn(c, d));
}
__device__ __forceinline__ float sm_wave_max(float v) {
  v = fmaxf(v, sm_dpp<0xB1>(v));
  v = fmaxf(v, sm_dpp<0x4E>(v));
  v = fmaxf(v, sm_dpp<0x141>(v));
  v = fmaxf(v, sm_dpp<0x140>(v));
  const float a = sm_lane(v, 0), b = sm_lane(v, 16), c = sm_lane(v, 32), d = sm_lane(v, 48);
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
}

__device__ __forceinline__ int sm_clamp(int i) { return i < 0 ? 0 : (i > SN - 1 ? SN - 1 : i); }

// linear interpolation of a [128]-strided 127 x 127 field at the clamped coordinates (yi, xj): scipy's interpn with fill_value 0 past 126
__device__ __forceinline__ float sm_sample(const float* __restrict__ f, float yi, float xj) {
  if (yi > (float)(SN - 1) || xj > (float)(SN - 1)) return 0.f;
  int i0 = (int)floorf(yi), j0 = (int)floorf(xj);
  i0 = i0 > SN - 2 ? SN - 2 : i0;
  j0 = j0 > SN - 2 ? SN - 2 : j0;
  const double wy = (double)yi - (double)i0, wx = (double)xj - (double)j0;
  const double f00 = f[i0 * SG + j0], f01 = f[i0 * SG + j0 + 1], f10 = f[(i0 + 1) * SG + j0], f11 = f[(i0 + 1) * SG + j0 + 1];
  return (float)(((1.0 - wy) * (1.0 - wx) * f00 + (1.0 - wy) * wx * f01) + (wy * (1.0 - wx) * f10 + wy * wx * f11));
}

// The fp32 pressure increments of this thread's cells, x, meet their fp64 total, xacc. The registers go through the pressure plane and a
// rolled loop, so that nothing beside x is live (each thread touches its own cells only: no barrier). LAST: the plane receives
// fp32(xacc + x), the frame's pressure; otherwise xacc += x and x starts again from 0.
template <int RR, bool LAST>
__device__ __forceinline__ void sm_flush_x(float (&x)[RR][2], float* __restrict__ prws, double* __restrict__ xacc, int row0, int col0) {
#pragma unroll
  for (int k = 0; k < RR; ++k) {
    *reinterpret_cast<float2*>(&prws[(row0 + k) * SG + col0]) = make_float2(x[k][0], x[k][1]);
    x[k][0] = 0.f; x[k][1] = 0.f;
  }
#pragma unroll 1
  for (int k = 0; k < RR; ++k) {
    const int c = (row0 + k) * SG + col0;
    const float2 part = *reinterpret_cast<const float2*>(&prws[c]);
    double2 t = *reinterpret_cast<const double2*>(&xacc[c]);
    t.x += (double)part.x; t.y += (double)part.y;
    if (LAST) *reinterpret_cast<float2*>(&prws[c]) = make_float2((float)t.x, (float)t.y);
    else *reinterpret_cast<double2*>(&xacc[c]) = t;
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void smoke_solve_kernel(SmokeP P) {
  constexpr int NW = NT / 64;          // waves
  constexpr int RR = SG / NW;          // rows per wave: 8 or 16
  constexpr int NGW = RR / 8;          // reduction groups per wave
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = w * RR, col0 = 2 * lane;
  const size_t n = blockIdx.x;

  __shared__ float halo_top[NW][SG], halo_bot[NW][SG];     // masked direction vector: first / last row of every wave
  __shared__ float red1[3][NGROUP], red2[NGROUP];
  __shared__ double fred[NQ][NGROUP];
  __shared__ double outs[7];
  if (threadIdx.x < 7) outs[threadIdx.x] = 0.0;

  float* __restrict__ ws = P.ws + n * (size_t)(WS_PLANES * SCELLS);
  float2* __restrict__ velws = reinterpret_cast<float2*>(ws);              // [128][128] (x, y)
  float* __restrict__ prws = ws + 2 * SCELLS;
  float* __restrict__ dbuf[2] = {ws + 3 * SCELLS, ws + 5 * SCELLS};        // each: density plane, set-zero density plane
  double* __restrict__ xacc = reinterpret_cast<double*>(ws + 7 * SCELLS);  // [128][128]: this thread's cells only
  const float* __restrict__ c1 = P.c1 + n * (size_t)P.nt * P.nx * P.nx;
  const float* __restrict__ c2 = P.c2 + n * (size_t)P.nt * P.nx * P.nx;
  const float2* __restrict__ vmask = reinterpret_cast<const float2*>(P.vmask);

  // the stencil of this thread's cells; padded cells (row or column 127) are inactive with diagonal -1
  float dg[RR][2];
  bool act[RR][2];
#pragma unroll
  for (int k = 0; k < RR; ++k)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = row0 + k, j = col0 + e;
      dg[k][e] = -1.f;
      act[k][e] = false;
      if (i < SN && j < SN) {
        const float* __restrict__ fe = P.fluid + (i + 1) * SE + (j + 1);
        const float cnt = (fe[SE] + fe[-SE]) + (fe[1] + fe[-1]);
        dg[k][e] = -fmaxf(cnt, 1.f);
        act[k][e] = P.active[(i + 1) * SE + (j + 1)] != 0.f;
      }
    }

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
        dbuf[0][c] = d; dbuf[0][SCELLS + c] = d;
        dbuf[1][c] = 0.f; dbuf[1][SCELLS + c] = 0.f;
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
          if (i >= 16 && i < 112 && j >= 16 && j < 112) {
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

    // ---- divergence (nd.py:367-377) = the CG's right-hand side, through the pressure plane of the workspace (own cells only)
#pragma unroll 1
    for (int k = 0; k < RR; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = row0 + k, j = col0 + e, c = i * SG + j;
        float d = 0.f;
        if (i < SN && j < SN) {
          const float2 v = velws[c];
          d = __fadd_rn(__fadd_rn(velws[c + SG].y, -v.y), __fadd_rn(velws[c + 1].x, -v.x));
        }
        prws[c] = d;
        xacc[c] = 0.0;
      }
    float x[RR][2], r[RR][2], p[RR][2], Ap[RR][2];
#pragma unroll
    for (int k = 0; k < RR; ++k) {
      const float2 d = *reinterpret_cast<const float2*>(&prws[(row0 + k) * SG + col0]);
      x[k][0] = 0.f; x[k][1] = 0.f;
      r[k][0] = d.x; r[k][1] = d.y;
      p[k][0] = d.x; p[k][1] = d.y;
    }

    // ---- conjugate gradient (phi/solver/base.py:56-103): x = 0, r = p = div
#pragma unroll 1
    for (int it = 0; it < P.max_iter; ++it) {
      float q[RR][2];
#pragma unroll
      for (int k = 0; k < RR; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e) q[k][e] = act[k][e] ? p[k][e] : 0.f;
      *reinterpret_cast<float2*>(&halo_top[w][col0]) = make_float2(q[0][0], q[0][1]);
      *reinterpret_cast<float2*>(&halo_bot[w][col0]) = make_float2(q[RR - 1][0], q[RR - 1][1]);
      __syncthreads();
      float2 up = make_float2(0.f, 0.f), dn = make_float2(0.f, 0.f);
      if (w > 0) up = *reinterpret_cast<const float2*>(&halo_bot[w - 1][col0]);
      if (w < NW - 1) dn = *reinterpret_cast<const float2*>(&halo_top[w + 1][col0]);
      float mr = 0.f;
#pragma unroll
      for (int g = 0; g < NGW; ++g) {
        float s_pap = 0.f, s_pr = 0.f;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const int k = g * 8 + kk;
          const float u0 = k > 0 ? q[k - 1][0] : up.x, u1 = k > 0 ? q[k - 1][1] : up.y;
          const float l0 = k < RR - 1 ? q[k + 1][0] : dn.x, l1 = k < RR - 1 ? q[k + 1][1] : dn.y;
          const float left0 = sm_prev_lane(q[k][1]), right1 = sm_next_lane(q[k][0]);
          const float nb0 = __fadd_rn(__fadd_rn(u0, l0), __fadd_rn(left0, q[k][1]));
          const float nb1 = __fadd_rn(__fadd_rn(u1, l1), __fadd_rn(q[k][0], right1));
          Ap[k][0] = __fmaf_rn(dg[k][0], p[k][0], act[k][0] ? nb0 : 0.f);
          Ap[k][1] = __fmaf_rn(dg[k][1], p[k][1], act[k][1] ? nb1 : 0.f);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            s_pap = __fmaf_rn(p[k][e], Ap[k][e], s_pap);
            s_pr = __fmaf_rn(p[k][e], r[k][e], s_pr);
            mr = fmaxf(mr, fabsf(r[k][e]));
          }
        }
        s_pap = sm_wave_sum(s_pap);
        s_pr = sm_wave_sum(s_pr);
        if (lane == 0) { red1[0][w * NGW + g] = s_pap; red1[1][w * NGW + g] = s_pr; }
      }
      mr = sm_wave_max(mr);
      if (lane == 0) {
#pragma unroll
        for (int g = 0; g < NGW; ++g) red1[2][w * NGW + g] = mr;
      }
      __syncthreads();
      double tmp = 0.0, pr = 0.0;
      float maxr = 0.f;
#pragma unroll
      for (int g = 0; g < NGROUP; ++g) {
        tmp += (double)red1[0][g];
        pr += (double)red1[1][g];
        maxr = fmaxf(maxr, red1[2][g]);
      }
      if (!(maxr >= P.accuracy) || tmp == 0.0) break;       // the same LDS values in every thread: one decision for the workgroup
      const float a = (float)(pr / tmp);
#pragma unroll
      for (int g = 0; g < NGW; ++g) {
        float s_rap = 0.f;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int k = g * 8 + kk;
            x[k][e] = __fmaf_rn(a, p[k][e], x[k][e]);
            r[k][e] = __fmaf_rn(-a, Ap[k][e], r[k][e]);
            s_rap = __fmaf_rn(r[k][e], Ap[k][e], s_rap);
          }
        s_rap = sm_wave_sum(s_rap);
        if (lane == 0) red2[w * NGW + g] = s_rap;
      }
      __syncthreads();
      double rap = 0.0;
#pragma unroll
      for (int g = 0; g < NGROUP; ++g) rap += (double)red2[g];
      const float b = (float)(-rap / tmp);
      // the reference's first pass: `momentum` IS `residual` there, so the old direction it scales is the updated residual
      if (it == 0) {
#pragma unroll
        for (int k = 0; k < RR; ++k) { p[k][0] = r[k][0]; p[k][1] = r[k][1]; }
      }
#pragma unroll
      for (int k = 0; k < RR; ++k)
#pragma unroll
        for (int e = 0; e < 2; ++e) p[k][e] = __fmaf_rn(b, p[k][e], r[k][e]);
      // x = sum of the steps a p is an accumulation: the fp32 registers hold the last XFLUSH steps only, the total is fp64
      if ((it & (XFLUSH - 1)) == XFLUSH - 1) sm_flush_x<RR, false>(x, prws, xacc, row0, col0);
    }

    // ---- pressure to the workspace, then v = (v - mask grad p) mask (flow.py:322-327, nd.py:603-614: symmetric padding)
    sm_flush_x<RR, true>(x, prws, xacc, row0, col0);
    __syncthreads();
    int oslot = P.slot[frame];
    oslot = oslot < P.n_out ? oslot : -1;
    const size_t obase = oslot >= 0 ? (n * P.n_out + oslot) * (size_t)SCELLS : 0;
#pragma unroll 1
    for (int k = 0; k < RR; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = row0 + k, j = col0 + e, c = i * SG + j;
        const int ic = sm_clamp(i), jc = sm_clamp(j);
        const float pc = prws[ic * SG + jc], pl = prws[ic * SG + sm_clamp(j - 1)], pu = prws[sm_clamp(i - 1) * SG + jc];
        const float2 m = vmask[c];
        float2 v = velws[c];
        v.x = __fmul_rn(__fadd_rn(v.x, -__fmul_rn(__fadd_rn(pc, -pl), m.x)), m.x);
        v.y = __fmul_rn(__fadd_rn(v.y, -__fmul_rn(__fadd_rn(pc, -pu), m.y)), m.y);
        velws[c] = v;
        if (oslot >= 0) reinterpret_cast<float2*>(P.vel)[obase + c] = v;
      }
    __syncthreads();

    // ---- advection of both densities (nd.py:422-427, scipy_backend.py:58-78) and the per-frame sums
    const float* __restrict__ src = dbuf[frame & 1];
    float* __restrict__ dst = dbuf[(frame & 1) ^ 1];
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
          float d = 0.f, z = 0.f;
          if (i < SN && j < SN) {
            const float2 v = velws[c];
            const float cy = __fmul_rn(__fadd_rn(velws[c + SG].y, v.y), 0.5f), cx = __fmul_rn(__fadd_rn(velws[c + 1].x, v.x), 0.5f);
            const float yi = fmaxf(0.f, fminf((float)SN, __fadd_rn((float)i, -cy)));
            const float xj = fmaxf(0.f, fminf((float)SN, __fadd_rn((float)j, -cx)));
            d = sm_sample(src, yi, xj);
            z = sm_sample(src + SCELLS, yi, xj);
          }
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
#pragma unroll
      for (int qn = 0; qn < NQ; ++qn) {
        const double t = wave_sum_d(s[qn]);
        if (lane == 0) fred[qn][w * NGW + g] = t;
      }
    }
    __syncthreads();
    double in_buckets = 0.0;
#pragma unroll
    for (int g = 0; g < NGROUP; ++g) in_buckets += fred[7][g];
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
          for (int g = 0; g < NGROUP; ++g) sb += fred[b][g];
          outs[b] += sb;
        }
        tot += outs[b];
      }
      for (int g = 0; g < NGROUP; ++g) zsum += fred[hit ? 9 : 8][g];
      P.ratio[n * (size_t)P.num_t + frame] = outs[1] / (tot + zsum);
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
