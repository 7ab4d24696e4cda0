// smoke_flow.h -- the steps of one smoke frame that the control-evaluation solver (smoke_solver.hip) and the data-set generator
// (smoke_datagen.hip) share, each written once: the thread layout, the DPP reductions, the stencil, the divergence, the conjugate-gradient
// pressure solve with its fp64 accumulation, the projection and the advection of one cell. Both kernels run one workgroup per simulation;
// what differs between them (where the rim of a frame's velocity comes from, the bucket rule, what is written out) stays in their files.
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
// neither the configuration, the batch nor its position in it, and every wave takes the same stopping decision.
//
// The per-frame steps around the CG loop go through a per-simulation workspace in global memory (L2): velocity [128][128][2], pressure
// [128][128], two buffers of the two densities, and the fp64 accumulator of the pressure (the sum of the CG steps a p is kept in fp32
// registers for 16 iterations at a time and added to it: the reference's fp32 `pressure += a * momentum` loses most of its accuracy in
// exactly that sum). Interpolation weights are fp64 (the reference interpolates in fp64 through scipy).
#pragma once
#include "common.h"

namespace smoke {

constexpr int SG = 128;               // staggered grid / padded cell grid
constexpr int SN = 127;               // cells per side
constexpr int SE = 129;               // extended masks
constexpr int SCELLS = SG * SG;
constexpr int NGROUP = 16;            // 8-row reduction groups
constexpr int WS_PLANES = 9;          // velocity (2), pressure, two buffers of two densities (4), the fp64 pressure accumulator (2)
constexpr int XFLUSH = 16;            // CG iterations between two flushes of the fp32 pressure increments into the fp64 accumulator

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

// the 16-cell rim of the staggered grid: the cells a control (or the generator's random walk) sets
__device__ __forceinline__ bool sm_interior(int i, int j) { return i >= 16 && i < 112 && j >= 16 && j < 112; }

// linear interpolation of a [128]-strided 127 x 127 field at the clamped coordinates (yi, xj): scipy's interpn with fill_value 0 past 126.
// T is the type the coordinates were computed in (float: the reference's, double: see sm_advect_cell); the weights are fp64 either way.
template <class T>
__device__ __forceinline__ float sm_sample(const float* __restrict__ f, T yi, T xj) {
  if (yi > (T)(SN - 1) || xj > (T)(SN - 1)) return 0.f;
  int i0 = (int)floor(yi), j0 = (int)floor(xj);
  i0 = i0 > SN - 2 ? SN - 2 : i0;
  j0 = j0 > SN - 2 ? SN - 2 : j0;
  const double wy = (double)yi - (double)i0, wx = (double)xj - (double)j0;
  const double f00 = f[i0 * SG + j0], f01 = f[i0 * SG + j0 + 1], f10 = f[(i0 + 1) * SG + j0], f11 = f[(i0 + 1) * SG + j0 + 1];
  return (float)(((1.0 - wy) * (1.0 - wx) * f00 + (1.0 - wy) * wx * f01) + (wy * (1.0 - wx) * f10 + wy * wx * f11));
}

// The LDS of one workgroup: the halo rows of the CG, its reductions, and NQ per-frame fp64 sums of the kernel that uses it.
template <int NW, int NQ>
struct SmShared {
  float halo_top[NW][SG], halo_bot[NW][SG];     // masked direction vector: first / last row of every wave
  float red1[3][NGROUP], red2[NGROUP];
  double fred[NQ][NGROUP];
  double outs[7];
};

// the workspace of simulation n
struct SmWorkspace {
  float2* __restrict__ vel;            // [128][128] (x, y)
  float* __restrict__ pr;              // pressure plane
  float* __restrict__ dbuf0;           // the two buffers, each: density plane, set-zero density plane
  float* __restrict__ dbuf1;
  __device__ __forceinline__ float* buffer(int which) const { return which ? dbuf1 : dbuf0; }
  double* __restrict__ xacc;           // [128][128]: a thread's own cells only
};
__device__ __forceinline__ SmWorkspace sm_workspace(float* ws_all, size_t n) {
  float* ws = ws_all + n * (size_t)(WS_PLANES * SCELLS);
  SmWorkspace W;
  W.vel = reinterpret_cast<float2*>(ws);
  W.pr = ws + 2 * SCELLS;
  W.dbuf0 = ws + 3 * SCELLS;
  W.dbuf1 = ws + 5 * SCELLS;
  W.xacc = reinterpret_cast<double*>(ws + 7 * SCELLS);
  return W;
}

// the stencil of this thread's cells; padded cells (row or column 127) are inactive with diagonal -1
template <int RR>
__device__ __forceinline__ void sm_stencil(const float* __restrict__ fluid, const float* __restrict__ active, int row0, int col0,
                                           float (&dg)[RR][2], bool (&act)[RR][2]) {
#pragma unroll
  for (int k = 0; k < RR; ++k)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = row0 + k, j = col0 + e;
      dg[k][e] = -1.f;
      act[k][e] = false;
      if (i < SN && j < SN) {
        const float* __restrict__ fe = fluid + (i + 1) * SE + (j + 1);
        const float cnt = (fe[SE] + fe[-SE]) + (fe[1] + fe[-1]);
        dg[k][e] = -fmaxf(cnt, 1.f);
        act[k][e] = active[(i + 1) * SE + (j + 1)] != 0.f;
      }
    }
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

// divergence (nd.py:367-377) = the CG's right-hand side, into the pressure plane of the workspace (own cells only); the fp64 total starts at 0
template <int RR>
__device__ __forceinline__ void sm_divergence(const SmWorkspace& W, int row0, int col0) {
#pragma unroll 1
  for (int k = 0; k < RR; ++k)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = row0 + k, j = col0 + e, c = i * SG + j;
      float d = 0.f;
      if (i < SN && j < SN) {
        const float2 v = W.vel[c];
        d = __fadd_rn(__fadd_rn(W.vel[c + SG].y, -v.y), __fadd_rn(W.vel[c + 1].x, -v.x));
      }
      W.pr[c] = d;
      W.xacc[c] = 0.0;
    }
}

// Conjugate gradient (phi/solver/base.py:56-103) on the right-hand side in the pressure plane: x = 0, r = p = rhs, until max|r| < accuracy
// or max_iter iterations; leaves the pressure, fp32(the fp64 sum of the steps), in the pressure plane. Ends with the writes of a thread's
// own cells: the caller puts a barrier before anybody reads a neighbour's pressure.
template <int NT, int NQ>
__device__ __forceinline__ void sm_pressure_solve(SmShared<NT / 64, NQ>& sh, const float (&dg)[SG / (NT / 64)][2], const bool (&act)[SG / (NT / 64)][2],
                                                  const SmWorkspace& W, int max_iter, float accuracy, int lane, int w, int row0, int col0) {
  constexpr int NW = NT / 64;          // waves
  constexpr int RR = SG / NW;          // rows per wave: 8 or 16
  constexpr int NGW = RR / 8;          // reduction groups per wave
  float* __restrict__ prws = W.pr;
  double* __restrict__ xacc = W.xacc;
  float x[RR][2], r[RR][2], p[RR][2], Ap[RR][2];
#pragma unroll
  for (int k = 0; k < RR; ++k) {
    const float2 d = *reinterpret_cast<const float2*>(&prws[(row0 + k) * SG + col0]);
    x[k][0] = 0.f; x[k][1] = 0.f;
    r[k][0] = d.x; r[k][1] = d.y;
    p[k][0] = d.x; p[k][1] = d.y;
  }

#pragma unroll 1
  for (int it = 0; it < max_iter; ++it) {
    float q[RR][2];
#pragma unroll
    for (int k = 0; k < RR; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) q[k][e] = act[k][e] ? p[k][e] : 0.f;
    *reinterpret_cast<float2*>(&sh.halo_top[w][col0]) = make_float2(q[0][0], q[0][1]);
    *reinterpret_cast<float2*>(&sh.halo_bot[w][col0]) = make_float2(q[RR - 1][0], q[RR - 1][1]);
    __syncthreads();
    float2 up = make_float2(0.f, 0.f), dn = make_float2(0.f, 0.f);
    if (w > 0) up = *reinterpret_cast<const float2*>(&sh.halo_bot[w - 1][col0]);
    if (w < NW - 1) dn = *reinterpret_cast<const float2*>(&sh.halo_top[w + 1][col0]);
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
      if (lane == 0) { sh.red1[0][w * NGW + g] = s_pap; sh.red1[1][w * NGW + g] = s_pr; }
    }
    mr = sm_wave_max(mr);
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < NGW; ++g) sh.red1[2][w * NGW + g] = mr;
    }
    __syncthreads();
    double tmp = 0.0, pr = 0.0;
    float maxr = 0.f;
#pragma unroll
    for (int g = 0; g < NGROUP; ++g) {
      tmp += (double)sh.red1[0][g];
      pr += (double)sh.red1[1][g];
      maxr = fmaxf(maxr, sh.red1[2][g]);
    }
    if (!(maxr >= accuracy) || tmp == 0.0) break;       // the same LDS values in every thread: one decision for the workgroup
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
      if (lane == 0) sh.red2[w * NGW + g] = s_rap;
    }
    __syncthreads();
    double rap = 0.0;
#pragma unroll
    for (int g = 0; g < NGROUP; ++g) rap += (double)sh.red2[g];
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
  sm_flush_x<RR, true>(x, prws, xacc, row0, col0);
}

// v = (v - mask grad p) mask (flow.py:322-327, nd.py:603-614: symmetric padding) on this thread's cells; emit(i, j, c, v) sees every result
template <int RR, class Emit>
__device__ __forceinline__ void sm_project(const SmWorkspace& W, const float2* __restrict__ vmask, int row0, int col0, Emit emit) {
#pragma unroll 1
  for (int k = 0; k < RR; ++k)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = row0 + k, j = col0 + e, c = i * SG + j;
      const int ic = sm_clamp(i), jc = sm_clamp(j);
      const float pc = W.pr[ic * SG + jc], pl = W.pr[ic * SG + sm_clamp(j - 1)], pu = W.pr[sm_clamp(i - 1) * SG + jc];
      const float2 m = vmask[c];
      float2 v = W.vel[c];
      v.x = __fmul_rn(__fadd_rn(v.x, -__fmul_rn(__fadd_rn(pc, -pl), m.x)), m.x);
      v.y = __fmul_rn(__fadd_rn(v.y, -__fmul_rn(__fadd_rn(pc, -pu), m.y)), m.y);
      W.vel[c] = v;
      emit(i, j, c, v);
    }
}

// advection of both densities at cell (i, j) (nd.py:422-427, scipy_backend.py:58-78): src = density plane, then set-zero density plane.
// WIDE = false: the coordinate idx - v is formed in fp32, the velocity's dtype, as the reference forms it (the evaluation solver: its
// bits are the reference's arithmetic). WIDE = true: the same fp32 centred velocity, but the subtraction and the clamp in fp64. Near
// idx = 100 the fp32 difference carries an error of up to 3.8e-6 cells every frame, which is what limits the density (and, at a smoke
// front's leading edge, the bucket sums) once the velocity is accurate; in fp64 that term is gone.
template <bool WIDE>
__device__ __forceinline__ void sm_advect_cell(const float2* __restrict__ velws, const float* __restrict__ src, int i, int j, int c, float& d, float& z) {
  d = 0.f; z = 0.f;
  if (i < SN && j < SN) {
    const float2 v = velws[c];
    const float cy = __fmul_rn(__fadd_rn(velws[c + SG].y, v.y), 0.5f), cx = __fmul_rn(__fadd_rn(velws[c + 1].x, v.x), 0.5f);
    if (WIDE) {
      const double yi = fmax(0.0, fmin((double)SN, (double)i - (double)cy));
      const double xj = fmax(0.0, fmin((double)SN, (double)j - (double)cx));
      d = sm_sample(src, yi, xj);
      z = sm_sample(src + SCELLS, yi, xj);
    } else {
      const float yi = fmaxf(0.f, fminf((float)SN, __fadd_rn((float)i, -cy)));
      const float xj = fmaxf(0.f, fminf((float)SN, __fadd_rn((float)j, -cx)));
      d = sm_sample(src, yi, xj);
      z = sm_sample(src + SCELLS, yi, xj);
    }
  }
}

// the NQ per-frame sums of one 8-row group: fp64 over the wave, lane 0 leaves them in the group's slot
template <int NQ, int NW>
__device__ __forceinline__ void sm_group_sums(SmShared<NW, NQ>& sh, const double (&s)[NQ], int lane, int slot) {
#pragma unroll
  for (int qn = 0; qn < NQ; ++qn) {
    const double t = wave_sum_d(s[qn]);
    if (lane == 0) sh.fred[qn][slot] = t;
  }
}

}  // namespace smoke
