// burgers_step.h -- the explicit-Euler step of the Burgers finite-difference solver, shared by the two kernels that integrate it:
// burgers.hip (control evaluation: a dense forcing, interpolated) and burgers_datagen.hip (data-set generation: the forcing from tables).
// Both say the step once, here: the point update in the reference's operation order, the DPP / LDS halo, the record rule.
//
// Pm is the kernel's parameter struct; the step reads its s, sub_s and the fp32 constants h, d, dm, dt.
#pragma once
#include "common.h"

// one point: a = u[i-1], b = u[i], e = u[i+1], fv = f[f_idx][i]
template <class Pm>
__device__ __forceinline__ float bg_update(float a, float b, float e, float fv, const Pm& p) {
  const float tr = __fadd_rn(__fmul_rn(__fmul_rn(a, a), p.h), __fmul_rn(__fmul_rn(e, e), -p.h));              // -(1/2) transport
  const float df = __fadd_rn(__fadd_rn(__fmul_rn(a, p.d), __fmul_rn(b, p.dm)), __fmul_rn(e, p.d));             // diffusion
  return __fadd_rn(b, __fmul_rn(p.dt, __fadd_rn(__fadd_rn(tr, df), fv)));
}

// DPP wave shifts (wave_shr:1 / wave_shl:1): the value of lane l - 1 / l + 1, 0 where there is none
__device__ __forceinline__ float bg_from_prev_lane(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float bg_from_next_lane(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
}

// g0 as a value the compiler cannot see through: keeps the per-point index arithmetic of the rare paths (records, interval changes) from being
// hoisted out of the step loop into registers (3-4 per point otherwise: 118 VGPRs at P = 8 instead of ~50)
__device__ __forceinline__ int bg_opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// the columns g % sub_s == 0 of a lane's P values into a record row
template <int P, class Pm>
__device__ __forceinline__ void bg_record(const float (&u)[P], int g0, float* __restrict__ row, const Pm& p) {
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const int g = bg_opaque(g0) + k;
    if (g < p.s && g % p.sub_s == 0) row[g / p.sub_s] = u[k];
  }
}

// halo[par][0][w + 1] = last point of wave w, halo[par][1][w] = first point of wave w; halo[.][0][0] and halo[.][1][W] stay 0 (the ghosts)
template <int W>
__device__ __forceinline__ void bg_halo_init(float (&halo)[2][2][W + 1]) {
  if (W > 1) {
    if (threadIdx.x < 4 * (W + 1)) (&halo[0][0][0])[threadIdx.x] = 0.f;
    __syncthreads();
  }
}

// One step of every point of the workgroup: u <- u + dt (-(1/2) transport + diffusion + fc); points past the grid stay 0. Names the kernel's
// W, P, u[P], fc[P], halo, par, lane, w, wave_full, g0 and p. A macro, not a function: as an inlined function the same text moved the register
// allocation of 7 of the solver's 24 instantiations (one of them down an occupancy step); as text in the kernel they compile as before.
#define BG_STEP()                                                                                       \
  do {                                                                                                  \
    float nu[P];                                                                                        \
    if (W > 1) {                                                                                        \
      if (lane == 0) halo[par][1][w] = u[0];                                                            \
      if (lane == 63) halo[par][0][w + 1] = u[P - 1];                                                   \
    }                                                                                                   \
    const float from_prev = bg_from_prev_lane(u[P - 1]), from_next = bg_from_next_lane(u[0]);           \
    _Pragma("unroll") for (int k = 1; k < P - 1; ++k) nu[k] = bg_update(u[k - 1], u[k], u[k + 1], fc[k], p); \
    float left = from_prev, right = from_next;                                                          \
    if (W > 1) {                                                                                        \
      __syncthreads();                                                                                  \
      const float hl = halo[par][0][w], hr = halo[par][1][w + 1];                                       \
      left = lane == 0 ? hl : left;                                                                     \
      right = lane == 63 ? hr : right;                                                                  \
      par ^= 1;                                                                                         \
    }                                                                                                   \
    nu[0] = bg_update(left, u[0], u[1], fc[0], p);                                                      \
    nu[P - 1] = bg_update(u[P - 2], u[P - 1], right, fc[P - 1], p);                                     \
    if (wave_full) {                                                                                    \
      _Pragma("unroll") for (int k = 0; k < P; ++k) u[k] = nu[k];                                       \
    } else {                                                                                            \
      const int gq = bg_opaque(g0);                                                                     \
      _Pragma("unroll") for (int k = 0; k < P; ++k) u[k] = gq + k < p.s ? nu[k] : 0.f;                  \
    }                                                                                                   \
  } while (0)
