// burgers_reconstruct.hip -- the wavelet branch of diffuse_2dconv (eval_ddpm_burgers.py:185-195) as ONE launch for the whole batch: the sampled
// state x [B][C][H][W] in network units becomes u [B][n_t][n_x] and f [B][n_t - 1][n_x],
//   u_f = IDWT2((x RESCALER)[:, 0:8, :h, :w])[:, :, :n_t, :n_x],  u = u_f[:, 0],  f = u_f[:, 1, :n_t - 1]
// (bior2.4, periodization, single level; channels 0-3 = LL, da, ad, dd of u, 4-7 of f: wave_trans.tensor_to_coef). include/wdno_hip.h states
// the contract; wdno_amd/burgers/reconstruct.py: plan() chooses the tile.
//
// Synthesis along one axis as in csrc/burgers_guidance.hip (N = 2M outputs from M (lo, hi) pairs, off = L/2 - 1; oracle/dwt_ref.py:
// synthesis_per):  out[i] = sum over m < L with e = i + off - m even of lo[(e / 2) mod M] g_lo[m] + hi[(e / 2) mod M] g_hi[m],
// summed over m ascending with the two products of a tap added first, no product contracted into a sum: the same order and roundings as the
// guidance kernel's residual, so the fields scored here are the fields the objective was evaluated on.
//
// Layout. One workgroup of 256 threads per (sample, field, tile of tn reconstruction rows, full width), passes in the order H, W:
//   H pass  reads the coefficients in place through x's strides (a row of the tile reads the L/2 coefficient rows within the filter's reach,
//           periodic wrap included; x RESCALER is formed on the fly) and writes (lo_w, hi_w) [2][tn][w] to LDS;
//   W pass  LDS -> registers -> u or f, cropped to n_x columns (and to n_t - 1 rows for f).
// The H pass has no halo in LDS and the only buffer is w (not 2w) wide: 8 tn w bytes, 13 440 B for the evaluation's 41 x 60 block at
// tn = 28. Nothing outside the block is read, nothing is atomic and every sum has a fixed order: a sample's bits do not depend on the batch
// size or on its index.
#include "common.h"

namespace {

constexpr int NT = 256;

template <int L> struct RTaps { float lo[L], hi[L]; };      // rec_lo, rec_hi

struct BRecP {
  const float* x; const float* resc; float* u; float* f;
  int64_t ss; int cs, rs;                    // strides of sample, channel, row (elements)
  int h, w, n_t, n_x, tn, ntile;
};

__device__ __forceinline__ int wrap1(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }      // -n <= v < 2n

template <int L>
__global__ __launch_bounds__(NT) void burgers_reconstruct_kernel(BRecP p, RTaps<L> g) {
  constexpr int OFF = L / 2 - 1;
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int field = blockIdx.x / p.ntile, tile = blockIdx.x - field * p.ntile;
  const int nout = field ? p.n_t - 1 : p.n_t;             // rows of this field's output
  const int r0 = tile * p.tn, rows = min(p.tn, nout - r0);
  if (rows <= 0) return;                                   // (the last tile of f when n_t - 1 is a multiple of tn: the whole workgroup leaves)
  const int h = p.h, w = p.w, tn = p.tn;
  float* const LW = smem;                                  // [2][tn][w]: (lo_w, hi_w) of the tile's rows
  const float* const xb = p.x + (size_t)b * p.ss + (size_t)(4 * field) * p.cs;
  // H pass
  for (int idx = tid; idx < 2 * rows * w; idx += NT) {
    const int pair = idx / (rows * w), rem = idx - pair * rows * w, ii = rem / w, kw = rem - ii * w;
    const int i = r0 + ii, ch = 4 * field + 2 * pair;
    const float rl = p.resc[ch], rh = p.resc[ch + 1];
    const float* const xl = xb + (size_t)(2 * pair) * p.cs + kw;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < L; ++m) {
      const int e = i + OFF - m;
      if ((e & 1) == 0) {
        const size_t at = (size_t)wrap1(e >> 1, h) * p.rs;
        acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(__fmul_rn(xl[at], rl), g.lo[m]), __fmul_rn(__fmul_rn(xl[at + p.cs], rh), g.hi[m])));
      }
    }
    LW[(pair * tn + ii) * w + kw] = acc;
  }
  __syncthreads();
  // W pass
  float* const ob = (field ? p.f : p.u) + ((size_t)b * nout + r0) * p.n_x;
  const float* const HI = LW + tn * w;
  for (int idx = tid; idx < rows * p.n_x; idx += NT) {
    const int ii = idx / p.n_x, j = idx - ii * p.n_x;
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < L; ++m) {
      const int e = j + OFF - m;
      if ((e & 1) == 0) {
        const int k = ii * w + wrap1(e >> 1, w);
        acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(LW[k], g.lo[m]), __fmul_rn(HI[k], g.hi[m])));
      }
    }
    ob[idx] = acc;
  }
}

}  // namespace

extern "C" int wdno_burgers_reconstruct(const float* x, const float* rescaler, float* u, float* f, const wdno_burgers_reconstruct_desc* d,
                                        const float* filt, wdno_stream_t s) {
  WDNO_REQUIRE(x && rescaler && u && f && d && filt && x != u && x != f && u != f);
  WDNO_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(rescaler) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(f)) & 3) == 0);
  if (d->mode != 0 || d->L != 10) return WDNO_EUNSUPPORTED;
  constexpr int L = 10;
  WDNO_REQUIRE(d->B > 0 && d->B <= 65535 && d->C >= 8 && d->H > 0 && d->W > 0);
  WDNO_REQUIRE(d->row_stride >= d->W && (int64_t)d->chan_stride >= (int64_t)d->H * d->row_stride &&
               d->sample_stride >= (int64_t)d->C * d->chan_stride);      // strides that do not fit
  WDNO_REQUIRE((int64_t)d->C * d->chan_stride < ((int64_t)1 << 31) && (int64_t)d->B * d->sample_stride < ((int64_t)1 << 40));
  WDNO_REQUIRE(d->h > 0 && d->h <= d->H && d->w > 0 && d->w <= d->W && 2 * d->h >= L && 2 * d->w >= L);      // a block larger than the tensor
  WDNO_REQUIRE(d->n_t >= 2 && d->n_t <= 2 * d->h && d->n_x >= 1 && d->n_x <= 2 * d->w);                       // a crop larger than the reconstruction
  WDNO_REQUIRE((int64_t)d->B * d->n_t * d->n_x < ((int64_t)1 << 40));
  WDNO_REQUIRE(d->tn >= 2 && !(d->tn & 1) && d->ntile > 0 && (int64_t)(d->ntile - 1) * d->tn < d->n_t && (int64_t)d->ntile * d->tn >= d->n_t);
  WDNO_REQUIRE(2 * (int64_t)d->ntile <= 65535);
  const int64_t need = 4 * 2 * (int64_t)d->tn * d->w;
  WDNO_REQUIRE(d->lds_bytes >= need && d->lds_bytes <= 65536);
  BRecP p;
  p.x = x; p.resc = rescaler; p.u = u; p.f = f;
  p.ss = d->sample_stride; p.cs = d->chan_stride; p.rs = d->row_stride;
  p.h = d->h; p.w = d->w; p.n_t = d->n_t; p.n_x = d->n_x; p.tn = d->tn; p.ntile = d->ntile;
  RTaps<L> g;
  for (int m = 0; m < L; ++m) { g.lo[m] = filt[2 * L + m]; g.hi[m] = filt[3 * L + m]; }
  burgers_reconstruct_kernel<L><<<dim3(2 * d->ntile, d->B), NT, (size_t)d->lds_bytes, as_stream(s)>>>(p, g);
  return wdno_check_launch();
}
