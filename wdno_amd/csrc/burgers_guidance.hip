// burgers_guidance.hip -- the gradient of the Burgers control objective (eval_ddpm_burgers.py:108-147, test_util.py:100-126) in closed form,
// as ONE launch that turns the U-Net's noise estimate into the guided one (diffusion_1d.py:205-227): predict x0, rescale, 2-D synthesis
// (H pass then W pass, periodization), residual, adjoint synthesis, rescale, schedule, add. include/wdno_hip.h states the mathematics.
//
// Layout. 1 + ntile workgroups of 1024 threads per sample (blockIdx.y = sample), every intermediate in LDS:
//   block 0      field u. J reads only reconstruction rows 0 and n_t - 1, so only those two rows are synthesised (each from the L/2
//                coefficient rows within the filter's reach, periodic wrap included) and their adjoint reaches the same few rows.
//   block 1 + j  field f, coefficient columns [j tw, (j + 1) tw): the H passes are column-independent and the W passes reach L/2 - 1
//                coefficient columns to each side, so a tile stages tw + L - 2 columns (periodic) and needs nothing from its neighbours.
// Every block also writes the part of `out` where g = 0 (a copy of eps, or zeros in gradient mode): block 0 the rest of channels 0-3,
// tile j the rest of its columns of channels 4-7 (the last tile up to column W), and all blocks share channels 8.. .
//
// Synthesis along one axis (N = 2M outputs from M (lo, hi) pairs, off = L/2 - 1; oracle/dwt_ref.py: synthesis_per):
//   out[i] = sum over m < L with e = i + off - m even of lo[(e / 2) mod M] g_lo[m] + hi[(e / 2) mod M] g_hi[m]
// and its adjoint: dlo[k] = sum_m g_lo[m] r[(2k + m - off) mod N], dhi likewise. Sums run over m ascending, nothing is atomic, and no
// product is contracted into a sum, so a sample's bits do not depend on the batch.
#include "common.h"

namespace {

struct GuidP {
  const float* xt; const float* in; float* out;
  const int64_t* t; const float* c1; const float* c2; const float* s; const float* resc; const float* targ;
  int C, H, W, ss, cs, rs;
  int h, w, n_t, n_x, ntile, tw, T;
  int condition_f, clip;
  float cu, cf;                   // 2 wu / n_x and 2 wu wf
};

constexpr int NT = 1024;      // threads of a workgroup: the phases are short dependent chains of loads, so a block wants all the waves a CU takes

template <int L> struct GTaps { float lo[L], hi[L]; };      // rec_lo, rec_hi

__device__ __forceinline__ int wrap1(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }      // -n <= v < 2n

// per-sample scalars and the two element-wise ends of the chain
struct GuidS {
  bool fused; float c1, c2, s;
  __device__ __forceinline__ float coef(const GuidP& p, size_t idx, int ch) const {      // (x0 RESCALER) at one element
    float v = p.in[idx];
    if (fused) {
      v = __fadd_rn(__fmul_rn(c1, p.xt[idx]), -__fmul_rn(c2, v));
      if (p.clip) v = fminf(fmaxf(v, -1.f), 1.f);
    }
    return __fmul_rn(v, p.resc[ch]);
  }
  __device__ __forceinline__ void guided(const GuidP& p, size_t idx, int ch, float gsum) const {
    const float g = __fmul_rn(p.resc[ch], gsum);
    p.out[idx] = fused ? __fadd_rn(p.in[idx], __fmul_rn(g, s)) : g;
  }
  __device__ __forceinline__ void plain(const GuidP& p, size_t idx) const { p.out[idx] = fused ? p.in[idx] : 0.f; }
};

template <int L>
__global__ __launch_bounds__(NT) void burgers_guidance_kernel(GuidP p, GTaps<L> g) {
  constexpr int OFF = L / 2 - 1;
  extern __shared__ __align__(16) float smem[];
  float* const tap = smem;                      // [2][L]: the taps once more, for the places that index them by a run-time m
  float* const buf = smem + 2 * L;
  const int tid = threadIdx.x, blk = blockIdx.x, nblk = gridDim.x;
  const size_t base = (size_t)blockIdx.y * p.ss;
  GuidS q;
  q.fused = p.xt != nullptr;
  q.c1 = q.c2 = q.s = 0.f;
  if (q.fused) {
    long long tb = p.t[blockIdx.y];
    tb = tb < 0 ? 0 : (tb >= p.T ? p.T - 1 : tb);
    q.c1 = p.c1[tb]; q.c2 = p.c2[tb]; q.s = p.s[tb];
  }
#pragma unroll
  for (int m = 0; m < L; ++m)
    if (tid == m) { tap[m] = g.lo[m]; tap[L + m] = g.hi[m]; }
  const int h = p.h, w = p.w, Nh = 2 * h, Nw = 2 * w;

  if (blk == 0) {
    // ------------------------------------------------------------------------------------------ field u: rows 0 and n_t - 1
    const int nrow = p.condition_f ? 1 : 2;
    float* const A = buf;                       // [nrow][2][w]: (lo_w, hi_w) of the rows; later D, their W-adjoint
    float* const R = buf + 4 * w;               // [nrow][Nw]: the residual rows
    for (int idx = tid; idx < nrow * 2 * w; idx += NT) {
      const int ri = idx / (2 * w), rem = idx - ri * 2 * w, pair = rem / w, kw = rem - pair * w;
      const int i = ri ? p.n_t - 1 : 0;
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < L; ++m) {
        const int e = i + OFF - m;
        if ((e & 1) == 0) {
          const int k = wrap1(e >> 1, h);
          const size_t at = base + (size_t)(2 * pair) * p.cs + (size_t)k * p.rs + kw;
          acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(q.coef(p, at, 2 * pair), g.lo[m]), __fmul_rn(q.coef(p, at + p.cs, 2 * pair + 1), g.hi[m])));
        }
      }
      A[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < nrow * Nw; idx += NT) {
      const int ri = idx / Nw, j = idx - ri * Nw;
      float r = 0.f;
      if (j < p.n_x) {
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < L; ++m) {
          const int e = j + OFF - m;
          if ((e & 1) == 0) {
            const int k = wrap1(e >> 1, w);
            acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(A[(ri * 2) * w + k], g.lo[m]), __fmul_rn(A[(ri * 2 + 1) * w + k], g.hi[m])));
          }
        }
        r = __fmul_rn(p.cu, __fadd_rn(acc, -p.targ[((size_t)blockIdx.y * 2 + ri) * p.n_x + j]));
      }
      R[idx] = r;
    }
    __syncthreads();
    for (int idx = tid; idx < nrow * 2 * w; idx += NT) {      // D over A: A was last read before the barrier above
      const int ri = idx / (2 * w), rem = idx - ri * 2 * w, pair = rem / w, kw = rem - pair * w;
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < L; ++m) acc = __fadd_rn(acc, __fmul_rn(pair ? g.hi[m] : g.lo[m], R[ri * Nw + wrap1(2 * kw + m - OFF, Nw)]));
      A[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < 4 * p.H * p.W; idx += NT) {     // channels 0-3, whole planes
      const int ch = idx / (p.H * p.W), rem = idx - ch * p.H * p.W, k = rem / p.W, col = rem - k * p.W;
      const size_t at = base + (size_t)ch * p.cs + (size_t)k * p.rs + col;
      bool hit = false;
      float acc = 0.f;
      if (k < h && col < w) {
        for (int ri = 0; ri < nrow; ++ri) {
          const int i = ri ? p.n_t - 1 : 0;
          const int m = wrap1(i + OFF - 2 * k, Nh);            // the one tap that links reconstruction row i to coefficient row k
          if (m < L) {
            hit = true;
            acc = __fadd_rn(acc, __fmul_rn(tap[(ch & 1) * L + m], A[(ri * 2 + (ch >> 1)) * w + col]));
          }
        }
      }
      if (hit) q.guided(p, at, ch, acc); else q.plain(p, at);
    }
  } else {
    // ------------------------------------------------------------------------------------------ field f: one column tile
    const int tile = blk - 1, c0 = tile * p.tw, n = min(w, c0 + p.tw) - c0;
    const int tq = p.tw + 2 * OFF, rw = 2 * p.tw + L - 2, NR = p.n_t - 1;
    float* const CO = buf;                      // [4][h][tq]: the coefficient columns c0 - OFF .. of the four bands
    float* const LW = CO + 4 * h * tq;          // [2][NR][tq]: (lo_w, hi_w); later D [2][NR][tw], their W-adjoint on the tile's own columns
    float* const R = LW + 2 * NR * tq;          // [NR][rw]: the residual on columns 2 c0 - OFF ..
    for (int idx = tid; idx < 4 * h * tq; idx += NT) {
      const int band = idx / (h * tq), rem = idx - band * h * tq, k = rem / tq, qq = rem - k * tq;
      const int col = ((c0 - OFF + qq) % w + w) % w;
      CO[idx] = q.coef(p, base + (size_t)(4 + band) * p.cs + (size_t)k * p.rs + col, 4 + band);
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * NR * tq; idx += NT) {
      const int pair = idx / (NR * tq), rem = idx - pair * NR * tq, i = rem / tq, qq = rem - i * tq;
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < L; ++m) {
        const int e = i + OFF - m;
        if ((e & 1) == 0) {
          const int k = wrap1(e >> 1, h);
          acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(CO[((2 * pair) * h + k) * tq + qq], g.lo[m]), __fmul_rn(CO[((2 * pair + 1) * h + k) * tq + qq], g.hi[m])));
        }
      }
      LW[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < NR * rw; idx += NT) {
      const int i = idx / rw, jj = idx - i * rw;
      const int j = wrap1(2 * c0 - OFF + jj, Nw) % Nw;          // (a tile wider than the field wraps more than once on the right)
      float r = 0.f;
      if (j < p.n_x) {
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < L; ++m) {
          const int e = jj - m;                                  // = j + OFF - m up to the even shift 2 (c0 - OFF)
          if ((e & 1) == 0) {
            const int qq = (e >> 1) + OFF;                       // staged column of coefficient column e / 2 + c0 - OFF: 0 .. tq - 1
            acc = __fadd_rn(acc, __fadd_rn(__fmul_rn(LW[i * tq + qq], g.lo[m]), __fmul_rn(LW[(NR + i) * tq + qq], g.hi[m])));
          }
        }
        r = __fmul_rn(p.cf, acc);
      }
      R[idx] = r;
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * NR * n; idx += NT) {          // D over LW: LW was last read before the barrier above
      const int pair = idx / (NR * n), rem = idx - pair * NR * n, i = rem / n, kl = rem - i * n;
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < L; ++m) acc = __fadd_rn(acc, __fmul_rn(pair ? g.hi[m] : g.lo[m], R[i * rw + 2 * kl + m]));
      LW[(pair * NR + i) * p.tw + kl] = acc;
    }
    __syncthreads();
    const int cend = tile == p.ntile - 1 ? p.W : c0 + n, cw = cend - c0;
    for (int idx = tid; idx < 4 * p.H * cw; idx += NT) {        // channels 4-7, this tile's columns
      const int band = idx / (p.H * cw), rem = idx - band * p.H * cw, k = rem / cw, col = c0 + rem - k * cw;
      const size_t at = base + (size_t)(4 + band) * p.cs + (size_t)k * p.rs + col;
      if (k < h && col < w) {
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < L; ++m) {
          const int i = wrap1(2 * k + m - OFF, Nh);
          if (i < NR) acc = __fadd_rn(acc, __fmul_rn((band & 1) ? g.hi[m] : g.lo[m], LW[((band >> 1) * NR + i) * p.tw + col - c0]));
        }
        q.guided(p, at, 4 + band, acc);
      } else {
        q.plain(p, at);
      }
    }
  }
  // channels 8 .. C - 1 carry no gradient: shared by the sample's blocks
  const int rest = (p.C - 8) * p.H * p.W;
  for (int idx = blk * NT + tid; idx < rest; idx += nblk * NT) {
    const int ch = idx / (p.H * p.W), rem = idx - ch * p.H * p.W, k = rem / p.W, col = rem - k * p.W;
    q.plain(p, base + (size_t)(8 + ch) * p.cs + (size_t)k * p.rs + col);
  }
}

}  // namespace

extern "C" int wdno_burgers_guidance(const float* x_t, const float* in, const int64_t* t, const float* c1, const float* c2, const float* s_table,
                                     const float* rescaler, const float* target, float* out, const wdno_burgers_guidance_desc* d,
                                     const float* filt, wdno_stream_t s) {
  WDNO_REQUIRE(in && rescaler && target && out && d && filt && in != out && x_t != out);
  WDNO_REQUIRE(!x_t || (t && c1 && c2 && s_table && d->num_timesteps > 0));
  if (d->mode != 0 || d->L != 10) return WDNO_EUNSUPPORTED;
  constexpr int L = 10;
  WDNO_REQUIRE(d->B > 0 && d->B <= 65535 && d->C >= 8 && d->H > 0 && d->W > 0);
  WDNO_REQUIRE(d->row_stride >= d->W && (int64_t)d->chan_stride >= (int64_t)d->H * d->row_stride && (int64_t)d->sample_stride >= (int64_t)d->C * d->chan_stride);
  WDNO_REQUIRE((int64_t)d->B * d->sample_stride < ((int64_t)1 << 40));
  WDNO_REQUIRE(d->h > 0 && d->h <= d->H && d->w > 0 && d->w <= d->W && 2 * d->h >= L && 2 * d->w >= L);
  WDNO_REQUIRE(d->n_t >= 2 && d->n_t <= 2 * d->h && d->n_x >= 1 && d->n_x <= 2 * d->w);
  WDNO_REQUIRE(d->tw > 0 && d->ntile > 0 && (int64_t)(d->ntile - 1) * d->tw < d->w && (int64_t)d->ntile * d->tw >= d->w);
  const int64_t tq = d->tw + L - 2, rw = 2 * (int64_t)d->tw + L - 2, NR = d->n_t - 1;
  const int64_t need_f = 4 * (int64_t)d->h * tq + 2 * NR * tq + NR * rw, need_u = 8 * (int64_t)d->w;
  const int64_t need = 4 * (2 * L + (need_f > need_u ? need_f : need_u));
  WDNO_REQUIRE(d->lds_bytes >= need && d->lds_bytes <= 65536);
  GuidP p;
  p.xt = x_t; p.in = in; p.out = out; p.t = t; p.c1 = c1; p.c2 = c2; p.s = s_table; p.resc = rescaler; p.targ = target;
  p.C = d->C; p.H = d->H; p.W = d->W; p.ss = d->sample_stride; p.cs = d->chan_stride; p.rs = d->row_stride;
  p.h = d->h; p.w = d->w; p.n_t = d->n_t; p.n_x = d->n_x; p.ntile = d->ntile; p.tw = d->tw; p.T = d->num_timesteps;
  p.condition_f = d->condition_f != 0; p.clip = d->clip_x0 != 0;
  p.cu = (float)(2.0 * (double)d->wu / d->n_x);
  p.cf = (float)(2.0 * (double)d->wu * (double)d->wf);
  GTaps<L> g;
  for (int m = 0; m < L; ++m) { g.lo[m] = filt[2 * L + m]; g.hi[m] = filt[3 * L + m]; }
  burgers_guidance_kernel<L><<<dim3(1 + d->ntile, d->B), NT, (size_t)d->lds_bytes, as_stream(s)>>>(p, g);
  return wdno_check_launch();
}
