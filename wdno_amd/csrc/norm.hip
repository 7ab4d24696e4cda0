// norm.hip -- GroupNorm(+scale/shift)+SiLU on channels-last tensors (HBM-bound). The steps its kernels share are stated once in norm_tiles.h;
// the channel LayerNorm is layernorm.hip.
//
// GroupNorm [N, S, C] with G groups (G = 1 is a whole-sample reduction of up to 1024*64*64 elements for Burgers):
//   pass 1  gn_partial  : per (sample, row-chunk) per-channel sum / sum-of-squares, accumulated in fp64
//   pass 2  gn_finalize : per sample: group mean / rstd (fp64), folded per-channel affine  y = act(a[c]*x + b[c])
//   pass 3  gn_apply    : one read of x, one write of y
// Backward mirrors it: per-channel sums of dz and dz*xhat, a per-sample finalize producing the parameter
// gradients and the two group means, then one elementwise pass for dx.
#include "norm_tiles.h"

static inline int gn_chunks(int64_t S, int64_t N, int C) {
  int64_t c = cdiv64(S, 64);
  if (c > 64) c = 64;
  if (c < 1) c = 1;
  // few samples x few rows of many channels (the deep levels of the Burgers U-Net: 16 samples x 64 pixels x 1024 channels was 16 blocks,
  // 34 us per backward reduction): finer chunks, down to one round of loads (4 rows per row group) each, until ~256 blocks exist
  int txp = pow2ceil(C >> 2);
  if (txp > 256) txp = 256;
  const int nty = 256 / (txp < 1 ? 1 : txp);
  // (and with one or two LARGE samples -- super-resolution sampling at batch 2: 307 200 pixels each -- more than 64 chunks: 128 blocks were 38.6 us per
  // statistics pass over 157 MB)
  const int64_t cap = N > 0 && 512 / N > 64 ? 512 / N : 64;
  while (c < cap && N * c < 256 && S / (2 * c) >= 4 * nty) c *= 2;
  return (int)c;
}

// ---------------------------------------------------------------------------------------------- per-channel partial sums
// MODE 0: (sum x, sum x^2)         MODE 1: (sum dz, sum dz*xhat) with dz = dy * act'(a x + b)
template <int MODE, typename XT = float, typename DT = float>
__global__ __launch_bounds__(256) void gn_partial_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                          const float* __restrict__ cb /*[N][C][4]*/, const float* __restrict__ gb /*[N][G][4]*/,
                                                          double* __restrict__ part, int64_t S, int C, int cg, int G, int txp,
                                                          int64_t rows_per_chunk, int silu, float* __restrict__ mx = nullptr) {
  // mx (optional): per (sample, chunk) max|dz| and max|xhat| (MODE 1) or max|x| (MODE 0) -- what the finalize kernels need to
  // bound |dx| / |y| before the apply pass runs
  __shared__ double red[256 * 8];
  __shared__ float redm[8];
  float m0[4] = {0.f, 0.f, 0.f, 0.f}, m1[4] = {0.f, 0.f, 0.f, 0.f};
  const int n = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int C4 = C >> 2;
  const int tx = threadIdx.x & (txp - 1), ty = threadIdx.x / txp, nty = 256 / txp;
  const int64_t r0 = (int64_t)chunk * rows_per_chunk;
  int64_t r1 = r0 + rows_per_chunk;
  if (r1 > S) r1 = S;
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (tx < C4) {
    float ca[4], cbb[4], mean[4], rstd[4];
    if (MODE == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int c = tx * 4 + j;
        ca[j] = cb[((int64_t)n * C + c) * 4 + 0];
        cbb[j] = cb[((int64_t)n * C + c) * 4 + 1];
        int g = c / cg;
        mean[j] = gb[((int64_t)n * G + g) * 4 + 0];
        rstd[j] = gb[((int64_t)n * G + g) * 4 + 1];
      }
    }
    const int64_t e0 = ((int64_t)n * S) * C + tx * 4;             // element offset of this thread's four channels in row 0 of the sample
    // four rows per round (eight of bf16 storage: the same bytes in flight -- with four, the bf16 form of the backward reduction was SLOWER than
    // the fp32 one, 105 vs 93 us per launch at Burgers batch 256), all loads requested before the first is used (one row at a time leaves
    // ~4 MB in flight chip-wide)
    constexpr int RIF = std::is_same<XT, gn_bf16>::value ? 8 : 4;
    for (int64_t rb = r0 + ty; rb < r1; rb += RIF * nty) {
      float4 vv[RIF], dd[RIF];
#pragma unroll
      for (int u = 0; u < RIF; ++u) {
        const int64_t r = rb + u * nty;
        const bool ok = r < r1;
        vv[u] = ok ? gn_ld<XT>::ld4(x, e0 + r * C) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == 1) dd[u] = ok ? gn_ld<DT>::ld4(dy, e0 + r * C) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < RIF; ++u) {
        if (rb + u * nty >= r1) break;
        const float4 v = vv[u];
        float xv[4] = {v.x, v.y, v.z, v.w};
        if (MODE == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { s0[j] += (double)xv[j]; s1[j] += (double)xv[j] * (double)xv[j]; m0[j] = fmaxf(m0[j], fabsf(xv[j])); }
        } else {
          const float4 d = dd[u];
          float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float dz = gn_bwd_dz(dv[j], ca[j], cbb[j], xv[j], silu);
            const float xh = gn_xhat(xv[j], mean[j], rstd[j]);
            s0[j] += (double)dz;
            s1[j] += (double)dz * (double)xh;
            m0[j] = fmaxf(m0[j], fabsf(dz)); m1[j] = fmaxf(m1[j], fabsf(xh));
          }
        }
      }
    }
  }
  // reduce over the row groups: red[ty][tx][8]
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[(ty * txp + tx) * 8 + j] = s0[j]; red[(ty * txp + tx) * 8 + 4 + j] = s1[j]; }
  __syncthreads();
  if (ty == 0 && tx < C4) {
    for (int t = 1; t < nty; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) { s0[j] += red[(t * txp + tx) * 8 + j]; s1[j] += red[(t * txp + tx) * 8 + 4 + j]; }
    double* o = part + (((int64_t)n * nchunk + chunk) * C + tx * 4) * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) { o[j * 2] = s0[j]; o[j * 2 + 1] = s1[j]; }
  }
  if (mx) {                       // block maxima of |dz| and |xhat| (MODE 1) / of |x| (MODE 0)
    // inline, not gn_block_max<2>: that one lays LDS out as [value][wave], this as [wave][value], and all six instantiations changed
    float a = fmaxf(fmaxf(m0[0], m0[1]), fmaxf(m0[2], m0[3])), b = fmaxf(fmaxf(m1[0], m1[1]), fmaxf(m1[2], m1[3]));
    a = wave_max(a); b = wave_max(b);
    if ((threadIdx.x & 63) == 0) { redm[(threadIdx.x >> 6) * 2] = a; redm[(threadIdx.x >> 6) * 2 + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float* o = mx + ((int64_t)n * nchunk + chunk) * 2;
      o[0] = fmaxf(fmaxf(redm[0], redm[2]), fmaxf(redm[4], redm[6]));
      o[1] = fmaxf(fmaxf(redm[1], redm[3]), fmaxf(redm[5], redm[7]));
    }
  }
}

// ---------------------------------------------------------------------------------------------- forward finalize
// one block per (sample, slice of groups). writes stats[n][g] = (mean, rstd), cb[n][c] = (a, b, k1, 0), gb[n][g] = (mean, rstd, 0, 0)
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ part, const float* __restrict__ stats_in,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ ss, float* __restrict__ stats_out,
                                                           float* __restrict__ cb, float* __restrict__ gb, int64_t S, int C, int G,
                                                           int nchunk, float eps, const float* __restrict__ mx = nullptr,
                                                           float* __restrict__ bound_rec = nullptr) {
  __shared__ double chs[GN_MAXC], chq[GN_MAXC];
  __shared__ float gmean[GN_MAXC], grstd[GN_MAXC];
  const int n = blockIdx.x, cg = C / G;
  const gn_slice sl = gn_block_slice(cg, G);
  if (sl.gs0 >= sl.gs1) return;
  gamma += sl.cs0; beta += sl.cs0;
  if (ss) ss += sl.cs0;
  cb += (int64_t)sl.cs0 * 4; gb += (int64_t)sl.gs0 * 4;
  if (stats_out) stats_out += (int64_t)sl.gs0 * 2;
  if (stats_in) stats_in += (int64_t)sl.gs0 * 2;
  const int Call = C, Gall = G;
  C = sl.csn; G = sl.gs1 - sl.gs0;
  if (part) {
    gn_chunk_totals(part, n, nchunk, Call, chs, chq, sl.cs0, sl.csn);
    if (cg > 64) {
      // few, wide groups (GroupNorm(1, C) of the Burgers U-Net): the whole block reduces each group. These lines and the loop head below stand in
      // gn_bwd_finalize_kernel too: as functions they changed both kernels (profiles/norm_tiles_header.md)
      __shared__ double ra[256], rb[256];
      for (int g = 0; g < G; ++g) {
        double a = 0, b = 0;
        for (int c = g * cg + threadIdx.x; c < (g + 1) * cg; c += 256) { a += chs[c]; b += chq[c]; }
        ra[threadIdx.x] = a; rb[threadIdx.x] = b;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
          if (threadIdx.x < o) { ra[threadIdx.x] += ra[threadIdx.x + o]; rb[threadIdx.x] += rb[threadIdx.x + o]; }
          __syncthreads();
        }
        if (threadIdx.x == 0) { chs[g * cg] = ra[0]; chq[g * cg] = rb[0]; }      // group totals parked in the first channel slot
        __syncthreads();
      }
    }
    for (int g = threadIdx.x; g < G; g += 256) {
      double a = 0, b = 0;
      if (cg > 64) { a = chs[g * cg]; b = chq[g * cg]; }
      else for (int c = g * cg; c < (g + 1) * cg; ++c) { a += chs[c]; b += chq[c]; }
      double m = (double)cg * (double)S;
      double mean = a / m;
      double var = b / m - mean * mean;
      if (var < 0) var = 0;
      float rstd = (float)(1.0 / sqrt(var + (double)eps));
      gmean[g] = (float)mean; grstd[g] = rstd;
      stats_out[((int64_t)n * Gall + g) * 2 + 0] = (float)mean;
      stats_out[((int64_t)n * Gall + g) * 2 + 1] = rstd;
    }
  } else {
    for (int g = threadIdx.x; g < G; g += 256) {
      gmean[g] = stats_in[((int64_t)n * Gall + g) * 2 + 0];
      grstd[g] = stats_in[((int64_t)n * Gall + g) * 2 + 1];
    }
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    float* o = gb + ((int64_t)n * Gall + g) * 4;
    o[0] = gmean[g]; o[1] = grstd[g]; o[2] = 0.f; o[3] = 0.f;
  }
  float ma = 0.f, mb = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    int g = c / cg;
    float sc1 = ss ? ss[(int64_t)n * 2 * Call + c] + 1.0f : 1.0f;
    float sh = ss ? ss[(int64_t)n * 2 * Call + Call + c] : 0.0f;
    float k1 = grstd[g] * gamma[c];
    float a = k1 * sc1;
    float b = (beta[c] - gmean[g] * k1) * sc1 + sh;
    float* o = cb + ((int64_t)n * Call + c) * 4;
    o[0] = a; o[1] = b; o[2] = a; o[3] = 0.f;   // k1*(s+1) == a
    ma = fmaxf(ma, fabsf(a)); mb = fmaxf(mb, fabsf(b));
  }
  if (bound_rec) {          // |act(a x + b)| <= max|a| max|x| + max|b|: known before the apply pass (gn_apply_planes_kernel)
    float mxx = 0.f;
    for (int k = threadIdx.x; k < nchunk; k += 256) mxx = fmaxf(mxx, mx[((int64_t)n * nchunk + k) * 2]);
    const float v[3] = {wave_max(ma), wave_max(mb), wave_max(mxx)};
    float t[3];
    if (gn_block_max(v, t))
      atomicMax(reinterpret_cast<unsigned*>(bound_rec) + (n & (WDNO_AMAX_SLOTS - 1)) * WDNO_AMAX_STRIDE, __float_as_uint(t[0] * t[2] + t[1]));
  }
}

template <typename XT = float>
__global__ __launch_bounds__(256) void gn_apply_kernel(const void* __restrict__ x, const float* __restrict__ cb, float* __restrict__ y,
                                                        int64_t S, int C, int silu, float* __restrict__ amax_rec) {
  const int n = blockIdx.y;
  const int C4 = C >> 2;
  const int64_t total4 = S * C4;
  const int64_t xe = (int64_t)n * S * C;
  float4* yp = reinterpret_cast<float4*>(y + (int64_t)n * S * C);
  const float4* cbp = reinterpret_cast<const float4*>(cb + (int64_t)n * C * 4);
  const int64_t stride = (int64_t)gridDim.x * 256;
  float am = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
    int c4 = (int)(i % C4);
    float4 v = gn_ld<XT>::ld4(x, xe + i * 4);
    float4 k0 = cbp[c4 * 4 + 0], k1 = cbp[c4 * 4 + 1], k2 = cbp[c4 * 4 + 2], k3 = cbp[c4 * 4 + 3];
    float4 o;
    // gn_fwd_elem four times, written out: ONE branch on silu for the four, and the four affine steps pair up into packed instructions
    o.x = k0.x * v.x + k0.y; o.y = k1.x * v.y + k1.y; o.z = k2.x * v.z + k2.y; o.w = k3.x * v.w + k3.y;
    if (silu) { o.x = silu_f(o.x); o.y = silu_f(o.y); o.z = silu_f(o.z); o.w = silu_f(o.w); }
    yp[i] = o;
    am = amax4(am, o);
  }
  if (amax_rec) amax_record_emit(am, amax_rec, blockIdx.y * gridDim.x + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------- backward finalize / apply
// one block per (sample, slice of groups): parameter-gradient pieces and the two group means
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const double* __restrict__ part, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ ss,
                                                               float* __restrict__ gb, float* __restrict__ dgb, float* __restrict__ dss,
                                                               int64_t S, int C, int G, int nchunk, const float* __restrict__ cb = nullptr,
                                                               const float* __restrict__ mx = nullptr, float* __restrict__ bound_rec = nullptr) {
  __shared__ double chA[GN_MAXC], chB[GN_MAXC];
  const int n = blockIdx.x, cg = C / G;
  const gn_slice sl = gn_block_slice(cg, G);
  if (sl.gs0 >= sl.gs1) return;
  gamma += sl.cs0; beta += sl.cs0;
  if (ss) ss += sl.cs0;
  if (dss) dss += sl.cs0;
  dgb += sl.cs0; gb += (int64_t)sl.gs0 * 4;
  if (cb) cb += (int64_t)sl.cs0 * 4;
  const int Call = C, Gall = G;
  C = sl.csn; G = sl.gs1 - sl.gs0;
  gn_chunk_totals(part, n, nchunk, Call, chA, chB, sl.cs0, sl.csn);
  for (int c = threadIdx.x; c < C; c += 256) {
    const double a = chA[c], b = chB[c];
    float sc1 = ss ? ss[(int64_t)n * 2 * Call + c] + 1.0f : 1.0f;
    if (dss) {
      dss[(int64_t)n * 2 * Call + c] = (float)((double)gamma[c] * b + (double)beta[c] * a);   // d scale
      dss[(int64_t)n * 2 * Call + Call + c] = (float)a;                                          // d shift
    }
    dgb[((int64_t)n * 2 + 0) * Call + c] = (float)((double)sc1 * b);   // d gamma (this sample)
    dgb[((int64_t)n * 2 + 1) * Call + c] = (float)((double)sc1 * a);   // d beta
    double w = (double)gamma[c] * (double)sc1;
    chA[c] = w * a; chB[c] = w * b;
  }
  __syncthreads();
  if (cg > 64) {                       // few, wide groups: block-wide reduction per group (inline: see gn_finalize_kernel)
    __shared__ double ra[256], rb[256];
    for (int g = 0; g < G; ++g) {
      double a = 0, b = 0;
      for (int c = g * cg + threadIdx.x; c < (g + 1) * cg; c += 256) { a += chA[c]; b += chB[c]; }
      ra[threadIdx.x] = a; rb[threadIdx.x] = b;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { ra[threadIdx.x] += ra[threadIdx.x + o]; rb[threadIdx.x] += rb[threadIdx.x + o]; }
        __syncthreads();
      }
      if (threadIdx.x == 0) { chA[g * cg] = ra[0]; chB[g * cg] = rb[0]; }
      __syncthreads();
    }
  }
  for (int g = threadIdx.x; g < G; g += 256) {
    double a = 0, b = 0;
    if (cg > 64) { a = chA[g * cg]; b = chB[g * cg]; }
    else for (int c = g * cg; c < (g + 1) * cg; ++c) { a += chA[c]; b += chB[c]; }
    double m = (double)cg * (double)S;
    float* o = gb + ((int64_t)n * Gall + g) * 4;
    float rstd = o[1];
    o[2] = (float)(a / m) * rstd;
    o[3] = (float)(b / m) * rstd;
  }
  if (bound_rec) {
    // |dx| = |k.z dz - g.z - xhat g.w| <= max|k.z| max|dz| + max|g.z| + max|xhat| max|g.w|: an upper bound of max|dx| that is known
    // BEFORE the apply pass, so that pass can write the (hi, lo) fp16 planes of dx directly (gn_bwd_apply_planes_kernel)
    __syncthreads();
    float mdz = 0.f, mxh = 0.f, mk = 0.f, mz = 0.f, mw = 0.f;
    for (int k = threadIdx.x; k < nchunk; k += 256) {
      mdz = fmaxf(mdz, mx[((int64_t)n * nchunk + k) * 2]); mxh = fmaxf(mxh, mx[((int64_t)n * nchunk + k) * 2 + 1]);
    }
    for (int c = threadIdx.x; c < C; c += 256) mk = fmaxf(mk, fabsf(cb[((int64_t)n * Call + c) * 4 + 2]));
    for (int g = threadIdx.x; g < G; g += 256) {
      mz = fmaxf(mz, fabsf(gb[((int64_t)n * Gall + g) * 4 + 2])); mw = fmaxf(mw, fabsf(gb[((int64_t)n * Gall + g) * 4 + 3]));
    }
    const float v[5] = {wave_max(mdz), wave_max(mxh), wave_max(mk), wave_max(mz), wave_max(mw)};
    float t[5];
    if (gn_block_max(v, t)) {
      const float bound = t[2] * t[0] + t[3] + t[1] * t[4];
      atomicMax(reinterpret_cast<unsigned*>(bound_rec) + (n & (WDNO_AMAX_SLOTS - 1)) * WDNO_AMAX_STRIDE, __float_as_uint(bound));
    }
  }
}

__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const float* __restrict__ cb, const float* __restrict__ gb,
                                                            float* __restrict__ dx, int64_t S, int C, int cg, int G, int silu,
                                                            float* __restrict__ amax_rec) {
  const int n = blockIdx.y;
  const int C4 = C >> 2;
  const int64_t total4 = S * C4;
  const float4* xp = reinterpret_cast<const float4*>(x + (int64_t)n * S * C);
  const float4* dp = reinterpret_cast<const float4*>(dy + (int64_t)n * S * C);
  float4* op = reinterpret_cast<float4*>(dx + (int64_t)n * S * C);
  const float4* cbp = reinterpret_cast<const float4*>(cb + (int64_t)n * C * 4);
  const float4* gbp = reinterpret_cast<const float4*>(gb + (int64_t)n * G * 4);
  const int64_t stride = (int64_t)gridDim.x * 256;
  float am = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
    int c4 = (int)(i % C4);
    float4 v = xp[i], d = dp[i];
    float xv[4] = {v.x, v.y, v.z, v.w}, dv[4] = {d.x, d.y, d.z, d.w}, o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int c = c4 * 4 + j;
      const float4 k = cbp[c], gq = gbp[c / cg];
      o[j] = gn_bwd_elem(k, gq, xv[j], dv[j], silu);
    }
    const float4 ov = make_float4(o[0], o[1], o[2], o[3]);
    op[i] = ov;
    am = amax4(am, ov);
  }
  if (amax_rec) amax_record_emit(am, amax_rec, blockIdx.y * gridDim.x + blockIdx.x);
}

// y as (hi, lo) fp16 planes (scale from the bound gn_finalize_kernel left in `rec`): the output of a Block whose only reader is the
// next convolution. A thread owns 8 channels.
template <typename XT = float>
__global__ __launch_bounds__(256) void gn_apply_planes_kernel(const void* __restrict__ x, const float* __restrict__ cb,
                                                               _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                               float* __restrict__ scale_out, const float* __restrict__ rec,
                                                               int64_t S, int C, int silu) {
  const int n = blockIdx.y;
  const int C8 = C >> 3;
  const int64_t total8 = S * C8;
  const bool single = lo == nullptr;                 // one bf16 plane, no scale (WDNO_CONV_MATH=bf16)
  const float s = gn_planes_scale(single, rec);
  if (!single && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) scale_out[0] = s;
  const int64_t xe = (int64_t)n * S * C;
  _Float16* hp = hi + (int64_t)n * S * C;
  _Float16* lp = single ? nullptr : lo + (int64_t)n * S * C;
  const float4* cbp = reinterpret_cast<const float4*>(cb + (int64_t)n * C * 4);
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int c0 = gn_planes_c0(C8);
  float ka[8], kb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { const float4 k = cbp[c0 + j]; ka[j] = k.x; kb[j] = k.y; }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += stride) {
    float xv[8];
    gn_ld8<XT>(x, xe + i * 8, xv);
    gn_half8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float o = gn_fwd_elem(ka[j], kb[j], xv[j], silu);
      gn_pack_at(h, l, j, o, s, single);
    }
    *reinterpret_cast<gn_half8*>(hp + i * 8) = h;
    if (!single) *reinterpret_cast<gn_half8*>(lp + i * 8) = l;
  }
}

// y = act(a x + b) + res as BOTH the fp32 tensor and its (hi, lo) fp16 planes: the tail of a ResnetBlock with an identity skip
// (unet.py:167-176, conv3d.py:286-300). The sum is the next block's skip (fp32) and the operand of its first convolution (planes): this
// replaces the apply pass, the add and the split (28 bytes per element over three launches) by one pass of 16. Scale from
// max|a| max|x| + max|b| (gn_finalize_kernel, in `rec`) + max|res| (the amax record of res).
template <typename XT = float>
__global__ __launch_bounds__(256) void gn_apply_add_planes_kernel(const void* __restrict__ x, const float* __restrict__ cb,
                                                                   const float* __restrict__ res, float* __restrict__ y,
                                                                   _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                                   float* __restrict__ scale_out, const float* __restrict__ rec,
                                                                   const float* __restrict__ rec_res, float* __restrict__ amax_out,
                                                                   int64_t S, int C, int silu) {
  const int n = blockIdx.y;
  const int C8 = C >> 3;
  const int64_t total8 = S * C8;
  const bool planes = hi != nullptr;                 // hi == nullptr: the fp32 sum only (its reader is a LayerNorm, not a convolution)
  const bool single = lo == nullptr;                 // one bf16 plane, no scale (WDNO_CONV_MATH=bf16)
  const float s = gn_planes_scale<true>(single, rec, rec_res);
  if (!single && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) scale_out[0] = s;
  const int64_t xe = (int64_t)n * S * C;
  const float* rp = res + (int64_t)n * S * C;
  float* yp = y + (int64_t)n * S * C;
  _Float16* hp = planes ? hi + (int64_t)n * S * C : nullptr;
  _Float16* lp = single ? nullptr : lo + (int64_t)n * S * C;
  const float4* cbp = reinterpret_cast<const float4*>(cb + (int64_t)n * C * 4);
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int c0 = gn_planes_c0(C8);
  float ka[8], kb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { const float4 k = cbp[c0 + j]; ka[j] = k.x; kb[j] = k.y; }
  float am = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += stride) {
    float xv[8];
    gn_ld8<XT>(x, xe + i * 8, xv);
    float rv[8], ov[8];
    gn_ld8<float>(rp, i * 8, rv);
    gn_half8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float o = gn_fwd_elem(ka[j], kb[j], xv[j], silu);
      o += rv[j];
      ov[j] = o;
      am = fmaxf(am, fabsf(o));
      gn_pack_at(h, l, j, o, s, single);
    }
    *reinterpret_cast<float4*>(yp + i * 8) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    *reinterpret_cast<float4*>(yp + i * 8 + 4) = make_float4(ov[4], ov[5], ov[6], ov[7]);
    if (planes) *reinterpret_cast<gn_half8*>(hp + i * 8) = h;
    if (planes && !single) *reinterpret_cast<gn_half8*>(lp + i * 8) = l;
  }
  if (amax_out) amax_record_emit(am, amax_out, blockIdx.y * gridDim.x + blockIdx.x);
}

// dx as (hi, lo) fp16 planes (scale from the bound gn_bwd_finalize_kernel left in `rec`) + per-block column sums of dx (the bias
// gradient of the convolution in front of the norm). A thread owns 8 channels: 16-byte plane stores; its channel group is fixed
// (gn_planes_c0), so the column sums stay in registers until the block reduces them.
template <typename XT = float, typename DT = float>
__global__ __launch_bounds__(256) void gn_bwd_apply_planes_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                                   const float* __restrict__ cb, const float* __restrict__ gb,
                                                                   _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                                   float* __restrict__ scale_out, const float* __restrict__ rec,
                                                                   double* __restrict__ csp, int64_t S, int C, int cg, int G, int silu) {
  __shared__ double red[256][9];
  const int n = blockIdx.y;
  const int C8 = C >> 3;
  const int64_t total8 = S * C8;
  const bool single = lo == nullptr;                 // one bf16 plane, no scale (WDNO_CONV_MATH=bf16)
  const float s = gn_planes_scale(single, rec);
  if (!single && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) scale_out[0] = s;
  const int64_t xe = (int64_t)n * S * C;
  _Float16* hp = hi + (int64_t)n * S * C;
  _Float16* lp = single ? nullptr : lo + (int64_t)n * S * C;
  const float4* cbp = reinterpret_cast<const float4*>(cb + (int64_t)n * C * 4);
  const float4* gbp = reinterpret_cast<const float4*>(gb + (int64_t)n * G * 4);
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int c0 = gn_planes_c0(C8);
  float4 kk[8], gq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { kk[j] = cbp[c0 + j]; gq[j] = gbp[(c0 + j) / cg]; }
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total8; i += stride) {
    float xv[8], dv[8];
    gn_ld8<XT>(x, xe + i * 8, xv);
    gn_ld8<DT>(dy, xe + i * 8, dv);
    gn_half8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float o = gn_bwd_elem(kk[j], gq[j], xv[j], dv[j], silu);
      acc[j] += (double)o;
      gn_pack_at(h, l, j, o, s, single);
    }
    *reinterpret_cast<gn_half8*>(hp + i * 8) = h;
    if (!single) *reinterpret_cast<gn_half8*>(lp + i * 8) = l;
  }
  // block reduction of the column sums: threads with the same channel group are C8 apart
#pragma unroll
  for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = acc[j];
  __syncthreads();
  if (threadIdx.x < C8) {
    for (int t = threadIdx.x + C8; t < 256; t += C8)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += red[t][j];
    double* o = csp + ((int64_t)n * gridDim.x + blockIdx.x) * C + c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = acc[j];
  }
}

__global__ __launch_bounds__(PRS_THREADS) void gn_bwd_tail_kernel(const double* __restrict__ csp, float* __restrict__ dx_colsum, int nb, int C, int nbx,
                                                                     const float* __restrict__ dgb, float* __restrict__ dgb_sum, int N) {
  if ((int)blockIdx.x < nbx) {
    partial_rows_sum_body<double>(csp, dx_colsum, nb, C, (int)blockIdx.x);
    return;
  }
  // sum over the samples of the per-sample (d gamma, d beta) pieces: 32 columns x 32 row groups per block, four sums per thread (one thread
  // per column walking all N rows was 256 dependent loads at batch 256: most of this kernel's 88 us there)
  partial_rows_sum_body<float>(dgb, dgb_sum, N, 2 * C, (int)blockIdx.x - nbx);
}

// ---------------------------------------------------------------------------------------------- host
static int gn_check(int64_t N, int64_t S, int C, int G) {
  if (N <= 0 || S <= 0 || C <= 0 || G <= 0 || N > 65535) return WDNO_EINVAL;
  if ((C & 3) || C > GN_MAXC || (C % G) != 0) return WDNO_EUNSUPPORTED;
  return WDNO_OK;
}
// the shapes the planes kernels take: a thread keeps one group of 8 channels (gn_planes_c0)
static bool gn_planes_ok(int C) {
  const int C8 = C / 8;
  return !((C & 7) || C8 > 256 || (C8 & (C8 - 1)));
}
// slices of groups per sample for the finalize kernels: every group its own block while the groups are narrow (the statistics of wide groups --
// GroupNorm(1, C) of the Burgers U-Net -- are reduced by a whole block)
static inline unsigned gn_slices(int C, int G) { return C / G > 64 ? 1u : (unsigned)(G < 32 ? G : 32); }
// blocks per sample of an apply pass whose threads take `per` channels each
static inline int gn_apply_grid(int64_t S, int C, int per) {
  int gx = stream_grid(S * (C / per), 256);
  return gx > 512 ? 512 : gx;
}
// blocks per sample of the planes backward (dx delivered as fp16 (hi, lo) planes: see include/wdno_hip.h)
static inline int gn_planes_grid(int64_t N, int64_t S, int C) {
  int gx = stream_grid(S * (C / 8), 256);
  int cap = (int)(2048 / N);         // blocks per sample: every block leaves one row of column-sum partials, ~2048 rows in total
  if (cap < 2) cap = 2;              // (at batch 256 the final reduction over 32768 rows cost 36 us per GroupNorm)
  if (cap > GN_PLANES_CAP) cap = GN_PLANES_CAP;
  if (gx > cap) gx = cap;
  return gx;
}

// Everything the host derives from a shape, in one place: the launch shapes, the three workspace sizes and where each region lives.
//   ws    : [ double part[N][nchunk][C][2] | room for cb and gb (unused: they live in `stats`) | 64 ] and, from the next 64-byte boundary
//           (`tail`), what the planes forms add:
//             forward : float mx[N][nchunk][2]
//             backward: double csp[N * GN_PLANES_CAP][C] | float mx[N][nchunk][2]
//   stats : [ float (mean, rstd)[N][G] | float cb[N][C][4] (per-channel affine) | float gb[N][G][4] ] -- the two tables the forward finalize derives
//           are kept so that the backward reads them instead of re-deriving them with one more 8-block launch per norm (30 x 6.7 us per smoke
//           training step; a launch that small costs its full duration, measured by removing the equally small column sums: -0.13 ms per step).
struct gn_plan {
  int rc;                            // gn_check of the shape; the launch shapes and the pointers are set only when it is WDNO_OK
  size_t ws_bytes, fwd_planes_bytes, bwd_planes_bytes, tail;
  int nchunk, txp;                   // gn_partial: row chunks per sample; threads across the channel quads of a row
  int64_t rows_per_chunk;
  unsigned slices;                   // finalize kernels: blocks per sample
  int grid4, grid8, planes_grid;     // blocks per sample: fp32 apply passes, forward planes passes, backward planes pass
  double* part;
  float *cb, *gb;
  float* mx;                         // forward planes forms
  double* csp;                       // backward planes form, its mx behind the column-sum partials
  float* mx_bwd;
};
static gn_plan gn_make_plan(int64_t N, int64_t S, int C, int G, void* ws = nullptr, const float* stats = nullptr) {
  gn_plan p = {};
  p.nchunk = gn_chunks(S, N, C);
  const size_t mx_bytes = (size_t)N * p.nchunk * 2 * sizeof(float), csp_bytes = (size_t)N * GN_PLANES_CAP * C * sizeof(double);
  p.ws_bytes = (size_t)N * p.nchunk * C * 2 * sizeof(double) + (size_t)N * C * 4 * sizeof(float) + (size_t)N * G * 4 * sizeof(float) + 64;
  p.fwd_planes_bytes = p.ws_bytes + mx_bytes + 128;
  p.bwd_planes_bytes = p.ws_bytes + mx_bytes + csp_bytes + 64;
  p.tail = (p.ws_bytes + 63) & ~(size_t)63;
  p.rc = gn_check(N, S, C, G);
  if (p.rc) return p;
  p.txp = pow2ceil(C / 4);
  p.rows_per_chunk = cdiv64(S, p.nchunk);
  p.slices = gn_slices(C, G);
  p.grid4 = gn_apply_grid(S, C, 4);
  p.grid8 = gn_apply_grid(S, C, 8);
  p.planes_grid = gn_planes_grid(N, S, C);
  if (!ws || !stats) return p;       // a size or tail query
  p.part = (double*)ws;
  p.cb = const_cast<float*>(stats) + (size_t)N * G * 2;
  p.gb = p.cb + (size_t)N * C * 4;      // entries 2, 3 of a group are the backward's own (the two group means): written by gn_bwd_finalize_kernel
  p.mx = (float*)((char*)ws + p.tail);
  p.csp = (double*)((char*)ws + p.tail);
  p.mx_bwd = (float*)(p.csp + (size_t)N * GN_PLANES_CAP * C);
  return p;
}
extern "C" size_t wdno_groupnorm_ws_bytes(int64_t N, int64_t S, int C, int G) { return gn_make_plan(N, S, C, G).ws_bytes; }
extern "C" size_t wdno_groupnorm_fwd_planes_ws_bytes(int64_t N, int64_t S, int C, int G) { return gn_make_plan(N, S, C, G).fwd_planes_bytes; }
extern "C" size_t wdno_groupnorm_bwd_planes_ws_bytes(int64_t N, int64_t S, int C, int G) { return gn_make_plan(N, S, C, G).bwd_planes_bytes; }
extern "C" size_t wdno_groupnorm_stats_floats(int64_t N, int C, int G) { return (size_t)N * G * 2 + (size_t)N * C * 4 + (size_t)N * G * 4; }
// where the column-sum partials of dx live inside ws (doubles [rows][C]) when the backward is called with dx_colsum == NULL
extern "C" int wdno_groupnorm_bwd_planes_tail(int64_t N, int64_t S, int C, int G, size_t* csp_offset, int* rows) {
  const gn_plan p = gn_make_plan(N, S, C, G);
  if (p.rc) return p.rc;
  WDNO_REQUIRE(csp_offset && rows);
  *csp_offset = p.tail;
  *rows = (int)N * p.planes_grid;
  return WDNO_OK;
}

// x_bf16 / dy_bf16 (the _t entry points): the tensor is bf16 storage (gn_bf16); arithmetic and every other operand unchanged.
// Runs the statement with XT / DT naming the storage types of x and dy (a statement that names XT only passes dy_bf16 = 0).
#define GN_WITH_TYPES(XB, DB, ...) do { \
    if (XB) { using XT = gn_bf16; if (DB) { using DT = gn_bf16; __VA_ARGS__; } else { using DT = float; __VA_ARGS__; } } \
    else { using XT = float; if (DB) { using DT = gn_bf16; __VA_ARGS__; } else { using DT = float; __VA_ARGS__; } } } while (0)

extern "C" int wdno_groupnorm_act_fwd_amax_t(const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, float* y,
                                      float* stats, float* amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                      void* ws, size_t ws_bytes, wdno_stream_t s) {
  const gn_plan p = gn_make_plan(N, S, C, G, ws, stats);
  if (p.rc) return p.rc;
  if (ws_bytes < p.ws_bytes) return WDNO_EWORKSPACE;
  hipStream_t st = as_stream(s);
  GN_WITH_TYPES(x_bf16, 0, gn_partial_kernel<0, XT><<<dim3(p.nchunk, (unsigned)N), 256, 0, st>>>(x, nullptr, nullptr, nullptr, p.part, S, C, C / G, G, p.txp,
                                                                                               p.rows_per_chunk, 0));
  gn_finalize_kernel<<<dim3((unsigned)N, p.slices), 256, 0, st>>>(p.part, nullptr, gamma, beta, ss, stats, p.cb, p.gb, S, C, G, p.nchunk, eps);
  GN_WITH_TYPES(x_bf16, 0, gn_apply_kernel<XT><<<dim3(p.grid4, (unsigned)N), 256, 0, st>>>(x, p.cb, y, S, C, silu, amax_rec));
  return wdno_check_launch();
}
extern "C" int wdno_groupnorm_act_fwd_amax(const float* x, const float* gamma, const float* beta, const float* ss, float* y,
                                      float* stats, float* amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                      void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_groupnorm_act_fwd_amax_t(x, 0, gamma, beta, ss, y, stats, amax_rec, N, S, C, G, eps, silu, ws, ws_bytes, s);
}
extern "C" int wdno_groupnorm_act_fwd(const float* x, const float* gamma, const float* beta, const float* ss, float* y,
                                      float* stats, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                      void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_groupnorm_act_fwd_amax(x, gamma, beta, ss, y, stats, nullptr, N, S, C, G, eps, silu, ws, ws_bytes, s);
}
extern "C" int wdno_groupnorm_act_bwd_amax(const float* x, const float* dy, const float* gamma, const float* beta, const float* ss,
                                      const float* stats, float* dx, float* dgb_partial, float* dss, float* amax_rec,
                                      int64_t N, int64_t S, int C, int G, int silu, void* ws, size_t ws_bytes, wdno_stream_t s) {
  const gn_plan p = gn_make_plan(N, S, C, G, ws, stats);
  if (p.rc) return p.rc;
  if (ws_bytes < p.ws_bytes) return WDNO_EWORKSPACE;
  hipStream_t st = as_stream(s);
  gn_partial_kernel<1><<<dim3(p.nchunk, (unsigned)N), 256, 0, st>>>(x, dy, p.cb, p.gb, p.part, S, C, C / G, G, p.txp, p.rows_per_chunk, silu);
  gn_bwd_finalize_kernel<<<dim3((unsigned)N, p.slices), 256, 0, st>>>(p.part, gamma, beta, ss, p.gb, dgb_partial, dss, S, C, G, p.nchunk);
  gn_bwd_apply_kernel<<<dim3(p.grid4, (unsigned)N), 256, 0, st>>>(x, dy, p.cb, p.gb, dx, S, C, C / G, G, silu, amax_rec);
  return wdno_check_launch();
}
extern "C" int wdno_groupnorm_act_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* ss,
                                      const float* stats, float* dx, float* dgb_partial, float* dss,
                                      int64_t N, int64_t S, int C, int G, int silu, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_groupnorm_act_bwd_amax(x, dy, gamma, beta, ss, stats, dx, dgb_partial, dss, nullptr, N, S, C, G, silu, ws, ws_bytes, s);
}

// the statistics passes of both forward planes forms; with two planes the partial pass leaves its maxima in mx and the finalize its bound in bound_rec
static void gn_fwd_planes_stats(const gn_plan& p, const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, float* stats,
                                float* bound_rec, bool two_planes, int64_t N, int64_t S, int C, int G, float eps, hipStream_t st) {
  GN_WITH_TYPES(x_bf16, 0, gn_partial_kernel<0, XT><<<dim3(p.nchunk, (unsigned)N), 256, 0, st>>>(x, nullptr, nullptr, nullptr, p.part, S, C, C / G, G, p.txp,
                                                                                               p.rows_per_chunk, 0, two_planes ? p.mx : nullptr));
  gn_finalize_kernel<<<dim3((unsigned)N, p.slices), 256, 0, st>>>(p.part, nullptr, gamma, beta, ss, stats, p.cb, p.gb, S, C, G, p.nchunk, eps, p.mx,
                                                                  two_planes ? bound_rec : nullptr);
}
extern "C" int wdno_groupnorm_act_fwd_planes_t(const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, void* y_hi, void* y_lo,
                                             float* y_scale, float* stats, float* bound_rec, int64_t N, int64_t S, int C, int G, float eps,
                                             int silu, void* ws, size_t ws_bytes, wdno_stream_t s) {
  const gn_plan p = gn_make_plan(N, S, C, G, ws, stats);
  if (p.rc) return p.rc;
  if (!gn_planes_ok(C)) return WDNO_EUNSUPPORTED;
  if (ws_bytes < p.fwd_planes_bytes) return WDNO_EWORKSPACE;
  hipStream_t st = as_stream(s);
  gn_fwd_planes_stats(p, x, x_bf16, gamma, beta, ss, stats, bound_rec, y_lo != nullptr, N, S, C, G, eps, st);
  GN_WITH_TYPES(x_bf16, 0, gn_apply_planes_kernel<XT><<<dim3(p.grid8, (unsigned)N), 256, 0, st>>>(x, p.cb, (_Float16*)y_hi, (_Float16*)y_lo, y_scale, bound_rec,
                                                                                                S, C, silu));
  return wdno_check_launch();
}
extern "C" int wdno_groupnorm_act_fwd_planes(const float* x, const float* gamma, const float* beta, const float* ss, void* y_hi, void* y_lo,
                                             float* y_scale, float* stats, float* bound_rec, int64_t N, int64_t S, int C, int G, float eps,
                                             int silu, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_groupnorm_act_fwd_planes_t(x, 0, gamma, beta, ss, y_hi, y_lo, y_scale, stats, bound_rec, N, S, C, G, eps, silu, ws, ws_bytes, s);
}

extern "C" int wdno_groupnorm_act_add_fwd_planes_t(const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, const float* residual,
                                                 const float* res_rec, float* y, void* y_hi, void* y_lo, float* y_scale, float* stats,
                                                 float* bound_rec, float* y_amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                                 void* ws, size_t ws_bytes, wdno_stream_t s) {
  const gn_plan p = gn_make_plan(N, S, C, G, ws, stats);
  if (p.rc) return p.rc;
  if (!gn_planes_ok(C)) return WDNO_EUNSUPPORTED;
  if (!residual || !y || (y_lo && (!y_hi || !res_rec || !bound_rec || !y_scale))) return WDNO_EINVAL;      // y_hi == NULL: fp32 sum only
  if (ws_bytes < p.fwd_planes_bytes) return WDNO_EWORKSPACE;
  hipStream_t st = as_stream(s);
  gn_fwd_planes_stats(p, x, x_bf16, gamma, beta, ss, stats, bound_rec, y_lo != nullptr, N, S, C, G, eps, st);
  GN_WITH_TYPES(x_bf16, 0, gn_apply_add_planes_kernel<XT><<<dim3(p.grid8, (unsigned)N), 256, 0, st>>>(x, p.cb, residual, y, (_Float16*)y_hi, (_Float16*)y_lo,
                                                                                                    y_scale, bound_rec, res_rec, y_amax_rec, S, C, silu));
  return wdno_check_launch();
}
extern "C" int wdno_groupnorm_act_add_fwd_planes(const float* x, const float* gamma, const float* beta, const float* ss, const float* residual,
                                                 const float* res_rec, float* y, void* y_hi, void* y_lo, float* y_scale, float* stats,
                                                 float* bound_rec, float* y_amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                                 void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_groupnorm_act_add_fwd_planes_t(x, 0, gamma, beta, ss, residual, res_rec, y, y_hi, y_lo, y_scale, stats, bound_rec, y_amax_rec, N, S, C, G, eps, silu,
                                             ws, ws_bytes, s);
}

extern "C" int wdno_groupnorm_act_bwd_planes_t(const void* x, int x_bf16, const void* dy, int dy_bf16, const float* gamma, const float* beta, const float* ss,
                                             const float* stats, void* dx_hi, void* dx_lo, float* dx_scale, float* dx_colsum,
                                             float* dgb_partial, float* dgb_sum, float* dss, float* bound_rec, int64_t N, int64_t S, int C, int G, int silu,
                                             void* ws, size_t ws_bytes, wdno_stream_t s) {
  const gn_plan p = gn_make_plan(N, S, C, G, ws, stats);
  if (p.rc) return p.rc;
  if (!gn_planes_ok(C)) return WDNO_EUNSUPPORTED;
  if (ws_bytes < p.bwd_planes_bytes) return WDNO_EWORKSPACE;
  hipStream_t st = as_stream(s);
  const int gx = p.planes_grid;
  GN_WITH_TYPES(x_bf16, dy_bf16, gn_partial_kernel<1, XT, DT><<<dim3(p.nchunk, (unsigned)N), 256, 0, st>>>(x, dy, p.cb, p.gb, p.part, S, C, C / G, G, p.txp,
                                                                                                         p.rows_per_chunk, silu, dx_lo ? p.mx_bwd : nullptr));
  gn_bwd_finalize_kernel<<<dim3((unsigned)N, p.slices), 256, 0, st>>>(p.part, gamma, beta, ss, p.gb, dgb_partial, dss, S, C, G, p.nchunk, p.cb, p.mx_bwd,
                                                                      dx_lo ? bound_rec : nullptr);
  GN_WITH_TYPES(x_bf16, dy_bf16, gn_bwd_apply_planes_kernel<XT, DT><<<dim3(gx, (unsigned)N), 256, 0, st>>>(x, dy, p.cb, p.gb, (_Float16*)dx_hi, (_Float16*)dx_lo,
                                                                                                         dx_scale, bound_rec, p.csp, S, C, C / G, G, silu));
  // one launch for both reductions that end the backward: the column sums of dx (partials of the apply pass) and, when dgb_sum is given, the
  // sum over the samples of the per-sample parameter-gradient pieces (was a colsum_rows launch of the caller: same fp64 sum in row order)
  // (dx_colsum == NULL: the caller sums the partials later with everything else that ends the backward -- wdno_rows_sum_multi over the
  // N * gx rows at wdno_groupnorm_bwd_planes_tail's offset of ws, and over the N rows of dgb_partial)
  const int nbx = dx_colsum ? cdiv(C, 32) : 0, nby = dgb_sum ? cdiv(2 * C, 32) : 0;
  if (nbx + nby) gn_bwd_tail_kernel<<<nbx + nby, PRS_THREADS, 0, st>>>(p.csp, dx_colsum, (int)N * gx, C, nbx, dgb_partial, dgb_sum, (int)N);
  return wdno_check_launch();
}

extern "C" int wdno_groupnorm_act_bwd_planes(const float* x, const float* dy, const float* gamma, const float* beta, const float* ss,
                                             const float* stats, void* dx_hi, void* dx_lo, float* dx_scale, float* dx_colsum,
                                             float* dgb_partial, float* dgb_sum, float* dss, float* bound_rec, int64_t N, int64_t S, int C, int G, int silu,
                                             void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_groupnorm_act_bwd_planes_t(x, 0, dy, 0, gamma, beta, ss, stats, dx_hi, dx_lo, dx_scale, dx_colsum, dgb_partial, dgb_sum, dss, bound_rec, N, S, C, G,
                                         silu, ws, ws_bytes, s);
}
