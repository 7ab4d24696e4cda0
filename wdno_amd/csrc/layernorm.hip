// layernorm.hip -- channel LayerNorm on channels-last rows (HBM-bound). GroupNorm is norm.hip.
#include "common.h"

// ---------------------------------------------------------------------------------------------- channel LayerNorm
// rows [P][C]; a row is handled by TPR lanes holding VPL float4 each. y = (x - mean) / sqrt(var + eps) * g
template <int TPR, int VPL, bool BWD>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ dy, float* __restrict__ out,
                                                         float* __restrict__ dg_part, int64_t P, int C, float eps,
                                                         const float* __restrict__ add_to, float* __restrict__ dx_amax,
                                                         _Float16* __restrict__ y_hi = nullptr, _Float16* __restrict__ y_lo = nullptr,
                                                         float* __restrict__ y_scale = nullptr) {
  constexpr int RPB = 256 / TPR;
  __shared__ float red[BWD ? 256 * VPL * 4 : 1];
  const int C4 = C >> 2;
  const int lane = threadIdx.x % TPR, rloc = threadIdx.x / TPR;
  float4 gv[VPL];
  bool cok[VPL];
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    int c4 = lane + v * TPR;
    cok[v] = c4 < C4;
    gv[v] = cok[v] ? reinterpret_cast<const float4*>(g)[c4] : make_float4(0, 0, 0, 0);
  }
  float dgacc[VPL][4];
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int j = 0; j < 4; ++j) dgacc[v][j] = 0.f;
  const float invC = 1.0f / (float)C;
  const int64_t rstride = (int64_t)gridDim.x * RPB;
  float ps = 1.0f;                 // forward with planes output: |y| = |xhat g| <= sqrt(C) max|g|, a scale every block derives by itself
  if (!BWD && y_hi && y_lo) {
    float mg = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) mg = amax4(mg, gv[v]);
    ps = scale_from_amax(sqrtf((float)C) * group_max<TPR>(mg));
    if (blockIdx.x == 0 && threadIdx.x == 0) y_scale[0] = ps;
  }
  float am = 0.f;       // max|y| (forward: left in the amax record dg_part points to, if any) / max|dx| (backward: in dx_amax, if any)
  // all lanes of a row group iterate together (uniform trip count per group)
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < P; r0 += rstride) {
    int64_t r = r0 + rloc;
    bool rok = r < P;
    float4 xv[VPL];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      xv[v] = (rok && cok[v]) ? reinterpret_cast<const float4*>(x + r * C)[lane + v * TPR] : make_float4(0, 0, 0, 0);
      s += (xv[v].x + xv[v].y) + (xv[v].z + xv[v].w);
    }
    float mean = group_sum<TPR>(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      if (cok[v]) {
        xv[v].x -= mean; xv[v].y -= mean; xv[v].z -= mean; xv[v].w -= mean;
        q += (xv[v].x * xv[v].x + xv[v].y * xv[v].y) + (xv[v].z * xv[v].z + xv[v].w * xv[v].w);
      }
    }
    float var = group_sum<TPR>(q) * invC;
    float rstd = 1.0f / sqrtf(var + eps);
    if (!BWD) {
#pragma unroll
      for (int v = 0; v < VPL; ++v)
        if (rok && cok[v]) {
          float4 o;
          o.x = xv[v].x * rstd * gv[v].x; o.y = xv[v].y * rstd * gv[v].y;
          o.z = xv[v].z * rstd * gv[v].z; o.w = xv[v].w * rstd * gv[v].w;
          if (y_hi) {
            typedef _Float16 half4v __attribute__((ext_vector_type(4)));
            const float t[4] = {o.x, o.y, o.z, o.w};
            half4v h, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) { _Float16 th, tl; plane_pack(t[j], ps, y_lo == nullptr, th, tl); h[j] = th; l[j] = tl; }
            reinterpret_cast<half4v*>(y_hi + r * C)[lane + v * TPR] = h;
            if (y_lo) reinterpret_cast<half4v*>(y_lo + r * C)[lane + v * TPR] = l;
            continue;
          }
          reinterpret_cast<float4*>(out + r * C)[lane + v * TPR] = o;
          am = amax4(am, o);
        }
    } else {
      float4 dv[VPL];
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        dv[v] = (rok && cok[v]) ? reinterpret_cast<const float4*>(dy + r * C)[lane + v * TPR] : make_float4(0, 0, 0, 0);
        // xhat in xv, dxhat = dy * g
        xv[v].x *= rstd; xv[v].y *= rstd; xv[v].z *= rstd; xv[v].w *= rstd;
        dgacc[v][0] += dv[v].x * xv[v].x; dgacc[v][1] += dv[v].y * xv[v].y;
        dgacc[v][2] += dv[v].z * xv[v].z; dgacc[v][3] += dv[v].w * xv[v].w;
        dv[v].x *= gv[v].x; dv[v].y *= gv[v].y; dv[v].z *= gv[v].z; dv[v].w *= gv[v].w;
        m1 += (dv[v].x + dv[v].y) + (dv[v].z + dv[v].w);
        m2 += (dv[v].x * xv[v].x + dv[v].y * xv[v].y) + (dv[v].z * xv[v].z + dv[v].w * xv[v].w);
      }
      m1 = group_sum<TPR>(m1) * invC;
      m2 = group_sum<TPR>(m2) * invC;
#pragma unroll
      for (int v = 0; v < VPL; ++v)
        if (rok && cok[v]) {
          float4 o;
          o.x = rstd * (dv[v].x - m1 - xv[v].x * m2); o.y = rstd * (dv[v].y - m1 - xv[v].y * m2);
          o.z = rstd * (dv[v].z - m1 - xv[v].z * m2); o.w = rstd * (dv[v].w - m1 - xv[v].w * m2);
          if (add_to) {          // the gradient arriving at x over the skip connection of Residual(PreNorm(fn)): one add launch less
            const float4 t = reinterpret_cast<const float4*>(add_to + r * C)[lane + v * TPR];
            o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
          }
          reinterpret_cast<float4*>(out + r * C)[lane + v * TPR] = o;
          am = amax4(am, o);
        }
    }
  }
  if (!BWD && dg_part) amax_record_emit(am, dg_part, blockIdx.x);
  if (BWD && dx_amax) amax_record_emit(am, dx_amax, blockIdx.x);
  if (BWD) {
    // reduce dg over the RPB row groups of the block, write one partial row per block
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[((rloc * TPR + lane) * VPL + v) * 4 + j] = dgacc[v][j];
    __syncthreads();
    if (rloc == 0) {
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        if (!cok[v]) continue;
        float a[4] = {0, 0, 0, 0};
        for (int t = 0; t < RPB; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += red[((t * TPR + lane) * VPL + v) * 4 + j];
        reinterpret_cast<float4*>(dg_part + (int64_t)blockIdx.x * C)[lane + v * TPR] = make_float4(a[0], a[1], a[2], a[3]);
      }
    }
  }
}

static inline int ln_blocks(int64_t P, int rpb) {
  int64_t nb = cdiv64(P, rpb);
  if (nb > 1024) nb = 1024;
  return (int)nb;
}
static inline void ln_shape(int C, int& tpr, int& vpl) {
  int c4 = C / 4;
  if (c4 <= 64) { tpr = pow2ceil(c4); if (tpr < 2) tpr = 2; vpl = 1; }
  else { tpr = 64; vpl = pow2ceil(cdiv(c4, 64)); }
}
// The argument checks and the launch shape of P rows of C channels, for every entry point (ln_launch and wdno_layernorm_plan ask here).
// cmul: the channel multiple of the form -- 4, or 8 for the planes output (plane rows are whole groups of 8 channels).
static int ln_choose(int64_t P, int C, wdno_ln_plan& pl, int cmul = 4) {
  pl = wdno_ln_plan{0, 0, 0, 0, 0, WDNO_OK};
  if (!(P > 0 && C >= cmul)) return pl.rc = WDNO_EINVAL;
  if ((C & (cmul - 1)) || C > 1024) return pl.rc = WDNO_EUNSUPPORTED;
  ln_shape(C, pl.tpr, pl.vpl);
  pl.rows_per_block = 256 / pl.tpr;
  pl.blocks = ln_blocks(P, pl.rows_per_block);
  pl.max_rows_walk = (int)cdiv64(P, (int64_t)pl.blocks * pl.rows_per_block);
  return WDNO_OK;
}
extern "C" int wdno_layernorm_plan(int64_t P, int C, wdno_ln_plan* out) {
  if (!out) return WDNO_EINVAL;
  ln_choose(P, C, *out);
  return WDNO_OK;
}
extern "C" size_t wdno_layernorm_bwd_ws_bytes(int64_t P, int C) { return (size_t)1024 * C * sizeof(float); }
// checks, chooses (the plan is handed back in pl) and launches. The backward leaves one row of dg partials per block in dgp: dgp_bytes behind it.
template <bool BWD, int CMUL = 4>
static int ln_launch(wdno_ln_plan& pl, const float* x, const float* g, const float* dy, float* out, float* dgp, size_t dgp_bytes, int64_t P, int C,
                     float eps, hipStream_t st, const float* add_to = nullptr, float* dx_amax = nullptr, _Float16* y_hi = nullptr,
                     _Float16* y_lo = nullptr, float* y_scale = nullptr) {
  int rc = ln_choose(P, C, pl, CMUL);
  if (rc) return rc;
  if (BWD && dgp_bytes < wdno_layernorm_bwd_ws_bytes(P, C)) return WDNO_EWORKSPACE;
  const int tpr = pl.tpr, vpl = pl.vpl, nb = pl.blocks;
#define LN_CASE(T, V) layernorm_kernel<T, V, BWD><<<nb, 256, 0, st>>>(x, g, dy, out, dgp, P, C, eps, add_to, dx_amax, y_hi, y_lo, y_scale)
  if (vpl == 1) {
    switch (tpr) {
      case 2: LN_CASE(2, 1); break;
      case 4: LN_CASE(4, 1); break;
      case 8: LN_CASE(8, 1); break;
      case 16: LN_CASE(16, 1); break;
      case 32: LN_CASE(32, 1); break;
      default: LN_CASE(64, 1); break;
    }
  } else if (vpl == 2) LN_CASE(64, 2);
  else if (vpl == 4) LN_CASE(64, 4);
  else return WDNO_EUNSUPPORTED;
#undef LN_CASE
  return WDNO_OK;
}
extern "C" int wdno_layernorm_fwd_amax(const float* x, const float* g, float* y, float* amax_rec, int64_t P, int C, float eps,
                                       wdno_stream_t s) {
  wdno_ln_plan pl;
  int rc = ln_launch<false>(pl, x, g, nullptr, y, amax_rec, 0, P, C, eps, as_stream(s));
  if (rc) return rc;
  return wdno_check_launch();
}
extern "C" int wdno_layernorm_fwd_planes(const float* x, const float* g, void* y_hi, void* y_lo, float* y_scale, int64_t P, int C, float eps,
                                         wdno_stream_t s) {
  wdno_ln_plan pl;
  int rc = ln_launch<false, 8>(pl, x, g, nullptr, nullptr, nullptr, 0, P, C, eps, as_stream(s), nullptr, nullptr, (_Float16*)y_hi, (_Float16*)y_lo, y_scale);
  if (rc) return rc;
  return wdno_check_launch();
}
extern "C" int wdno_layernorm_fwd(const float* x, const float* g, float* y, int64_t P, int C, float eps, wdno_stream_t s) {
  return wdno_layernorm_fwd_amax(x, g, y, nullptr, P, C, eps, s);
}
extern "C" int wdno_layernorm_bwd_add_amax(const float* x, const float* g, const float* dy, const float* add_to, float* dx, float* dg,
                                           float* amax_rec, int64_t P, int C, float eps, void* ws, size_t ws_bytes, wdno_stream_t s) {
  wdno_ln_plan pl;
  int rc = ln_launch<true>(pl, x, g, dy, dx, (float*)ws, ws_bytes, P, C, eps, as_stream(s), add_to, amax_rec);
  if (rc) return rc;
  partial_rows_sum_kernel<float><<<cdiv(C, 32), PRS_THREADS, 0, as_stream(s)>>>((const float*)ws, dg, pl.blocks, C);
  return wdno_check_launch();
}
extern "C" int wdno_layernorm_bwd_add(const float* x, const float* g, const float* dy, const float* add_to, float* dx, float* dg, int64_t P,
                                      int C, float eps, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_layernorm_bwd_add_amax(x, g, dy, add_to, dx, dg, nullptr, P, C, eps, ws, ws_bytes, s);
}
extern "C" int wdno_layernorm_bwd(const float* x, const float* g, const float* dy, float* dx, float* dg, int64_t P, int C,
                                  float eps, void* ws, size_t ws_bytes, wdno_stream_t s) {
  return wdno_layernorm_bwd_add(x, g, dy, nullptr, dx, dg, P, C, eps, ws, ws_bytes, s);
}
