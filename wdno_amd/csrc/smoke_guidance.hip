// smoke_guidance.hip -- the gradient of the smoke control objective (smoke/inference_2d.py:30-66) in closed form, as TWO launches that turn
// the U-Net's noise estimate into the guided one (diffusion_2d.py:723-754): predict x0, rescale, 3-D synthesis of what J reads, residual
// (launch 1) -- adjoint synthesis, schedule, add, and the copy of everything J does not reach (launch 2). include/wdno_hip.h states the
// mathematics; wdno_amd/smoke/guidance.py: plan() chooses the tiles.
//
// Zero-mode filter bank of L = 6 taps (bior1.3), off = L - 2 = 4, one axis (csrc/dwt.hip: the per-axis synthesis_kernel / analysis_kernel with reversed taps):
//   synthesis  x[n]  = sum over m < L with n + 4 - m even, K = (n + 4 - m) / 2 in [0, M):  lo[K] g_lo[m] + hi[K] g_hi[m]        (N = 2M - 4)
//   adjoint    dlo[K] = sum over m < L with n = 2K + m - 4 in [0, N):  g_lo[m] r[n],   dhi likewise
// in the order W, H, T (synthesis) and T, H, W (adjoint) with band = 4 bt + 2 bh + bw, the channel of field f being 8 f + band.
//
// Launch 1, synthesis_kernel: one workgroup of 256 threads per (sample, field, tile of tn reconstruction frames x hn rows, full width).
//   Output frames [n0, n0 + tn) read coefficient frames n0/2 .. n0/2 + tn/2 + 1 (KT = tn/2 + 2; rows alike, KH = hn/2 + 2): the tile stages
//   them band pair by band pair (ST), x0 RESCALER formed on the fly from (x_t, eps) in place in the packed state, and runs the W pass into S1,
//   the H pass into S2 and the T pass into registers, from where the scaled, cropped residual goes to the workspace. Fields 3 and 4 are
//   synthesised in full, field 0 on its frame tile 0 only (J reads frame 0).
// Launch 2, adjoint_kernel: one workgroup per (sample, field, tile of kt coefficient frames x kh rows, full width). It reads the 2 kt + 4
//   residual frames x 2 kh + 4 rows within the filter's reach (zero outside the crop), T pass from global into A1, H pass into A2, W pass
//   into registers, and writes out = eps + s g for the 8 channels of its tile (columns >= wc: the copy). Field 0 has tiles on coefficient
//   frames < 3 only: frame 0 of the reconstruction reaches no further. All workgroups of a sample, and `ncopy` more, share the rest of
//   the tensor: a copy of eps (zeros in gradient mode), plus the constant term on the smoke-out channel.
// Every sum runs over m ascending in fmaf chains of fixed length, nothing is atomic: a sample's bits do not depend on the batch.
#include "common.h"

namespace {

constexpr int L = 6;
constexpr int NT = 256;

struct STaps { float lo[L], hi[L]; };      // rec_lo, rec_hi

struct SGuidP {
  const float* xt; const float* in; float* out; float* ws;
  const int64_t* t; const float* c1; const float* c2; const float* s; const float* resc; const float* init_u; const float* succ;
  int F, C, H, W;
  int64_t ss; int fs, cs, rs;                // strides of sample, frame, channel, row (elements)
  int tc, hc, wc, to, ho, wo;
  int half, T, clip, cc;
  int use0, use34;                           // which residuals exist: field 0 (init_u given, w_init != 0), fields 3 and 4 (not cc, w_energy != 0)
  int tn, hn, kt, kh;                        // tiles of launch 1 (reconstruction frames, rows; even) and of launch 2 (coefficient frames, rows)
  int vec;                                   // the shared copy moves float4
  float ce, ci;                              // 2 w_energy / (2 to ho wo) and 2 w_init / (ho wo)
};

// per-sample scalars and the two element-wise ends of the chain
struct SGuidS {
  bool fused; float c1, c2, s;
  __device__ __forceinline__ void init(const SGuidP& p, int b) {
    fused = p.xt != nullptr;
    c1 = c2 = s = 0.f;
    if (fused) {
      long long tb = p.t[b];
      tb = tb < 0 ? 0 : (tb >= p.T ? p.T - 1 : tb);
      c1 = p.c1[tb]; c2 = p.c2[tb]; s = p.s[tb];
    }
  }
  __device__ __forceinline__ float coef(const SGuidP& p, size_t idx, int ch) const {      // (x0 RESCALER) at one element
    float v = p.in[idx];
    if (fused) {
      v = __fadd_rn(__fmul_rn(c1, p.xt[idx]), -__fmul_rn(c2, v));
      if (p.clip) v = fminf(fmaxf(v, -1.f), 1.f);
    }
    return __fmul_rn(v, p.resc[ch]);
  }
  __device__ __forceinline__ float guided(float in, float g) const {      // in = eps (fused) or anything (gradient mode)
    if (!fused) return g;
    return g == 0.f ? in : __fadd_rn(in, __fmul_rn(g, s));
  }
};

// workspace of one sample: fields 3 and 4 [2][to][ho][wo], then frame 0 of field 0 [ho][wo]
__device__ __forceinline__ size_t ws_sample(const SGuidP& p) { return (size_t)(2 * p.to + 1) * p.ho * p.wo; }

// ------------------------------------------------------------------------------------------------------------------ launch 1
__global__ __launch_bounds__(NT) void smoke_guidance_synthesis_kernel(SGuidP p, STaps g) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int KT = p.tn / 2 + 2, KH = p.hn / 2 + 2;
  const int nft = (p.to + p.tn - 1) / p.tn, nrt = (p.ho + p.hn - 1) / p.hn;
  int blk = blockIdx.x, field, n0, nfo;
  const int n34 = p.use34 ? 2 * nft * nrt : 0;
  if (blk < n34) {
    const int slot = blk / (nft * nrt);
    blk -= slot * nft * nrt;
    field = 3 + slot;
    n0 = (blk / nrt) * p.tn;
    nfo = min(p.tn, p.to - n0);
    blk %= nrt;
  } else {
    blk -= n34;
    field = 0; n0 = 0; nfo = 1;
  }
  const int h0 = blk * p.hn, nro = min(p.hn, p.ho - h0);
  const int k0t = n0 / 2, k0h = h0 / 2, wo = p.wo, wc = p.wc;
  float* const ST = smem;                        // [2][KT][KH][wc]: one (bw = 0, 1) band pair of the tile's coefficients
  float* const S1 = ST + 2 * KT * KH * wc;       // [4][KT][KH][wo]: after the W pass, (bt, bh) major
  float* const S2 = S1 + 4 * KT * KH * wo;       // [2][KT][hn][wo]: after the H pass
  SGuidS q;
  q.init(p, b);
  const size_t base = (size_t)b * p.ss;
  for (int pair = 0; pair < 4; ++pair) {
    for (int idx = tid; idx < 2 * KT * KH * wc; idx += NT) {
      const int kw = idx % wc;
      int r = idx / wc;
      const int lh = r % KH; r /= KH;
      const int lt = r % KT, bw = r / KT;
      const int kf = k0t + lt, kr = k0h + lh, ch = 8 * field + 2 * pair + bw;
      float v = 0.f;
      if (kf < p.tc && kr < p.hc) v = q.coef(p, base + (size_t)kf * p.fs + (size_t)ch * p.cs + (size_t)kr * p.rs + kw, ch);
      ST[idx] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < KT * KH * wo; idx += NT) {
      const int n = idx % wo, row = idx / wo;
      const int par = n & 1, kb = (n + 4 - par) >> 1;      // taps m = par + 2 j read coefficient kb - j
      const float* lo = ST + row * wc;
      const float* hi = lo + KT * KH * wc;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int kk = kb - j;
        if (kk < wc) {
          acc = fmaf(lo[kk], par ? g.lo[2 * j + 1] : g.lo[2 * j], acc);
          acc = fmaf(hi[kk], par ? g.hi[2 * j + 1] : g.hi[2 * j], acc);
        }
      }
      S1[pair * KT * KH * wo + idx] = acc;
    }
    __syncthreads();
  }
  for (int idx = tid; idx < 2 * KT * p.hn * wo; idx += NT) {
    const int n = idx % wo;
    int r = idx / wo;
    const int dr = r % p.hn; r /= p.hn;
    const int lt = r % KT, bt = r / KT;
    const int row = h0 + dr, par = row & 1, kb = ((row + 4 - par) >> 1) - k0h;      // rows beyond hc were staged as zeros
    const float* lo = S1 + ((size_t)((2 * bt) * KT + lt) * KH) * wo + n;
    const float* hi = lo + KT * KH * wo;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc = fmaf(lo[(kb - j) * wo], par ? g.lo[2 * j + 1] : g.lo[2 * j], acc);
      acc = fmaf(hi[(kb - j) * wo], par ? g.hi[2 * j + 1] : g.hi[2 * j], acc);
    }
    S2[idx] = acc;
  }
  __syncthreads();
  float* const wsb = p.ws + (size_t)b * ws_sample(p);
  for (int idx = tid; idx < nfo * nro * wo; idx += NT) {
    const int n = idx % wo;
    int r = idx / wo;
    const int dr = r % nro, dn = r / nro;
    const int fr = n0 + dn, par = fr & 1, kb = ((fr + 4 - par) >> 1) - k0t;
    const float* lo = S2 + (size_t)dr * wo + n;
    const float* hi = lo + KT * p.hn * wo;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc = fmaf(lo[(kb - j) * p.hn * wo], par ? g.lo[2 * j + 1] : g.lo[2 * j], acc);
      acc = fmaf(hi[(kb - j) * p.hn * wo], par ? g.hi[2 * j + 1] : g.hi[2 * j], acc);
    }
    const int row = h0 + dr;
    if (field == 0)
      wsb[(size_t)2 * p.to * p.ho * wo + (size_t)row * wo + n] = __fmul_rn(__fadd_rn(acc, -p.init_u[((size_t)b * p.ho + row) * wo + n]), p.ci);
    else
      wsb[(((size_t)(field - 3) * p.to + fr) * p.ho + row) * wo + n] = __fmul_rn(acc, p.ce);
  }
}

// ------------------------------------------------------------------------------------------------------------------ launch 2
// the residual at (frame, row, column < wo) of a field, zero outside the crop
__device__ __forceinline__ float rload(const SGuidP& p, const float* wsb, int field, int fr, int row, int n) {
  if (row < 0 || row >= p.ho || fr < 0) return 0.f;
  if (field == 0) return fr == 0 ? wsb[(size_t)2 * p.to * p.ho * p.wo + (size_t)row * p.wo + n] : 0.f;
  return fr < p.to ? wsb[(((size_t)(field - 3) * p.to + fr) * p.ho + row) * p.wo + n] : 0.f;
}

// frames of field 0 whose coefficients frame 0 of the reconstruction reaches: 2 k + m - 4 = 0 for a tap m < L
__device__ __host__ __forceinline__ int reach0(int tc) { return tc < 3 ? tc : 3; }

__device__ __forceinline__ bool in_tiles(const SGuidP& p, int fr, int ch, int row) {      // written by an adjoint tile, not by the shared copy
  if (ch >= 40 || row >= p.hc) return false;
  const int f = ch >> 3;
  if (f == 0) return p.use0 && fr < reach0(p.tc);
  return f >= 3 && p.use34 && fr < p.tc;
}

__device__ __forceinline__ float succ_term(const SGuidP& p, int fr, int ch, int row) {   // g on the smoke-out channel, 0 elsewhere
  if (p.cc || ch != p.C - 1 || fr >= p.tc) return 0.f;
  return row < p.half ? -__fdiv_rn(p.succ[fr], (float)(p.half * p.W)) : -__fdiv_rn(p.succ[p.tc + fr], (float)((p.H - p.half) * p.W));
}

__global__ __launch_bounds__(NT) void smoke_guidance_adjoint_kernel(SGuidP p, STaps g, int ntiles) {
  extern __shared__ __align__(16) float smem[];
  const int tid = threadIdx.x, b = blockIdx.y;
  SGuidS q;
  q.init(p, b);
  const size_t base = (size_t)b * p.ss;
  if ((int)blockIdx.x < ntiles) {
    const int kt = p.kt, kh = p.kh, wo = p.wo, RH = 2 * kh + 4;
    const int nkt = (p.tc + kt - 1) / kt, nkt0 = (reach0(p.tc) + kt - 1) / kt, nkr = (p.hc + kh - 1) / kh;
    int blk = blockIdx.x, field, tcf;
    const int n34 = p.use34 ? 2 * nkt * nkr : 0;
    if (blk < n34) {
      const int slot = blk / (nkt * nkr);
      blk -= slot * nkt * nkr;
      field = 3 + slot; tcf = p.tc;
    } else {
      blk -= n34;
      field = 0; tcf = reach0(p.tc);
    }
    const int k0 = (blk / nkr) * kt, r0 = (blk % nkr) * kh;
    const int nk = min(kt, tcf - k0), nr = min(kh, p.hc - r0);
    float* const A1 = smem;                       // [2][kt][RH][wo]: after the T pass, bt major
    float* const A2 = A1 + 2 * kt * RH * wo;      // [4][kt][kh][wo]: after the H pass, (bt, bh) major
    const float* const wsb = p.ws + (size_t)b * ws_sample(p);
    for (int idx = tid; idx < kt * RH * wo; idx += NT) {
      const int n = idx % wo;
      int r = idx / wo;
      const int lr = r % RH, lk = r / RH;
      const int row = 2 * r0 - 4 + lr, f0 = 2 * (k0 + lk) - 4;
      float lo = 0.f, hi = 0.f;
#pragma unroll
      for (int m = 0; m < L; ++m) {
        const float v = rload(p, wsb, field, f0 + m, row, n);
        lo = fmaf(g.lo[m], v, lo);
        hi = fmaf(g.hi[m], v, hi);
      }
      A1[idx] = lo;
      A1[kt * RH * wo + idx] = hi;
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * kt * kh * wo; idx += NT) {
      const int n = idx % wo;
      int r = idx / wo;
      const int lh = r % kh; r /= kh;
      const int lk = r % kt, bt = r / kt;
      const float* a = A1 + ((size_t)(bt * kt + lk) * RH + 2 * lh) * wo + n;
      float lo = 0.f, hi = 0.f;
#pragma unroll
      for (int m = 0; m < L; ++m) {
        const float v = a[m * wo];
        lo = fmaf(g.lo[m], v, lo);
        hi = fmaf(g.hi[m], v, hi);
      }
      A2[((size_t)((2 * bt) * kt + lk) * kh + lh) * wo + n] = lo;
      A2[((size_t)((2 * bt + 1) * kt + lk) * kh + lh) * wo + n] = hi;
    }
    __syncthreads();
    for (int idx = tid; idx < 8 * nk * nr * p.W; idx += NT) {
      const int col = idx % p.W;
      int r = idx / p.W;
      const int lh = r % nr; r /= nr;
      const int lk = r % nk, band = r / nk;
      const int ch = 8 * field + band;
      const size_t at = base + (size_t)(k0 + lk) * p.fs + (size_t)ch * p.cs + (size_t)(r0 + lh) * p.rs + col;
      float gv = 0.f;
      if (col < p.wc) {
        const float* a = A2 + ((size_t)((band >> 1) * kt + lk) * kh + lh) * wo;
#pragma unroll
        for (int m = 0; m < L; ++m) {
          const int n = 2 * col + m - 4;
          const float v = (n >= 0 && n < wo) ? a[n] : 0.f;
          gv = fmaf((band & 1) ? g.hi[m] : g.lo[m], v, gv);
        }
      }
      p.out[at] = q.guided(q.fused ? p.in[at] : 0.f, gv);
    }
  }
  // everything no tile writes: shared by all workgroups of the sample
  const int nblk = gridDim.x, w4 = p.vec ? p.W / 4 : p.W;
  const int64_t items = (int64_t)p.F * p.C * p.H * w4;
  for (int64_t idx = (int64_t)blockIdx.x * NT + tid; idx < items; idx += (int64_t)nblk * NT) {      // (64-bit: idx + the stride may pass 2^31)
    const int c4 = (int)(idx % w4);
    int r = (int)(idx / w4);
    const int row = r % p.H; r /= p.H;
    const int ch = r % p.C, fr = r / p.C;
    if (in_tiles(p, fr, ch, row)) continue;
    const float gv = succ_term(p, fr, ch, row);
    const size_t at = base + (size_t)fr * p.fs + (size_t)ch * p.cs + (size_t)row * p.rs;
    if (p.vec) {
      float4 v = q.fused ? *reinterpret_cast<const float4*>(p.in + at + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      v.x = q.guided(v.x, gv); v.y = q.guided(v.y, gv); v.z = q.guided(v.z, gv); v.w = q.guided(v.w, gv);
      *reinterpret_cast<float4*>(p.out + at + 4 * c4) = v;
    } else {
      p.out[at + c4] = q.guided(q.fused ? p.in[at + c4] : 0.f, gv);
    }
  }
}

// floats of LDS of the two launches (wdno_amd/smoke/guidance.py: lds_bytes states the same)
int64_t lds1_floats(const wdno_smoke_guidance_desc* d) {
  const int64_t KT = d->tn / 2 + 2, KH = d->hn / 2 + 2;
  return 2 * KT * KH * d->wc + 4 * KT * KH * d->wo + 2 * KT * d->hn * d->wo;
}
int64_t lds2_floats(const wdno_smoke_guidance_desc* d) {
  return 2 * (int64_t)d->kt * (2 * d->kh + 4) * d->wo + 4 * (int64_t)d->kt * d->kh * d->wo;
}

int validate(const wdno_smoke_guidance_desc* d) {
  if (!d) return WDNO_EINVAL;
  if (d->mode != 1 || d->L != L) return WDNO_EUNSUPPORTED;
  WDNO_REQUIRE(d->B > 0 && d->B <= 65535 && d->F > 0 && d->C >= 42 && d->H > 1 && d->W > 0);
  WDNO_REQUIRE(d->row_stride >= d->W && (int64_t)d->chan_stride >= (int64_t)d->H * d->row_stride &&
               (int64_t)d->frame_stride >= (int64_t)d->C * d->chan_stride && d->sample_stride >= (int64_t)d->F * d->frame_stride);
  WDNO_REQUIRE((int64_t)d->F * d->C * d->H * d->W < ((int64_t)1 << 31) && (int64_t)d->B * d->sample_stride < ((int64_t)1 << 40));
  WDNO_REQUIRE(d->tc >= 3 && d->tc <= d->F && d->hc >= 3 && d->hc <= d->H && d->wc >= 3 && d->wc <= d->W);      // a block larger than the tensor
  WDNO_REQUIRE(d->to >= 1 && d->to <= 2 * d->tc - L + 2 && d->ho >= 1 && d->ho <= 2 * d->hc - L + 2 && d->wo >= 1 && d->wo <= 2 * d->wc - L + 2);      // a crop larger than the reconstruction
  WDNO_REQUIRE(d->half >= 1 && d->half < d->H);
  WDNO_REQUIRE(d->tn >= 2 && d->hn >= 2 && !(d->tn & 1) && !(d->hn & 1) && d->tn <= 64 && d->hn <= 64 && d->kt >= 1 && d->kh >= 1 && d->kt <= 64 && d->kh <= 64);
  WDNO_REQUIRE(d->ncopy >= 1 && d->ncopy <= 4096);
  WDNO_REQUIRE(d->lds1_bytes >= 4 * lds1_floats(d) && d->lds1_bytes <= 65536 && d->lds2_bytes >= 4 * lds2_floats(d) && d->lds2_bytes <= 65536);
  return WDNO_OK;
}

}  // namespace

extern "C" size_t wdno_smoke_guidance_ws_bytes(const wdno_smoke_guidance_desc* d) {
  if (validate(d) != WDNO_OK) return 0;
  return (size_t)d->B * (2 * (size_t)d->to + 1) * d->ho * d->wo * sizeof(float);
}

extern "C" int wdno_smoke_guidance(const float* x_t, const float* in, const int64_t* t, const float* c1, const float* c2, const float* s_table,
                                   const float* rescaler, const float* init_u, const float* succ, float* out, void* ws, size_t ws_bytes,
                                   const wdno_smoke_guidance_desc* d, const float* filt, wdno_stream_t s) {
  WDNO_REQUIRE(in && rescaler && out && d && filt && in != out && x_t != out);
  const int rc = validate(d);
  if (rc) return rc;
  WDNO_REQUIRE(!x_t || (t && c1 && c2 && s_table && d->num_timesteps > 0));
  WDNO_REQUIRE(d->is_condition_control || succ);
  WDNO_REQUIRE(!d->has_init_u || init_u);
  SGuidP p;
  p.xt = x_t; p.in = in; p.out = out; p.ws = (float*)ws;
  p.t = t; p.c1 = c1; p.c2 = c2; p.s = s_table; p.resc = rescaler; p.init_u = init_u; p.succ = succ;
  p.F = d->F; p.C = d->C; p.H = d->H; p.W = d->W;
  p.ss = d->sample_stride; p.fs = d->frame_stride; p.cs = d->chan_stride; p.rs = d->row_stride;
  p.tc = d->tc; p.hc = d->hc; p.wc = d->wc; p.to = d->to; p.ho = d->ho; p.wo = d->wo;
  p.half = d->half; p.T = d->num_timesteps; p.clip = d->clip_x0 != 0; p.cc = d->is_condition_control != 0;
  p.use0 = d->has_init_u && d->w_init != 0.f;
  p.use34 = !p.cc && d->w_energy != 0.f;
  p.tn = d->tn; p.hn = d->hn; p.kt = d->kt; p.kh = d->kh;
  const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  p.vec = d->W % 4 == 0 && d->row_stride % 4 == 0 && d->chan_stride % 4 == 0 && d->frame_stride % 4 == 0 && d->sample_stride % 4 == 0 && al16(in) && al16(out);
  p.ce = (float)(2.0 * (double)d->w_energy / (2.0 * d->to * d->ho * d->wo));
  p.ci = (float)(2.0 * (double)d->w_init / ((double)d->ho * d->wo));
  STaps g;
  for (int m = 0; m < L; ++m) { g.lo[m] = filt[2 * L + m]; g.hi[m] = filt[3 * L + m]; }
  const int nrt = cdiv(d->ho, d->hn), n1 = (p.use34 ? 2 * cdiv(d->to, d->tn) * nrt : 0) + (p.use0 ? nrt : 0);
  const int nkr = cdiv(d->hc, d->kh), n2 = (p.use34 ? 2 * cdiv(d->tc, d->kt) * nkr : 0) + (p.use0 ? cdiv(reach0(d->tc), d->kt) * nkr : 0);
  if (n1 > 0) {
    WDNO_REQUIRE(ws && ws_bytes >= wdno_smoke_guidance_ws_bytes(d) && (reinterpret_cast<uintptr_t>(ws) & 3) == 0);
    smoke_guidance_synthesis_kernel<<<dim3(n1, d->B), NT, (size_t)d->lds1_bytes, as_stream(s)>>>(p, g);
  }
  smoke_guidance_adjoint_kernel<<<dim3(n2 + d->ncopy, d->B), NT, (size_t)d->lds2_bytes, as_stream(s)>>>(p, g, n2);
  return wdno_check_launch();
}
