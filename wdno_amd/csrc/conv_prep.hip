// conv_prep.hip -- operand preparation for the 16-bit convolution kernels (conv_h3.hip has the arithmetic): amax and amax records, the fp16
// (hi, lo) split and the bf16 cast of an activation with their per-channel column sums, and the weight pack + split with its multi-tensor forms.
// All HBM-bound sweeps; none of them is a matrix kernel.
#include "conv_tiles.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------- amax / split
template <bool RECORD>
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ out) {
  __shared__ float red[4];
  const int64_t n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float m = 0.f;
  // four independent 16-byte loads in flight per thread: a bandwidth-bound sweep needs ~8 MB outstanding chip-wide
  const int64_t stride = (int64_t)gridDim.x * 1024;
  for (int64_t k0 = (int64_t)blockIdx.x * 1024 + threadIdx.x; k0 < n4; k0 += stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int64_t k = k0 + u * 256;
      v[u] = k < n4 ? x4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v[u].x), fabsf(v[u].y))), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
  }
  if (blockIdx.x == 0)
    for (int64_t k = (n4 << 2) + threadIdx.x; k < n; k += 256) m = fmaxf(m, fabsf(x[k]));
  if (RECORD) {
    amax_record_emit(m, reinterpret_cast<float*>(out), blockIdx.x);
    return;
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(out, __float_as_uint(m));      // non-negative floats order like their bit patterns
  }
}
// (conv_common.h) the record sweep behind a forward whose epilogue could not fill it: conv_h3.hip's split over the tap rows
void conv_amax_record_launch(const float* x, int64_t n, float* rec, hipStream_t st) {
  amax_kernel<true><<<stream_grid(n / 16 + 1, 256), 256, 0, st>>>(x, n, reinterpret_cast<unsigned*>(rec));
}
extern "C" int wdno_amax_record(const float* x, int64_t n, float* rec_zeroed, wdno_stream_t s) {
  WDNO_REQUIRE(n >= 0);
  if (n == 0) return WDNO_OK;
  amax_kernel<true><<<stream_grid(n / 16 + 1, 256), 256, 0, as_stream(s)>>>(x, n, reinterpret_cast<unsigned*>(rec_zeroed));
  return wdno_check_launch();
}
extern "C" int wdno_amax(const float* x, int64_t n, float* amax_zeroed, wdno_stream_t s) {
  WDNO_REQUIRE(n > 0);
  amax_kernel<false><<<stream_grid(n / 16 + 1, 256), 256, 0, as_stream(s)>>>(x, n, reinterpret_cast<unsigned*>(amax_zeroed));
  return wdno_check_launch();
}

// x [rows][C] fp32 -> hi, lo [rows][C8] fp16 (zero padded), scale_out[0] = s
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ x, const float* __restrict__ amax,
                                                     _Float16* __restrict__ hi, _Float16* __restrict__ lo, float* __restrict__ scale_out,
                                                     int64_t rows, int C, int C8) {
  const bool lp = lo == nullptr;                             // single bf16 plane, no scale
  const float s = lp ? 1.0f : scale_from_amax(amax_record_read(amax));
  if (!lp && blockIdx.x == 0 && threadIdx.x == 0) scale_out[0] = s;
  const int g8 = C8 >> 3;
  const int64_t total = rows * g8;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    int64_t r = i / g8;
    int c0 = (int)(i - r * g8) * 8;
    float v[8];
    const float* xp = x + r * C + c0;
    if (c0 + 8 <= C) {
      float4 a = *reinterpret_cast<const float4*>(xp), b = *reinterpret_cast<const float4*>(xp + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (c0 + e < C) ? xp[e] : 0.f;
    }
    if (lp) {
      typedef unsigned short us8 __attribute__((ext_vector_type(8)));
      us8 b;
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = bf16_rne(v[e]);
      *reinterpret_cast<us8*>(hi + r * C8 + c0) = b;
      continue;
    }
    half8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = v[e] * s;
      _Float16 th = (_Float16)t;
      h[e] = th;
      l[e] = (_Float16)(t - (float)th);
    }
    *reinterpret_cast<half8*>(hi + r * C8 + c0) = h;
    *reinterpret_cast<half8*>(lo + r * C8 + c0) = l;
  }
}
extern "C" int wdno_cast_bf16(const float* x, void* out, int64_t rows, int C, int C8, wdno_stream_t s) {
  WDNO_REQUIRE(rows > 0 && C > 0 && (C & 3) == 0 && (C8 & 7) == 0 && C8 >= C && C8 < C + 16);      // (up to a whole 16-channel block: 7-wide stems)
  int64_t total = rows * (C8 / 8);
  split_kernel<<<stream_grid(total, 256), 256, 0, as_stream(s)>>>(x, nullptr, (_Float16*)out, nullptr, nullptr, rows, C, C8);
  return wdno_check_launch();
}
extern "C" int wdno_split_f16(const float* x, const float* amax, void* hi, void* lo, float* scale_out, int64_t rows, int C, int C8,
                              wdno_stream_t s) {
  WDNO_REQUIRE(rows > 0 && C > 0 && (C & 3) == 0 && (C8 & 7) == 0 && C8 >= C && C8 < C + 16);      // (up to a whole 16-channel block: 7-wide stems)
  int64_t total = rows * (C8 / 8);
  split_kernel<<<stream_grid(total, 256), 256, 0, as_stream(s)>>>(x, amax, (_Float16*)hi, (_Float16*)lo, scale_out, rows, C, C8);
  return wdno_check_launch();
}

// split + per-channel column sums in one pass (the bias gradient of a convolution is the column sum of the same dy that is
// being split for the data / weight gradient kernels). Every thread always works on the same 8-channel group (the host
// only calls this for power-of-two group counts <= 256), accumulates its rows in fp32 and the block folds them to one
// double row of partials; partial_rows_sum_kernel<double> finishes, as for wdno_colsum.
__global__ __launch_bounds__(256) void split_colsum_kernel(const float* __restrict__ x, const float* __restrict__ amax,
                                                            _Float16* __restrict__ hi, _Float16* __restrict__ lo, float* __restrict__ scale_out,
                                                            double* __restrict__ part, int64_t rows, int C, int C8) {
  __shared__ float red[256][9];
  const bool lp = lo == nullptr;
  const float s = lp ? 1.0f : scale_from_amax(amax_record_read(amax));
  if (!lp && blockIdx.x == 0 && threadIdx.x == 0) scale_out[0] = s;
  const int g8 = C8 >> 3;
  const int64_t total = rows * g8;
  const int64_t stride = (int64_t)gridDim.x * 256;            // a multiple of g8: the channel group of a thread never changes
  float cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    int64_t r = i / g8;
    int c0 = (int)(i - r * g8) * 8;
    float v[8];
    const float* xp = x + r * C + c0;
    if (c0 + 8 <= C) {
      float4 a = *reinterpret_cast<const float4*>(xp), b = *reinterpret_cast<const float4*>(xp + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (c0 + e < C) ? xp[e] : 0.f;
    }
    if (lp) {
      typedef unsigned short us8 __attribute__((ext_vector_type(8)));
      us8 b;
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs[e] += v[e]; b[e] = bf16_rne(v[e]); }
      *reinterpret_cast<us8*>(hi + r * C8 + c0) = b;
      continue;
    }
    half8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      cs[e] += v[e];
      float t = v[e] * s;
      _Float16 th = (_Float16)t;
      h[e] = th;
      l[e] = (_Float16)(t - (float)th);
    }
    *reinterpret_cast<half8*>(hi + r * C8 + c0) = h;
    *reinterpret_cast<half8*>(lo + r * C8 + c0) = l;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = cs[e];
  __syncthreads();
  // threads t, t + g8, t + 2 g8, ... share the group t % g8
  for (int idx = threadIdx.x; idx < C8; idx += 256) {
    const int grp = idx >> 3, e = idx & 7;
    double acc = 0.0;
    for (int t = grp; t < 256; t += g8) acc += (double)red[t][e];
    part[(int64_t)blockIdx.x * C8 + idx] = acc;
  }
}
// ws: doubles [wdno_split_colsum_ws_bytes / 8]; colsum_out[C8] fp32. WDNO_EUNSUPPORTED unless C8/8 is a power of two <= 256.
extern "C" size_t wdno_split_colsum_ws_bytes(int64_t rows, int C8) {
  return (size_t)stream_grid(rows * (C8 / 8), 256) * (size_t)C8 * sizeof(double);
}
extern "C" int wdno_split_f16_colsum(const float* x, const float* amax, void* hi, void* lo, float* scale_out, float* colsum_out,
                                     void* ws, size_t ws_bytes, int64_t rows, int C, int C8, wdno_stream_t s) {
  WDNO_REQUIRE(rows > 0 && C > 0 && (C & 3) == 0 && (C8 & 7) == 0 && C8 >= C && C8 < C + 16);      // (up to a whole 16-channel block: 7-wide stems)
  const int g8 = C8 / 8;
  if (g8 > 256 || (g8 & (g8 - 1))) return WDNO_EUNSUPPORTED;
  if (ws_bytes < wdno_split_colsum_ws_bytes(rows, C8)) return WDNO_EWORKSPACE;
  const int grid = stream_grid(rows * g8, 256);
  split_colsum_kernel<<<grid, 256, 0, as_stream(s)>>>(x, amax, (_Float16*)hi, (_Float16*)lo, scale_out, (double*)ws, rows, C, C8);
  if (colsum_out)      // NULL: the caller sums the ws_bytes / (8 C8) rows of partials later (wdno_rows_sum_multi)
    partial_rows_sum_kernel<double><<<cdiv(C8, 32), PRS_THREADS, 0, as_stream(s)>>>((const double*)ws, colsum_out, grid, C8);
  return wdno_check_launch();
}

extern "C" int wdno_cast_bf16_colsum(const float* x, void* out, float* colsum_out, void* ws, size_t ws_bytes, int64_t rows, int C, int C8,
                                     wdno_stream_t s) {
  WDNO_REQUIRE(rows > 0 && C > 0 && (C & 3) == 0 && (C8 & 7) == 0 && C8 >= C && C8 < C + 16);      // (up to a whole 16-channel block: 7-wide stems)
  const int g8 = C8 / 8;
  if (g8 > 256 || (g8 & (g8 - 1))) return WDNO_EUNSUPPORTED;
  if (ws_bytes < wdno_split_colsum_ws_bytes(rows, C8)) return WDNO_EWORKSPACE;
  const int grid = stream_grid(rows * g8, 256);
  split_colsum_kernel<<<grid, 256, 0, as_stream(s)>>>(x, nullptr, (_Float16*)out, nullptr, nullptr, (double*)ws, rows, C, C8);
  if (colsum_out)
    partial_rows_sum_kernel<double><<<cdiv(C8, 32), PRS_THREADS, 0, as_stream(s)>>>((const double*)ws, colsum_out, grid, C8);
  return wdno_check_launch();
}

// ---------------------------------------------------------------------------------------------- weight pack + split
// raw weight w[K][C][kd][kh][kw] fp32  ->  fp16 planes of the packed operand, in one launch:
//   mode 0 (forward)  : out[dz][dy][a=k < A][dx][b=c < B]  = w[k][c][dz][dy][dx]
//   mode 1 (data grad): out[dz][dy][a=c < A][dx][b=k < B]  = w[k][c][kd-1-dz][kh-1-dy][kw-1-dx]
// A / B are the padded extents of the two channel roles (B % 8 == 0); entries outside K / C are zero.
// Tiled through LDS (round 2). The source element of output (tap, a, b) is w[(k*C + c)*T + tap] with (k, c) = (a, b) for the forward
// operand and (b, a), flipped taps, for the data-gradient operand: in w a run of c at fixed k is contiguous ([c][tap]), in the output a
// run of b is. A block moves a tile of KT k's x CT c's x all T taps: it reads KT contiguous runs of CT*T floats (coalesced 16-byte
// loads) into LDS and writes, per (tap, a), the tile's run of b as 8-element groups (16 B per plane per thread, contiguous across
// threads). The tile is long in the direction the output wants contiguous: forward 8 k x 128 c, data gradient 128 k x 8 c (scaled
// down so that the tile stays under PS_LDS_FLOATS for many taps). The first version ran one grid-stride loop over the output index
// with 4-byte reads T floats apart: every line of w was fetched once per tap and 9x over-fetched per access -- 3.1 ms per step for
// the 563 MB of Burgers weights (8.9 % of its batch-16 training step).
#define PS_LDS_FLOATS 10240
struct PackTile { int KT, CT, CTp, tiles_k, tiles_c; };
__host__ __device__ static inline PackTile pack_tile(int T, int A, int B, int mode) {
  PackTile t;
  // floats of the LDS tile [tap][KT][CT + 1]
  auto need = [&](int longd, int shortd) { return (int64_t)T * (mode ? (int64_t)longd * (shortd + 1) : (int64_t)shortd * (longd + 1)); };
  int longd = 128, shortd = 8;
  while (longd > 8 && need(longd, shortd) > PS_LDS_FLOATS) longd >>= 1;
  while (shortd > 1 && need(longd, shortd) > PS_LDS_FLOATS) shortd >>= 1;
  t.KT = mode ? longd : shortd;          // data gradient: b = k is the contiguous output index
  t.CT = mode ? shortd : longd;
  t.CTp = t.CT + 1;                      // LDS tile [tap][k][c] with an odd c pitch
  const int kext = mode ? B : A, cext = mode ? A : B;      // padded extents of k and c in the output
  t.tiles_k = (kext + t.KT - 1) / t.KT;
  t.tiles_c = (cext + t.CT - 1) / t.CT;
  return t;
}
// n / d for n * d < 2^32 with m = 2^32 / d + 1 (d > 1). Own copy of fastdiv.h's helper: on FastDiv both weight-pack kernels gain nine scalar instructions
__device__ __forceinline__ unsigned ps_magic(unsigned d) { return d > 1 ? (unsigned)((1ull << 32) / d) + 1u : 0u; }
__device__ __forceinline__ int ps_div(int n, int d, unsigned m) { return d == 1 ? n : (int)__umulhi((unsigned)n, m); }
__device__ __forceinline__ void pack_split_body(const float* __restrict__ w, const float* __restrict__ amax,
                                                _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                float* __restrict__ scale_out, int K, int C, int kd, int kh, int kw,
                                                int A, int B, int mode_in, int block, int nblocks) {
  __shared__ float tile[PS_LDS_FLOATS + 16];
  // modes 2 .. 5: forward operand of parity class (py, px) = ((mode - 2) >> 1, (mode - 2) & 1) of the (1,4,4) / stride (1,2,2) transposed
  // convolution, read straight from its weight w[in = C][out = K][1][4][4]:  W[k][c][0][dy][dx] = w[c][k][0][3 - py - 2 dy][3 - px - 2 dx]
  // (kd, kh, kw = 1, 2, 2). Only the gather below differs; everything after it is the forward layout.
  // modes 6 .. 9: data-gradient operand of tap (py, px) = ((mode - 6) >> 1, (mode - 6) & 1) of a (1,2,2) / stride (1,2,2) convolution (the folded
  // Downsample of the Burgers U-Net, unet.py:64-68), whose data gradient is four 1 x 1 convolutions of dy scattered to the four pixel parities:
  // out[a = c][b = k] = w[k][c][0][py][px]  (told kd, kh, kw = 1, 1, 1; data-gradient layout, only the gather differs)
  // modes 10 / 11: the forward operand of a 1 x 1 projection in the FRAGMENT order of csrc/attn_fused_wide.hip (to_qkv [384][C] / to_out [C][128] of
  // a temporal attention block): the 16-byte group (row a, channels 8 bg ..) moves so that the 64 lanes of one matrix-operand load read 1 KB
  //   10: a = ti 128 + h 32 + li, bg = 4 t + 2 hh + s  ->  ((((h 3 + ti) B/32 + t) 2 + s) 64 + hh 32 + li
  //   11: a = wv A/4 + mt 32 + li, bg = 4 t + 2 hh + s ->  ((((wv A/128 + mt) 4 + t) 2 + s) 64 + hh 32 + li
  const int frag = mode_in >= 10 ? mode_in - 9 : 0;
  const int parity = mode_in >= 2 && mode_in < 6 ? mode_in - 2 : -1;
  const int patch = mode_in >= 6 && mode_in < 10 ? mode_in - 6 : -1;
  const int mode = mode_in == 1 || patch >= 0 ? 1 : 0;
  const bool lp = lo == nullptr;                     // one bf16 plane, no scale (amax / scale_out may be NULL)
  const float s = lp ? 1.0f : scale_from_amax(amax[0]);
  if (!lp && block == 0 && threadIdx.x == 0) scale_out[0] = s;
  const int b8 = B >> 3;
  const int T = kd * kh * kw, khw = kh * kw;
  const PackTile pt = pack_tile(T, A, B, mode);
  if ((int64_t)T * pt.KT * pt.CTp > PS_LDS_FLOATS + 16) return;         // > ~600 taps: not a convolution of this code base
  const int ntiles = pt.tiles_k * pt.tiles_c;
  const int run = pt.CT * T;                         // floats per k row of the tile (contiguous in w)
  const int bt8 = (mode ? pt.KT : pt.CT) >> 3;       // 8-element output groups per (tap, a) inside the tile (>= 1: long dims are multiples of 8)
  const int at = mode ? pt.CT : pt.KT;               // values of a inside the tile
  const unsigned m_run = ps_magic(run), m_T = ps_magic(T), m_bt8 = ps_magic(bt8), m_at = ps_magic(at), m_khw = ps_magic(khw), m_kw = ps_magic(kw);
  for (int tl = block; tl < ntiles; tl += nblocks) {
    const int tk = ps_div(tl, pt.tiles_c, ps_magic(pt.tiles_c)), tc = tl - tk * pt.tiles_c;
    const int k0 = tk * pt.KT, c0 = tc * pt.CT;
    __syncthreads();
    // load: row kk of the tile = w[(k0 + kk)*C*T + c0*T ...], `run` contiguous floats ([c][tap]); zero where k >= K or c >= C
    const int cvalid = min(pt.CT, C - c0);           // may be <= 0 for padding tiles
    // eight loads per thread in flight (one at a time, behind a branch, the 36 loads of a thread per 8 x 128 x 9 tile were a chain of
    // round trips: 1.17 ms per step for the 563 MB of Burgers weights = 1.45 TB/s over read + write)
    const int nload = pt.KT * run;
    for (int idx0 = threadIdx.x; idx0 < nload; idx0 += 256 * 8) {
      float v[8];
      int dst[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = min(idx0 + 256 * u, nload - 1);
        const int kk = ps_div(idx, run, m_run), r = idx - kk * run;
        const int cl = ps_div(r, T, m_T), tap = r - cl * T;
        const bool ok = k0 + kk < K && cl < cvalid;
        const int64_t off = !ok ? 0 : patch >= 0 ? (((int64_t)(k0 + kk) * C + c0 + cl) * 4 + patch) : parity < 0 ? ((int64_t)(k0 + kk) * C + c0) * T + r
                            : ((int64_t)(c0 + cl) * K + (k0 + kk)) * 16 + (3 - (parity >> 1) - 2 * (tap >> 1)) * 4 + (3 - (parity & 1) - 2 * (tap & 1));
        v[u] = w[off];
        if (!ok) v[u] = 0.f;
        dst[u] = idx0 + 256 * u < nload ? (tap * pt.KT + kk) * pt.CTp + cl : -1;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (dst[u] >= 0) tile[dst[u]] = v[u];
    }
    __syncthreads();
    // store: items (tap, a_local, group of 8 b's), the group index fastest: 16 contiguous bytes per plane per thread
    const int nitems = T * at * bt8;
    for (int idx = threadIdx.x; idx < nitems; idx += 256) {
      int q = ps_div(idx, bt8, m_bt8);
      const int g = idx - q * bt8;
      const int tap = ps_div(q, at, m_at), al = q - tap * at;
      const int dz = ps_div(tap, khw, m_khw), rr = tap - dz * khw;
      const int dy = ps_div(rr, kw, m_kw), dx = rr - dy * kw;
      const int ts = mode ? T - 1 - tap : tap;       // all three axes flipped = the reversed linear tap index
      const int a = (mode ? c0 : k0) + al;
      const int bg = ((mode ? k0 : c0) >> 3) + g;    // 8-element group index along b
      if (a >= A || bg >= b8) continue;
      const float* src = mode ? tile + (ts * pt.KT + g * 8) * pt.CTp + al : tile + (ts * pt.KT + al) * pt.CTp + g * 8;
      const int step = mode ? pt.CTp : 1;
      half8 h, l;
      typedef unsigned short us8 __attribute__((ext_vector_type(8)));
      us8 bq;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = src[e * step];
        const float tv = v * s;
        const _Float16 th = (_Float16)tv;
        h[e] = th;
        l[e] = (_Float16)(tv - (float)th);
        bq[e] = bf16_rne(v);
      }
      int64_t i = ((((int64_t)dz * kh + dy) * A + a) * kw + dx) * b8 + bg;
      if (frag) {
        const int li = a & 31, t = bg >> 2, hh2 = (bg >> 1) & 1, s2 = bg & 1;
        if (frag == 1) { const int ti = a >> 7, hd = (a >> 5) & 3; i = ((((hd * 3 + ti) * (B >> 5) + t) * 2 + s2) * 64 + hh2 * 32 + li); }
        else { const int q4 = A >> 2, wv = a / q4, mt = (a - wv * q4) >> 5; i = ((((wv * (A >> 7) + mt) * 4 + t) * 2 + s2) * 64 + hh2 * 32 + li); }
      }
      if (lp) { *reinterpret_cast<us8*>(hi + i * 8) = bq; continue; }
      *reinterpret_cast<half8*>(hi + i * 8) = h;
      *reinterpret_cast<half8*>(lo + i * 8) = l;
    }
  }
}
__global__ __launch_bounds__(256) void pack_split_weight_kernel(const float* __restrict__ w, const float* __restrict__ amax,
                                                                 _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                                 float* __restrict__ scale_out, int K, int C, int kd, int kh, int kw,
                                                                 int A, int B, int mode) {
  pack_split_body(w, amax, hi, lo, scale_out, K, C, kd, kh, kw, A, B, mode, (int)blockIdx.x, (int)gridDim.x);
}
// Multi-tensor forms: after an optimiser step EVERY weight needs a fresh amax and fresh packed planes; with ~100 (smoke) to
// ~300 (Burgers) operands that is hundreds of 5-microsecond launches. One launch each, grid = (blocks per item, items), the
// per-item arguments come from a device-resident table (wdno_amax_item / wdno_wsplit_item in wdno_hip.h).
__global__ __launch_bounds__(256) void amax_multi_kernel(const wdno_amax_item* __restrict__ tab) {
  __shared__ float red[4];
  const wdno_amax_item it = tab[blockIdx.y];
  const float* x = (const float*)it.x;
  const int64_t n = it.n;
  float m = 0.f;
  // weights sit at 4-byte-aligned offsets of the flat parameter buffer: up to three leading and trailing elements by block 0, the 16-byte-aligned
  // body as float4 with four loads in flight (4-byte loads: 180 us for the 563 MB of Burgers weights = 3.1 TB/s)
  int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int64_t n4 = (n - head) >> 2, tail0 = head + 4 * n4;
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < head) m = fabsf(x[threadIdx.x]);
    if (tail0 + (int64_t)threadIdx.x < n) m = fmaxf(m, fabsf(x[tail0 + threadIdx.x]));
  }
  const float4* x4 = reinterpret_cast<const float4*>(x + head);
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; k + 3 * stride < n4; k += 4 * stride) {
    const float4 a = x4[k], b = x4[k + stride], c = x4[k + 2 * stride], d = x4[k + 3 * stride];
    m = amax4(amax4(m, a), b);
    m = amax4(amax4(m, c), d);
  }
  for (; k < n4; k += stride) m = amax4(m, x4[k]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.f) atomicMax((unsigned*)it.out, __float_as_uint(m));
  }
}
extern "C" int wdno_amax_multi(const void* table, int n_items, int blocks_per_item, wdno_stream_t s) {
  WDNO_REQUIRE(table && n_items > 0 && n_items <= 65535 && blocks_per_item > 0);
  amax_multi_kernel<<<dim3((unsigned)blocks_per_item, (unsigned)n_items), 256, 0, as_stream(s)>>>((const wdno_amax_item*)table);
  return wdno_check_launch();
}
__global__ __launch_bounds__(256) void pack_split_weight_multi_kernel(const wdno_wsplit_item* __restrict__ tab) {
  const wdno_wsplit_item it = tab[blockIdx.y];
  pack_split_body((const float*)it.w, (const float*)it.amax, (_Float16*)it.hi, (_Float16*)it.lo, (float*)it.scale_out, it.K, it.C, it.kd, it.kh,
                  it.kw, it.A, it.B, it.mode, (int)blockIdx.x, (int)gridDim.x);
}
extern "C" int wdno_pack_split_weight_multi(const void* table, int n_items, int blocks_per_item, wdno_stream_t s) {
  WDNO_REQUIRE(table && n_items > 0 && n_items <= 65535 && blocks_per_item > 0);
  pack_split_weight_multi_kernel<<<dim3((unsigned)blocks_per_item, (unsigned)n_items), 256, 0, as_stream(s)>>>((const wdno_wsplit_item*)table);
  return wdno_check_launch();
}
extern "C" int wdno_pack_split_weight(const float* w, const float* amax, void* hi, void* lo, float* scale_out, int K, int C, int kd, int kh,
                                      int kw, int A, int B, int mode, wdno_stream_t s) {
  WDNO_REQUIRE(K > 0 && C > 0 && kd > 0 && kh > 0 && kw > 0 && A > 0 && B > 0 && (B & 7) == 0 && mode >= 0 && mode <= 11);
  WDNO_REQUIRE(mode < 2 || mode > 5 || (kd == 1 && kh == 2 && kw == 2));      // parity classes of the (1,4,4) transposed convolution
  WDNO_REQUIRE(mode < 6 || (kd == 1 && kh == 1 && kw == 1));                  // taps of the (1,2,2) / stride 2 convolution
  WDNO_REQUIRE(mode != 1 && (mode < 6 || mode >= 10) ? (A >= K && B >= C) : (A >= C && B >= K));
  WDNO_REQUIRE(mode != 10 || (A == 384 && (B & 31) == 0 && lo != nullptr));      // fragment order: to_qkv of 4 heads of 32, to_out onto C = 128 m channels
  WDNO_REQUIRE(mode != 11 || (B == 128 && (A & 127) == 0 && lo != nullptr));
  WDNO_REQUIRE(lo == nullptr || (amax != nullptr && scale_out != nullptr));      // lo == NULL: one bf16 plane in `hi`
  int64_t total = (int64_t)kd * kh * A * kw * (B / 8);
  const PackTile ptile = pack_tile(kd * kh * kw, A, B, mode == 1 || (mode >= 6 && mode < 10) ? 1 : 0);
  if ((int64_t)kd * kh * kw * ptile.KT * ptile.CTp > PS_LDS_FLOATS + 16) return WDNO_EUNSUPPORTED;      // > 640 taps (every operand passes here first)
  (void)total;
  pack_split_weight_kernel<<<std::min(2048, ptile.tiles_k * ptile.tiles_c), 256, 0, as_stream(s)>>>(w, amax, (_Float16*)hi, (_Float16*)lo, scale_out, K, C, kd, kh, kw,
                                                                            A, B, mode);
  return wdno_check_launch();
}
