// linattn.hip -- linear attention of the two U-Nets (head dim fixed at 32, as in the reference): softmax over the 32 head channels for q,
// over all tokens for k. The 32x32 context k^T v is a genuine dense contraction over thousands of tokens -> v_mfma_f32_32x32x2_f32, streamed
// from global memory (each lane supplies one k and one v element per MFMA); the per-token 32x32 mat-vecs run on the same matrix instruction
// over tiles staged through LDS (attn_tiles.h), or on the vector ALU with the context broadcast from LDS (the thread-per-token kernels).
#include "attn_tiles.h"
#include "debug_modes.h"

#define KST 33
// ================================================================================================ linear attention
// pass 1: per (unit, column = head*32+d): max over tokens and sum of exp -> kstats[unit][col][2].
// A unit has up to 1600 tokens but there are only ~200 units: the token range is cut into `chunks` pieces (one block each,
// online-softmax partials into a scratch area) and a second tiny launch merges them, so the sweep fills the chip.
__device__ __forceinline__ void softmax_merge(float& m, float& l, float m2, float l2) {
  float mn = fmaxf(m, m2);
  float a = (m == -INFINITY) ? 0.f : l * expf(m - mn);
  float b = (m2 == -INFINITY) ? 0.f : l2 * expf(m2 - mn);
  l = a + b; m = mn;
}
__global__ __launch_bounds__(256) void linattn_kstats_kernel(const float* __restrict__ qkv, float* __restrict__ part, int n, int HD, int chunks) {
  __shared__ float rm[256], rl[256];
  const int unit = blockIdx.x / chunks, chunk = blockIdx.x - unit * chunks;
  const int per = (n + chunks - 1) / chunks;
  const int jb = chunk * per, je = min(n, jb + per);
  const int col = threadIdx.x % HD, rg = threadIdx.x / HD, nrg = 256 / HD;
  const float* kp = qkv + ((int64_t)unit * n) * (3 * HD) + HD + col;
  float m = -INFINITY, l = 0.f;
  // eight rows per round: the loads are requested together and the running sum is rescaled once per round (row by row the
  // online softmax is a chain of load -> exp -> exp with one 512-byte request in flight per wave)
  for (int j = jb + rg; j < je; j += 8 * nrg) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = j + u * nrg < je ? kp[(int64_t)(j + u * nrg) * 3 * HD] : -INFINITY;
    float mn = m;
#pragma unroll
    for (int u = 0; u < 8; ++u) mn = fmaxf(mn, v[u]);
    float add = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) add += expf(v[u] - mn);        // exp(-inf) = 0 for the rows past the end
    l = (m == -INFINITY ? 0.f : l * expf(m - mn)) + add;
    m = mn;
  }
  rm[threadIdx.x] = m; rl[threadIdx.x] = l;
  __syncthreads();
  if (rg == 0) {
    for (int t = 1; t < nrg; ++t) softmax_merge(m, l, rm[t * HD + col], rl[t * HD + col]);
    part[((int64_t)blockIdx.x * HD + col) * 2 + 0] = m;
    part[((int64_t)blockIdx.x * HD + col) * 2 + 1] = l;
  }
}
__global__ __launch_bounds__(256) void linattn_kstats_merge_kernel(const float* __restrict__ part, float* __restrict__ kstats, int64_t cols, int HD, int chunks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (unit, col)
  if (i >= cols) return;
  const int64_t unit = i / HD;
  const int col = (int)(i - unit * HD);
  float m = -INFINITY, l = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float* q = part + (((unit * chunks + c) * HD) + col) * 2;
    softmax_merge(m, l, q[0], q[1]);
  }
  kstats[i * 2] = m;
  kstats[i * 2 + 1] = l;
}

// pass 2 (MODE 0): ctx[d][e]  = sum_n softmax_n(k)[n][d] * v[n][e]        A = exp(k - m)/l, B = v
//        (MODE 1): dctx[d][e] = sum_n qs[n][d] * dout[n][e]                A = scale*softmax_d(q), B = dout ; also T[d]
// one block (4 waves) per (unit, head); every MFMA consumes two tokens.
template <int MODE>
__global__ __launch_bounds__(256) void linattn_ctx_kernel(const float* __restrict__ qkv, const float* __restrict__ other,
                                                           const float* __restrict__ kstats, const float* __restrict__ ctx_in,
                                                           float* __restrict__ ctx_out, float* __restrict__ tvec,
                                                           int n, int heads, float scale, int chunks = 1, float* __restrict__ part = nullptr) {
  // chunks > 1 (few (unit, head) pairs, many tokens: the Burgers U-Net has 16 x 4 of them over 4096 tokens -- 64 blocks on 256 CUs): the
  // token range is cut into `chunks` pieces, one block each, partial sums go to part[block][32][32] and linattn_ctx_merge_kernel adds them
  __shared__ float red[4][DH][KST];
  const int HD = heads * DH, RW = 3 * HD;
  const int uh = blockIdx.x / chunks, chunk = blockIdx.x - uh * chunks;
  const int unit = uh / heads, h = uh - unit * heads;
  const int clen = ((n + chunks - 1) / chunks + 7) & ~7;
  const int t0 = chunk * clen, t1 = min(n, t0 + clen);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, dd = lane & 31, hh = lane >> 5;
  float km = 0.f, kinvl = 1.f;
  if (MODE == 0) {
    km = kstats[((int64_t)unit * HD + h * DH + dd) * 2 + 0];
    kinvl = 1.0f / kstats[((int64_t)unit * HD + h * DH + dd) * 2 + 1];
  }
  f32x16 acc = tf_zero();
  const float* base = qkv + ((int64_t)unit * n) * RW + h * DH + dd;
  const float* ob = MODE == 1 ? other + ((int64_t)unit * n) * HD + h * DH + dd : nullptr;
  // eight token pairs per round: all sixteen row loads of a round are requested before the first is used (one pair per
  // iteration leaves a single 256-byte request in flight per wave and the kernel at ~1.5 TB/s)
  constexpr int UN = 8;
  for (int j0 = t0 + wave * 2; j0 < t1; j0 += 8 * UN) {
    float ra[UN], rb[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = j0 + 8 * u + hh;
      const bool ok = j < t1;
      if (MODE == 0) {
        ra[u] = ok ? base[(int64_t)j * RW + HD] : 0.f;
        rb[u] = ok ? base[(int64_t)j * RW + 2 * HD] : 0.f;
      } else {
        ra[u] = ok ? base[(int64_t)j * RW] : 0.f;
        rb[u] = ok ? ob[(int64_t)j * HD] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const bool ok = j0 + 8 * u + hh < t1;
      float a;
      if (MODE == 0) {
        a = ok ? expf(ra[u] - km) * kinvl : 0.f;
      } else {
        float mx = group_max<32>(ra[u]);
        float ex = expf(ra[u] - mx);
        float sm = group_sum<32>(ex);
        a = ok ? scale * ex / sm : 0.f;
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, rb[u], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) red[wave][(e & 3) + 8 * (e >> 2) + 4 * hh][dd] = acc[e];
  __syncthreads();
  // 1024 outputs / 256 threads
  if (chunks > 1) {
    float* po = part + (int64_t)blockIdx.x * DH * DH;
    for (int o = threadIdx.x; o < DH * DH; o += 256) {
      int r = o >> 5, c = o & 31;
      po[o] = (red[0][r][c] + red[1][r][c]) + (red[2][r][c] + red[3][r][c]);
    }
    return;
  }
  float* co = ctx_out + ((int64_t)unit * heads + h) * DH * DH;
  const float* ci = MODE == 1 ? ctx_in + ((int64_t)unit * heads + h) * DH * DH : nullptr;
  for (int o = threadIdx.x; o < DH * DH; o += 256) {
    int r = o >> 5, c = o & 31;
    float v = (red[0][r][c] + red[1][r][c]) + (red[2][r][c] + red[3][r][c]);
    co[o] = v;
    if (MODE == 1) red[0][r][c] = v * ci[o];   // each (r,c) is owned by exactly one thread
  }
  if (MODE == 1) {
    __syncthreads();
    if (threadIdx.x < DH) {
      float t = 0.f;
      for (int c = 0; c < DH; ++c) t += red[0][threadIdx.x][c];
      tvec[((int64_t)unit * heads + h) * DH + threadIdx.x] = t;
    }
  }
}

// sum of the chunk partials of linattn_ctx_kernel in chunk order; MODE 1 also T[d] = sum_e dctx[d][e] ctx[d][e]
template <int MODE>
__global__ __launch_bounds__(256) void linattn_ctx_merge_kernel(const float* __restrict__ part, const float* __restrict__ ctx_in,
                                                                 float* __restrict__ ctx_out, float* __restrict__ tvec, int chunks) {
  __shared__ float red[DH][KST];
  const int64_t uh = blockIdx.x;
  const float* p0 = part + uh * chunks * DH * DH;
  float* co = ctx_out + uh * DH * DH;
  const float* ci = MODE == 1 ? ctx_in + uh * DH * DH : nullptr;
  for (int o = threadIdx.x; o < DH * DH; o += 256) {
    float v = 0.f;
    for (int c = 0; c < chunks; ++c) v += p0[c * DH * DH + o];
    co[o] = v;
    if (MODE == 1) red[o >> 5][o & 31] = v * ci[o];
  }
  if (MODE == 1) {
    __syncthreads();
    if (threadIdx.x < DH) {
      float t = 0.f;
      for (int c = 0; c < DH; ++c) t += red[threadIdx.x][c];
      tvec[uh * DH + threadIdx.x] = t;
    }
  }
}
// pieces of the token range per (unit, head): enough blocks for ~2 per CU, at least 128 tokens each, at most LA_MAXCHUNKS
#define LA_MAXCHUNKS 16
static int la_ctx_chunks(int64_t units, int heads, int n_tok) {
  const int64_t uh = units * heads;
  int64_t c = (2 * (int64_t)wdno_num_cus() + uh - 1) / uh;
  if (c > n_tok / 128) c = n_tok / 128;
  if (c > LA_MAXCHUNKS) c = LA_MAXCHUNKS;
  if (c < 1) c = 1;
  return (int)c;
}
template <int MODE>
static void la_ctx_launch(const float* qkv, const float* other, const float* kstats, const float* ctx_in, float* ctx_out, float* tvec, float* part,
                          int64_t units, int n_tok, int heads, float scale, int chunks, hipStream_t st) {
  if (!part) chunks = 1;
  linattn_ctx_kernel<MODE><<<(unsigned)(units * heads * chunks), 256, 0, st>>>(qkv, other, kstats, ctx_in, ctx_out, tvec, n_tok, heads, scale, chunks, part);
  if (chunks > 1) linattn_ctx_merge_kernel<MODE><<<(unsigned)(units * heads), 256, 0, st>>>(part, ctx_in, ctx_out, tvec, chunks);
}

// pass 3: out[n][e] = scale * sum_d ctx[d][e] * softmax_d(q[n])[d]; one thread per (token, head)
__global__ __launch_bounds__(256) void linattn_out_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx, float* __restrict__ out,
                                   int n, int heads, float scale, float* __restrict__ amax_rec) {
  extern __shared__ __attribute__((aligned(16))) float cs[];   // [heads][32][32]
  const int HD = heads * DH, RW = 3 * HD;
  const int unit = blockIdx.x;
  const int h = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < heads * DH * DH; e += blockDim.x) cs[e] = ctx[(int64_t)unit * heads * DH * DH + e];
  __syncthreads();
  const int jt = blockIdx.y * 64 + (threadIdx.x & 63);
  const bool ok = jt < n;
  const int j = ok ? jt : n - 1;           // lanes past the last token redo it (all lanes stay active for the amax reduction) and store nothing
  const float4* qp = reinterpret_cast<const float4*>(qkv + ((int64_t)unit * n + j) * RW + h * DH);
  float q[DH];
#pragma unroll
  for (int e = 0; e < 8; ++e) { float4 v = qp[e]; q[4 * e] = v.x; q[4 * e + 1] = v.y; q[4 * e + 2] = v.z; q[4 * e + 3] = v.w; }
  float mx = q[0];
#pragma unroll
  for (int e = 1; e < DH; ++e) mx = fmaxf(mx, q[e]);
  float sm = 0.f;
#pragma unroll
  for (int e = 0; e < DH; ++e) { q[e] = expf(q[e] - mx); sm += q[e]; }
  float f = scale / sm;
  float o[DH];
#pragma unroll
  for (int e = 0; e < DH; ++e) o[e] = 0.f;
  const float4* cp = reinterpret_cast<const float4*>(cs + h * DH * DH);
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    float w = q[d] * f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float4 c = cp[d * 8 + e];
      o[4 * e] = fmaf(w, c.x, o[4 * e]); o[4 * e + 1] = fmaf(w, c.y, o[4 * e + 1]);
      o[4 * e + 2] = fmaf(w, c.z, o[4 * e + 2]); o[4 * e + 3] = fmaf(w, c.w, o[4 * e + 3]);
    }
  }
  float4* op = reinterpret_cast<float4*>(out + ((int64_t)unit * n + j) * HD + h * DH);
  float am = 0.f;
  if (ok) {
#pragma unroll
  for (int e = 0; e < 8; ++e) op[e] = make_float4(o[4 * e], o[4 * e + 1], o[4 * e + 2], o[4 * e + 3]);
  }
#pragma unroll
  for (int e = 0; e < DH; ++e) am = fmaxf(am, fabsf(o[e]));
  if (amax_rec) wave_amax_emit(am, amax_rec, (int)((blockIdx.y * gridDim.x + blockIdx.x) * heads + h));
}

// backward pass B2: one thread per (token, head):
//   dq = scale * qsm * (dqs - <qsm, dqs>),  dqs[d] = sum_e dout[e] ctx[d][e]
//   dv[e] = sum_d ks[d] dctx[d][e] ; dk[d] = ks[d] * (sum_e v[e] dctx[d][e] - T[d])
__global__ __launch_bounds__(256) void linattn_bwd_tok_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ kstats,
                                       const float* __restrict__ ctx, const float* __restrict__ dctx, const float* __restrict__ tvec,
                                       float* __restrict__ dqkv, int n, int heads, float scale, float* __restrict__ amax_rec) {
  extern __shared__ __attribute__((aligned(16))) float sm_[];
  const int HD = heads * DH, RW = 3 * HD;
  float* cs = sm_;                       // [heads][32][32]
  float* ds = cs + heads * DH * DH;      // [heads][32][32]
  float* km = ds + heads * DH * DH;      // [heads*32]
  float* kl = km + HD;                   // 1/l
  float* tv = kl + HD;
  const int unit = blockIdx.x;
  const int h = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < heads * DH * DH; e += blockDim.x) {
    cs[e] = ctx[(int64_t)unit * heads * DH * DH + e];
    ds[e] = dctx[(int64_t)unit * heads * DH * DH + e];
  }
  for (int e = threadIdx.x; e < HD; e += blockDim.x) {
    km[e] = kstats[((int64_t)unit * HD + e) * 2];
    kl[e] = 1.0f / kstats[((int64_t)unit * HD + e) * 2 + 1];
    tv[e] = tvec[(int64_t)unit * HD + e];
  }
  __shared__ unsigned blk_amax;
  if (threadIdx.x == 0) blk_amax = 0u;
  __syncthreads();
  const int j = blockIdx.y * 64 + (threadIdx.x & 63);
  if (j >= n) return;                       // (a finished wave no longer counts at the barrier below)
  float am = 0.f;
  const int64_t row = (int64_t)unit * n + j;
  const float4* cp = reinterpret_cast<const float4*>(cs + h * DH * DH);
  const float4* dp = reinterpret_cast<const float4*>(ds + h * DH * DH);
  float* wq = dqkv + row * RW + h * DH;
  {  // ---- dq
    float q[DH], go[DH];
    const float4* qp = reinterpret_cast<const float4*>(qkv + row * RW + h * DH);
    const float4* gp = reinterpret_cast<const float4*>(dout + row * HD + h * DH);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float4 v = qp[e]; q[4 * e] = v.x; q[4 * e + 1] = v.y; q[4 * e + 2] = v.z; q[4 * e + 3] = v.w;
      float4 g = gp[e]; go[4 * e] = g.x; go[4 * e + 1] = g.y; go[4 * e + 2] = g.z; go[4 * e + 3] = g.w;
    }
    float mx = q[0];
#pragma unroll
    for (int e = 1; e < DH; ++e) mx = fmaxf(mx, q[e]);
    float sm = 0.f;
#pragma unroll
    for (int e = 0; e < DH; ++e) { q[e] = expf(q[e] - mx); sm += q[e]; }
    float inv = 1.0f / sm, dot = 0.f;
    float dqs[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      float a = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float4 c = cp[d * 8 + e];
        a = fmaf(go[4 * e], c.x, a); a = fmaf(go[4 * e + 1], c.y, a); a = fmaf(go[4 * e + 2], c.z, a); a = fmaf(go[4 * e + 3], c.w, a);
      }
      q[d] *= inv;
      dqs[d] = a;
      dot = fmaf(q[d], a, dot);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float4 v = make_float4(scale * q[4 * e] * (dqs[4 * e] - dot), scale * q[4 * e + 1] * (dqs[4 * e + 1] - dot),
                                   scale * q[4 * e + 2] * (dqs[4 * e + 2] - dot), scale * q[4 * e + 3] * (dqs[4 * e + 3] - dot));
      reinterpret_cast<float4*>(wq)[e] = v;
      am = amax4(am, v);
    }
  }
  {  // ---- dk, dv
    float ks[DH], vv[DH], dv[DH];
    const float4* kp = reinterpret_cast<const float4*>(qkv + row * RW + HD + h * DH);
    const float4* vp = reinterpret_cast<const float4*>(qkv + row * RW + 2 * HD + h * DH);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float4 v = kp[e]; ks[4 * e] = v.x; ks[4 * e + 1] = v.y; ks[4 * e + 2] = v.z; ks[4 * e + 3] = v.w;
      float4 u = vp[e]; vv[4 * e] = u.x; vv[4 * e + 1] = u.y; vv[4 * e + 2] = u.z; vv[4 * e + 3] = u.w;
    }
#pragma unroll
    for (int e = 0; e < DH; ++e) { ks[e] = expf(ks[e] - km[h * DH + e]) * kl[h * DH + e]; dv[e] = 0.f; }
    float dk[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) {
      float a = 0.f, w = ks[d];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float4 c = dp[d * 8 + e];
        a = fmaf(vv[4 * e], c.x, a); a = fmaf(vv[4 * e + 1], c.y, a); a = fmaf(vv[4 * e + 2], c.z, a); a = fmaf(vv[4 * e + 3], c.w, a);
        dv[4 * e] = fmaf(w, c.x, dv[4 * e]); dv[4 * e + 1] = fmaf(w, c.y, dv[4 * e + 1]);
        dv[4 * e + 2] = fmaf(w, c.z, dv[4 * e + 2]); dv[4 * e + 3] = fmaf(w, c.w, dv[4 * e + 3]);
      }
      dk[d] = w * (a - tv[h * DH + d]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float4 gk = make_float4(dk[4 * e], dk[4 * e + 1], dk[4 * e + 2], dk[4 * e + 3]);
      const float4 gv = make_float4(dv[4 * e], dv[4 * e + 1], dv[4 * e + 2], dv[4 * e + 3]);
      reinterpret_cast<float4*>(wq + HD)[e] = gk;
      reinterpret_cast<float4*>(wq + 2 * HD)[e] = gv;
      am = amax4(amax4(am, gk), gv);
    }
  }
  if (amax_rec) {     // lanes past the last token have left: an LDS atomic per lane instead of a wave shuffle, one global atomic per block
    atomicMax(&blk_amax, __float_as_uint(am));
    __syncthreads();
    if (threadIdx.x == 0)
      atomicMax(reinterpret_cast<unsigned*>(amax_rec) + ((blockIdx.y * gridDim.x + blockIdx.x) & (WDNO_AMAX_SLOTS - 1)) * WDNO_AMAX_STRIDE, blk_amax);
  }
}

// The same backward pass on MFMA tiles: one wave per (unit, head, 32-token chunk), the four waves of a block take four
// consecutive chunks of one (unit, head) and share its ctx / dctx tiles. The thread-per-token kernel above needs 256 + 182
// registers (one wave per SIMD) and every lane walks its own 1.5-KB-strided rows; here the rows are staged through LDS by
// coalesced 128-byte reads (am_stage_rows) and the three 32 x 32 x 32 products run on v_mfma_f32_32x32x2_f32, computed
// TRANSPOSED so that lane (token, half) ends up with 16 of the token's 32 channels (runs of four: 16-byte stores):
//   dqs^T[d][t] = sum_e ctx[d][e]  dout[t][e]       a^T[d][t] = sum_e dctx[d][e] v[t][e]       dv^T[e][t] = sum_d dctx[d][e] ks[t][d]
// The channel softmax of q and the <qsm, dqs> dot product need the other half of the row: one lane ^ 32 exchange each.
#define LAM_TILE (32 * AM_TS)
__global__ __launch_bounds__(256, 2) void linattn_bwd_tok_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                       const float* __restrict__ kstats, const float* __restrict__ ctx,
                                                                       const float* __restrict__ dctx, const float* __restrict__ tvec,
                                                                       float* __restrict__ dqkv, int n, int heads, float scale,
                                                                       float* __restrict__ amax_rec, _Float16* __restrict__ pl_hi = nullptr,
                                                                       _Float16* __restrict__ pl_lo = nullptr, const float* __restrict__ rec_qkv = nullptr,
                                                                       const float* __restrict__ rec_dout = nullptr,
                                                                       const float* __restrict__ rec_dctx = nullptr, float* __restrict__ pl_scale = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float lsm[];
  float* Tc = lsm;                       // ctx  [d][e]
  float* Td = Tc + LAM_TILE;             // dctx [d][e]
  float* km = Td + LAM_TILE;             // per d: max, 1 / sum of the token softmax of k; T[d]
  float* kl = km + DH;
  float* tv = kl + DH;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  float* T1 = tv + DH + wave * 3 * LAM_TILE;      // q, then dout
  float* T2 = T1 + LAM_TILE;                      // k
  float* T3 = T2 + LAM_TILE;                      // v
  const int HD = heads * DH, RW = 3 * HD;
  const int unit = blockIdx.x / heads, h = blockIdx.x - unit * heads;
  {
    const float* cs = ctx + ((int64_t)unit * heads + h) * DH * DH;
    const float* ds = dctx + ((int64_t)unit * heads + h) * DH * DH;
    for (int e = threadIdx.x; e < DH * DH / 4; e += 256) {
      const int r = e >> 3, c4 = (e & 7) * 4;
      *reinterpret_cast<float4*>(Tc + r * AM_TS + c4) = reinterpret_cast<const float4*>(cs)[e];
      *reinterpret_cast<float4*>(Td + r * AM_TS + c4) = reinterpret_cast<const float4*>(ds)[e];
    }
    if (threadIdx.x < DH) {
      const int64_t col = (int64_t)unit * HD + h * DH + threadIdx.x;
      km[threadIdx.x] = kstats[col * 2];
      kl[threadIdx.x] = 1.0f / kstats[col * 2 + 1];
      tv[threadIdx.x] = tvec[col];
    }
  }
  __syncthreads();
  float am = 0.f;
  // Planes output (wdno_linattn_bwd_planes): with A = max|qkv|, G = max|dout|, D = max|dctx| (measured), ks, qsm <= 1 and |ctx| <= A:
  // |dq| <= 2 scale 32 A G,  |dk| <= 2 * 32 A D,  |dv| <= 32 D.
  float ps = 1.0f;
  if (pl_hi && pl_lo) {
    const float A = amax_record_read(rec_qkv), G = amax_record_read(rec_dout), D = amax_record_read(rec_dctx);
    ps = scale_from_amax(1.01f * fmaxf(64.f * scale * A * G, fmaxf(64.f * A * D, 32.f * D)));
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) pl_scale[0] = ps;
  }
  const int t0 = (blockIdx.y * 4 + wave) * 32;
  if (t0 < n) {                                     // (no block-wide barrier below)
    const int nv = min(32, n - t0);
    const bool tok = li < nv;
    const int64_t row0 = (int64_t)unit * n + t0;
    const float* qb = am_uniform(qkv + row0 * RW + h * DH);
    const float* gb = am_uniform(dout + row0 * HD + h * DH);
    float* db = const_cast<float*>(am_uniform(dqkv + row0 * RW + h * DH)) + (unsigned)(tok ? li : 0) * (unsigned)RW;
    const int64_t pbase = row0 * RW + h * DH + (int64_t)((unsigned)(tok ? li : 0) * (unsigned)RW);
    am_stage_rows(T1, qb, (unsigned)RW, nullptr, nullptr, 1.0f, nv, lane);
    am_stage_rows(T2, qb + HD, (unsigned)RW, nullptr, nullptr, 1.0f, nv, lane);
    am_stage_rows(T3, qb + 2 * HD, (unsigned)RW, nullptr, nullptr, 1.0f, nv, lane);
    __builtin_amdgcn_wave_barrier();
    // channel softmax of this lane's token: channels d = 8*e4 + 4*hh + c here, the other sixteen in lane ^ 32
    float qsm[16];
    {
      float mx = -INFINITY;
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const float4 t = *reinterpret_cast<const float4*>(T1 + li * AM_TS + 8 * e4 + 4 * hh);
        qsm[4 * e4] = t.x; qsm[4 * e4 + 1] = t.y; qsm[4 * e4 + 2] = t.z; qsm[4 * e4 + 3] = t.w;
        mx = fmaxf(fmaxf(mx, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sm = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) { qsm[e] = expf(qsm[e] - mx); sm += qsm[e]; }
      sm += __shfl_xor(sm, 32);
      const float inv = 1.0f / sm;
#pragma unroll
      for (int e = 0; e < 16; ++e) qsm[e] *= inv;
    }
    __builtin_amdgcn_wave_barrier();                // every lane has read its q row: the tile takes dout now
    am_stage_rows(T1, gb, (unsigned)HD, nullptr, nullptr, 1.0f, nv, lane);
    __builtin_amdgcn_wave_barrier();
    {   // ---- dq = scale * qsm * (dqs - <qsm, dqs>)
      float ca[16], ga[16];
      am_sel(Tc, li, hh, ca);
      am_sel(T1, li, hh, ga);
      const f32x16 acc = am_mfma16(ca, ga, tf_zero());
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) dot = fmaf(qsm[e], acc[e], dot);
      dot += __shfl_xor(dot, 32);
      float4 vv[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const float4 v = make_float4(scale * qsm[4 * e4] * (acc[4 * e4] - dot), scale * qsm[4 * e4 + 1] * (acc[4 * e4 + 1] - dot),
                                     scale * qsm[4 * e4 + 2] * (acc[4 * e4 + 2] - dot), scale * qsm[4 * e4 + 3] * (acc[4 * e4 + 3] - dot));
        vv[e4] = v;
        if (tok && !pl_hi) *reinterpret_cast<float4*>(db + 8 * e4 + 4 * hh) = v;
        if (tok) am = amax4(am, v);                      // lanes past the last token hold values of no token
      }
      if (tok && pl_hi) am_store_row_planes(pl_hi, pl_lo, pbase, hh, vv, ps);
    }
    {   // ---- dk[d] = ks[d] * (sum_e v[e] dctx[d][e] - T[d]),  ks = exp(k - max) / sum
      float da[16], va[16];
      am_sel(Td, li, hh, da);
      am_sel(T3, li, hh, va);
      const f32x16 acc = am_mfma16(da, va, tf_zero());
      float4 vk[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int d0 = 8 * e4 + 4 * hh;
        const float4 kk = *reinterpret_cast<const float4*>(T2 + li * AM_TS + d0);
        const float4 m4 = *reinterpret_cast<const float4*>(km + d0), l4 = *reinterpret_cast<const float4*>(kl + d0);
        const float4 t4 = *reinterpret_cast<const float4*>(tv + d0);
        const float4 v = make_float4(expf(kk.x - m4.x) * l4.x * (acc[4 * e4] - t4.x), expf(kk.y - m4.y) * l4.y * (acc[4 * e4 + 1] - t4.y),
                                     expf(kk.z - m4.z) * l4.z * (acc[4 * e4 + 2] - t4.z), expf(kk.w - m4.w) * l4.w * (acc[4 * e4 + 3] - t4.w));
        vk[e4] = v;
        if (tok && !pl_hi) *reinterpret_cast<float4*>(db + HD + d0) = v;
        if (tok) am = amax4(am, v);
      }
      if (tok && pl_hi) am_store_row_planes(pl_hi, pl_lo, pbase + HD, hh, vk, ps);
    }
    {   // ---- dv[e] = sum_d ks[d] dctx[d][e]: row operand = dctx read by columns (lane = e), column operand = ks[t][2m + hh]
      float da[16], ka[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int d = AM_D(m, hh);
        da[m] = Td[d * AM_TS + li];
        ka[m] = expf(T2[li * AM_TS + d] - km[d]) * kl[d];
      }
      const f32x16 acc = am_mfma16(da, ka, tf_zero());
      float4 vd[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const float4 v = make_float4(acc[4 * e4], acc[4 * e4 + 1], acc[4 * e4 + 2], acc[4 * e4 + 3]);
        vd[e4] = v;
        if (tok && !pl_hi) *reinterpret_cast<float4*>(db + 2 * HD + 8 * e4 + 4 * hh) = v;
        if (tok) am = amax4(am, v);
      }
      if (tok && pl_hi) am_store_row_planes(pl_hi, pl_lo, pbase + 2 * HD, hh, vd, ps);
    }
  }
  if (amax_rec) wave_amax_emit(am, amax_rec, (int)((blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave));
}

// pass 3 on MFMA tiles (same layout as linattn_bwd_tok_mfma_kernel): out^T[e][t] = sum_d ctx[d][e] qs[t][d], qs = scale * softmax_d(q).
// Row operand = ctx read by columns (lane = e), column operand = qs[t][2m + hh]; the two halves of a token's softmax sit in
// lanes t and t + 32.
__global__ __launch_bounds__(256, 2) void linattn_out_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ ctx,
                                                                   float* __restrict__ out, int n, int heads, float scale,
                                                                   float* __restrict__ amax_rec, _Float16* __restrict__ pl_hi = nullptr,
                                                                   _Float16* __restrict__ pl_lo = nullptr, const float* __restrict__ rec_qkv = nullptr,
                                                                   float* __restrict__ pl_scale = nullptr) {
  __shared__ __attribute__((aligned(16))) float Tc[LAM_TILE];
  __shared__ __attribute__((aligned(16))) float Tq[4][LAM_TILE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  const int HD = heads * DH, RW = 3 * HD;
  const int unit = blockIdx.x / heads, h = blockIdx.x - unit * heads;
  {
    const float* cs = ctx + ((int64_t)unit * heads + h) * DH * DH;
    for (int e = threadIdx.x; e < DH * DH / 4; e += 256) {
      const int r = e >> 3, c4 = (e & 7) * 4;
      *reinterpret_cast<float4*>(Tc + r * AM_TS + c4) = reinterpret_cast<const float4*>(cs)[e];
    }
  }
  __syncthreads();
  float ops = 1.0f;
  if (pl_hi && pl_lo) {
    ops = scale_from_amax(1.01f * scale * amax_record_read(rec_qkv));
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) pl_scale[0] = ops;
  }
  float am = 0.f;
  const int t0 = (blockIdx.y * 4 + wave) * 32;
  if (t0 < n) {
    const int nv = min(32, n - t0);
    const bool tok = li < nv;
    const int64_t row0 = (int64_t)unit * n + t0;
    float* T1 = Tq[wave];
    am_stage_rows(T1, am_uniform(qkv + row0 * RW + h * DH), (unsigned)RW, nullptr, nullptr, 1.0f, nv, lane);
    __builtin_amdgcn_wave_barrier();
    float qs[16], ca[16];
    am_sel(T1, li, hh, qs);
    float mx = qs[0];
#pragma unroll
    for (int m = 1; m < 16; ++m) mx = fmaxf(mx, qs[m]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sm = 0.f;
#pragma unroll
    for (int m = 0; m < 16; ++m) { qs[m] = expf(qs[m] - mx); sm += qs[m]; }
    sm += __shfl_xor(sm, 32);
    const float f = scale / sm;
#pragma unroll
    for (int m = 0; m < 16; ++m) { qs[m] *= f; ca[m] = Tc[AM_D(m, hh) * AM_TS + li]; }
    const f32x16 acc = am_mfma16(ca, qs, tf_zero());
    float* orow = out + (row0 + (tok ? li : 0)) * HD + h * DH;
    float4 vo[4];
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const float4 v = make_float4(acc[4 * e4], acc[4 * e4 + 1], acc[4 * e4 + 2], acc[4 * e4 + 3]);
      vo[e4] = v;
      if (tok && !pl_hi) *reinterpret_cast<float4*>(orow + 8 * e4 + 4 * hh) = v;
      am = amax4(am, v);
    }
    // planes for the to_out projection INSTEAD of the fp32 tensor (the backward works from ctx, not from out):
    // qs sums to `scale` over d and |ctx| <= max|v|, so |out| <= scale * max|qkv|
    if (tok && pl_hi) am_store_row_planes(pl_hi, pl_lo, (row0 + li) * HD + h * DH, hh, vo, ops);
  }
  if (amax_rec) wave_amax_emit(am, amax_rec, (int)((blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave));
}

static int la_check(int64_t units, int n, int heads) {
  if (units <= 0 || n <= 0 || heads <= 0 || units > 0x7fffffff / 8) return WDNO_EINVAL;
  if (heads != 1 && heads != 2 && heads != 4) return WDNO_EUNSUPPORTED;   // 64*heads threads per block
  return WDNO_OK;
}
// The backward workspace holds chunk partials of the context pass (LA_MAXCHUNKS per (unit, head)) only up to 2 x CUs (unit, head) pairs: the
// ONE statement of that condition -- wdno_linattn_ws_bytes sizes by it, la_choose cuts by it, la_bwd_ctx carves by it.
static bool la_ws_has_chunk_partials(int64_t units, int heads) { return units * heads <= 2 * (int64_t)wdno_num_cus(); }
// backward workspace: dctx [units,heads,32,32] + T [units,heads,32] (+ the partial contexts of a chunked token range)
extern "C" size_t wdno_linattn_ws_bytes(int64_t units, int heads) {
  const size_t chunk_part = la_ws_has_chunk_partials(units, heads) ? (size_t)units * heads * LA_MAXCHUNKS * DH * DH : 0;
  return ((size_t)units * heads * DH * DH + (size_t)units * heads * DH + chunk_part) * sizeof(float);
}
// the cuts of a call: the ONE place that decides them (the launch paths below and wdno_linattn_plan both ask here)
static int la_choose(int64_t units, int n_tok, int heads, bool backward, size_t ws_bytes, wdno_la_plan& pl) {
  pl = wdno_la_plan{0, 0, 0, 0, la_check(units, n_tok, heads)};
  if (pl.rc) return pl.rc;
  if (backward && ws_bytes < wdno_linattn_ws_bytes(units, heads)) return pl.rc = WDNO_EWORKSPACE;
  if (!backward) {
    pl.kstats_chunks = n_tok / 64;
    pl.kstats_chunks = pl.kstats_chunks < 1 ? 1 : (pl.kstats_chunks > 16 ? 16 : pl.kstats_chunks);
  }
  // forward: the chunk partials always have room (they go through `out` / the hi plane); backward: only where the workspace holds them
  pl.ctx_chunks = !backward || la_ws_has_chunk_partials(units, heads) ? la_ctx_chunks(units, heads, n_tok) : 1;
  pl.family = wdno_debug_mode == WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV ? 1 : 0;
  pl.token_tiles = cdiv(n_tok, pl.family ? 64 : 128);
  return WDNO_OK;
}
extern "C" int wdno_linattn_plan(int64_t units, int n_tok, int heads, int backward, size_t ws_bytes, wdno_la_plan* out) {
  if (!out) return WDNO_EINVAL;
  la_choose(units, n_tok, heads, backward != 0, ws_bytes, *out);
  return WDNO_OK;
}
// forward passes 1 and 2: the token softmax statistics of k (chunked or not), then the context. The partial statistics go through `ctx`
// (written only afterwards by the context kernel): chunks * HD * 2 <= 32 * HD floats per unit. The chunk partials of the context go through
// `part`, a buffer only the output kernel writes afterwards: `out` (units * heads * chunks * 1024 floats <= units * n_tok * HD because
// chunks <= n_tok / 128) or the hi plane (units * heads * chunks * 4096 bytes <= units * n_tok * HD * 2).
static void la_fwd_ctx(const float* qkv, float* kstats, float* ctx, float* part, int64_t units, int n_tok, int heads, float scale,
                       const wdno_la_plan& pl, hipStream_t st) {
  const int chunks = pl.kstats_chunks;
  if (chunks == 1) {
    linattn_kstats_kernel<<<(unsigned)units, 256, 0, st>>>(qkv, kstats, n_tok, heads * DH, 1);
  } else {
    linattn_kstats_kernel<<<(unsigned)(units * chunks), 256, 0, st>>>(qkv, ctx, n_tok, heads * DH, chunks);
    const int64_t cols = units * heads * DH;
    linattn_kstats_merge_kernel<<<(unsigned)cdiv64(cols, 256), 256, 0, st>>>(ctx, kstats, cols, heads * DH, chunks);
  }
  la_ctx_launch<0>(qkv, nullptr, kstats, nullptr, ctx, nullptr, part, units, n_tok, heads, scale, pl.ctx_chunks, st);
}
// backward pass 1: the workspace carved into dctx | T | chunk partials (where it holds them), then the context-gradient pass
struct LaBwdWs { float* dctx; float* tvec; };
static LaBwdWs la_bwd_ctx(const float* qkv, const float* dout, const float* ctx, void* ws, int64_t units, int n_tok, int heads, float scale,
                          const wdno_la_plan& pl, hipStream_t st) {
  float* dctx = (float*)ws;
  float* tvec = dctx + (size_t)units * heads * DH * DH;
  float* cpart = la_ws_has_chunk_partials(units, heads) ? tvec + (size_t)units * heads * DH : nullptr;
  la_ctx_launch<1>(qkv, dout, nullptr, ctx, dctx, tvec, cpart, units, n_tok, heads, scale, pl.ctx_chunks, st);
  return LaBwdWs{dctx, tvec};
}
// dynamic LDS of linattn_bwd_tok_mfma_kernel: ctx, dctx and three tiles per wave, the k statistics and T
#define LAM_BWD_LDS (((size_t)(2 + 4 * 3) * LAM_TILE + 3 * DH) * sizeof(float))

extern "C" int wdno_linattn_fwd(const float* qkv, float* out, float* kstats, float* ctx, int64_t units, int n_tok, int heads,
                                float scale, wdno_stream_t s) {
  return wdno_linattn_fwd_amax(qkv, out, kstats, ctx, nullptr, units, n_tok, heads, scale, s);
}
extern "C" int wdno_linattn_fwd_amax(const float* qkv, float* out, float* kstats, float* ctx, float* amax_rec, int64_t units, int n_tok,
                                     int heads, float scale, wdno_stream_t s) {
  wdno_la_plan pl;
  int rc = la_choose(units, n_tok, heads, false, 0, pl);
  if (rc) return rc;
  hipStream_t st = as_stream(s);
  la_fwd_ctx(qkv, kstats, ctx, out, units, n_tok, heads, scale, pl, st);
  if (pl.family == 0) {            // else: the thread-per-token kernel
    linattn_out_mfma_kernel<<<dim3((unsigned)(units * heads), (unsigned)pl.token_tiles), 256, 0, st>>>(qkv, ctx, out, n_tok, heads, scale, amax_rec);
    return wdno_check_launch();
  }
  size_t lds = (size_t)heads * DH * DH * sizeof(float);
  linattn_out_kernel<<<dim3((unsigned)units, (unsigned)pl.token_tiles), 64 * heads, lds, st>>>(qkv, ctx, out, n_tok, heads, scale, amax_rec);
  return wdno_check_launch();
}
extern "C" int wdno_linattn_bwd(const float* qkv, const float* dout, const float* kstats, const float* ctx, float* dqkv,
                                void* ws, size_t ws_bytes, int64_t units, int n_tok, int heads, float scale, wdno_stream_t s) {
  return wdno_linattn_bwd_amax(qkv, dout, kstats, ctx, dqkv, nullptr, ws, ws_bytes, units, n_tok, heads, scale, s);
}
extern "C" int wdno_linattn_bwd_amax(const float* qkv, const float* dout, const float* kstats, const float* ctx, float* dqkv,
                                     float* amax_rec, void* ws, size_t ws_bytes, int64_t units, int n_tok, int heads, float scale,
                                     wdno_stream_t s) {
  wdno_la_plan pl;
  int rc = la_choose(units, n_tok, heads, true, ws_bytes, pl);
  if (rc) return rc;
  hipStream_t st = as_stream(s);
  const LaBwdWs w = la_bwd_ctx(qkv, dout, ctx, ws, units, n_tok, heads, scale, pl, st);
  if (pl.family == 0) {            // else: the thread-per-token kernel
    static bool attr_done = false;      // once per process (and once more in wdno_linattn_bwd_planes)
    if (!attr_done) { am_dyn_lds((const void*)linattn_bwd_tok_mfma_kernel, LAM_BWD_LDS); attr_done = true; }
    linattn_bwd_tok_mfma_kernel<<<dim3((unsigned)(units * heads), (unsigned)pl.token_tiles), 256, LAM_BWD_LDS, st>>>(qkv, dout, kstats, ctx, w.dctx, w.tvec,
                                                                                                                 dqkv, n_tok, heads, scale, amax_rec);
    return wdno_check_launch();
  }
  size_t lds = ((size_t)2 * heads * DH * DH + 3 * heads * DH) * sizeof(float);
  if (lds > 64 * 1024) am_dyn_lds((const void*)linattn_bwd_tok_kernel, lds);
  linattn_bwd_tok_kernel<<<dim3((unsigned)units, (unsigned)pl.token_tiles), 64 * heads, lds, st>>>(qkv, dout, kstats, ctx, w.dctx, w.tvec, dqkv,
                                                                                                n_tok, heads, scale, amax_rec);
  return wdno_check_launch();
}

// dqkv as fp16 planes for the gradient kernels of the qkv projection. rec_dctx: a zeroed amax record, receives max|dctx| (a sweep over the
// small dctx tensor between the two launches). Always the MFMA token kernel on cdiv(n_tok, 128) tiles, whatever pl.family says.
extern "C" int wdno_linattn_bwd_planes(const float* qkv, const float* dout, const float* kstats, const float* ctx, void* dqkv_hi,
                                       void* dqkv_lo, float* dqkv_scale, const float* rec_qkv, const float* rec_dout, float* rec_dctx,
                                       void* ws, size_t ws_bytes, int64_t units, int n_tok, int heads, float scale, wdno_stream_t s) {
  int rc = la_check(units, n_tok, heads);
  if (rc) return rc;
  if (!dqkv_hi || (dqkv_lo && (!dqkv_scale || !rec_qkv || !rec_dout || !rec_dctx))) return WDNO_EINVAL;      // dqkv_lo == NULL: one bf16 plane
  wdno_la_plan pl;
  rc = la_choose(units, n_tok, heads, true, ws_bytes, pl);
  if (rc) return rc;
  hipStream_t st = as_stream(s);
  const LaBwdWs w = la_bwd_ctx(qkv, dout, ctx, ws, units, n_tok, heads, scale, pl, st);
  if (dqkv_lo) {
    rc = wdno_amax_record(w.dctx, (int64_t)units * heads * DH * DH, rec_dctx, s);
    if (rc) return rc;
  }
  static bool attr_done = false;      // once per process (and once more in wdno_linattn_bwd_amax)
  if (!attr_done) { am_dyn_lds((const void*)linattn_bwd_tok_mfma_kernel, LAM_BWD_LDS); attr_done = true; }
  linattn_bwd_tok_mfma_kernel<<<dim3((unsigned)(units * heads), (unsigned)cdiv(n_tok, 128)), 256, LAM_BWD_LDS, st>>>(
      qkv, dout, kstats, ctx, w.dctx, w.tvec, nullptr, n_tok, heads, scale, nullptr, (_Float16*)dqkv_hi, (_Float16*)dqkv_lo, rec_qkv, rec_dout, rec_dctx,
      dqkv_scale);
  return wdno_check_launch();
}

// forward with out delivered as fp16 planes only. Always the MFMA output kernel on cdiv(n_tok, 128) tiles; la_choose cannot refuse once
// la_check has passed (a forward plan needs no workspace).
extern "C" int wdno_linattn_fwd_planes(const float* qkv, void* out_hi, void* out_lo, float* out_scale, float* kstats, float* ctx,
                                       const float* rec_qkv, int64_t units, int n_tok, int heads, float scale, wdno_stream_t s) {
  int rc = la_check(units, n_tok, heads);
  if (rc) return rc;
  if (!out_hi || (out_lo && (!out_scale || !rec_qkv))) return WDNO_EINVAL;      // out_lo == NULL: one bf16 plane
  wdno_la_plan pl;
  la_choose(units, n_tok, heads, false, 0, pl);
  hipStream_t st = as_stream(s);
  la_fwd_ctx(qkv, kstats, ctx, (float*)out_hi, units, n_tok, heads, scale, pl, st);
  linattn_out_mfma_kernel<<<dim3((unsigned)(units * heads), (unsigned)cdiv(n_tok, 128)), 256, 0, st>>>(
      qkv, ctx, nullptr, n_tok, heads, scale, nullptr, (_Float16*)out_hi, (_Float16*)out_lo, rec_qkv, out_scale);
  return wdno_check_launch();
}
