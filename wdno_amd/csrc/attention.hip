// attention.hip -- softmax attention of the two U-Nets (head dim fixed at 32, as in the reference) over short token axes
// (temporal: 24/48 frames with rotary + relative-position bias; spatial mid-block: 64/100/400 tokens): one wavefront per
// (unit, head), K/V staged in LDS, rows streamed. HBM-bound (no reuse at n = 24); QK^T / PV are far too small to feed MFMA tiles.
// The lane-level steps the kernels share with each other and with linear attention (linattn.hip) are in attn_tiles.h.
#include "attn_tiles.h"
#include "debug_modes.h"

// ================================================================================================ softmax attention
// One THREAD per (unit, head, query row). The rotated K rows of an item live in LDS (every thread of the item reads the
// same row -> broadcast ds_read_b128, no conflicts); V rows and dO rows are read straight from global memory as
// wave-broadcast float4 loads (one cache line per item per load). Scores are recomputed in a second pass instead of
// being stored (n is 24..400), so the forward needs no per-thread arrays beyond q[32] / out[32].
struct AttnP {
  wdno_attn_desc d;
  float scale;
  int RW;   // 3*heads*32
  int HD;   // heads*32
  int ipb;  // items (unit, head) per block
  int kst;  // LDS floats per item for one [n][32] matrix (padded)
  int64_t n_items;
  int db_slices;   // matrix backward, bias gradient in LDS: 1 = one [heads][n][n] partial per wave (heads % 4 != 0: two waves can hold the same head)
  float* amax_rec;   // optional amax record (common.h) of the tensor the kernel writes: out (forward), dqkv (backward)
  // backward with dqkv delivered as fp16 (hi, lo) planes (wdno_attn_bwd_planes): the plane pointers, the amax records of qkv and
  // dout the scale bound is derived from, and where the scale is left
  _Float16* pl_hi; _Float16* pl_lo; const float* rec_qkv; const float* rec_dout; float* pl_scale;
};

#define ATT_THREADS 256
#define ATT_BWD_THREADS 128

__device__ __forceinline__ void load_row32(const float* __restrict__ p, float* v) {
  const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) { float4 t = q[e]; v[4 * e] = t.x; v[4 * e + 1] = t.y; v[4 * e + 2] = t.z; v[4 * e + 3] = t.w; }
}
__device__ __forceinline__ void store_row32(float* __restrict__ p, const float* v) {
  float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) q[e] = make_float4(v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]);
}
// interleaved-pair rotary: (x0, x1) -> (x0 c - x1 s, x1 c + x0 s); inverse = transpose
__device__ __forceinline__ void rotate32(float* v, const float* __restrict__ cs, const float* __restrict__ sn, bool inverse) {
  float c[DH], s[DH];
  load_row32(cs, c);
  load_row32(sn, s);
#pragma unroll
  for (int e = 0; e < DH; e += 2) {
    float x0 = v[e], x1 = v[e + 1];
    float s0 = inverse ? -s[e] : s[e], s1 = inverse ? -s[e + 1] : s[e + 1];
    v[e] = x0 * c[e] - x1 * s0;
    v[e + 1] = x1 * c[e + 1] + x0 * s1;
  }
}
__device__ __forceinline__ float dot32_lds(const float* q, const float* __restrict__ krow) {
  const float4* k4 = reinterpret_cast<const float4*>(krow);
  float a = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float4 t = k4[e];
    a = fmaf(q[4 * e], t.x, a); a = fmaf(q[4 * e + 1], t.y, a); a = fmaf(q[4 * e + 2], t.z, a); a = fmaf(q[4 * e + 3], t.w, a);
  }
  return a;
}

__global__ __launch_bounds__(ATT_THREADS) void attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ rcos,
                                                                const float* __restrict__ rsin, const float* __restrict__ bias,
                                                                float* __restrict__ out, AttnP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n = p.d.n_tok;
  const int il = threadIdx.x / n;                 // item slot inside the block (valid when < ipb)
  const int i0 = threadIdx.x - il * n;            // first row of this thread
  const int64_t item = (int64_t)blockIdx.x * p.ipb + il;
  const bool active = il < p.ipb && item < p.n_items;
  const AmItem w = am_item(p.d, item, active);
  const int h = w.h;
  const int64_t row0 = w.row0;
  float* Ks = smem + (active ? il : 0) * p.kst;
  const int rstep = p.ipb > 1 ? n : ATT_THREADS;  // ipb == 1: threads stride over rows
  if (active) {
    for (int j = i0; j < n; j += rstep) {
      float k[DH];
      load_row32(qkv + (row0 + (int64_t)j * p.d.st) * p.RW + p.HD + h * DH, k);
      if (rcos) rotate32(k, rcos + j * DH, rsin + j * DH, false);
      store_row32(Ks + j * DH, k);
    }
  }
  __syncthreads();
  if (!active) return;
  for (int i = i0; i < n; i += rstep) {
    float q[DH];
    load_row32(qkv + (row0 + (int64_t)i * p.d.st) * p.RW + h * DH, q);
#pragma unroll
    for (int e = 0; e < DH; ++e) q[e] *= p.scale;
    if (rcos) rotate32(q, rcos + i * DH, rsin + i * DH, false);
    const float* brow = bias ? bias + ((int64_t)h * n + i) * n : nullptr;
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < n; ++j) {
      float sv = dot32_lds(q, Ks + j * DH);
      if (brow) sv += brow[j];
      float mn = fmaxf(m, sv);
      l = l * expf(m - mn) + expf(sv - mn);
      m = mn;
    }
    const float inv = 1.0f / l;
    float o[DH];
#pragma unroll
    for (int e = 0; e < DH; ++e) o[e] = 0.f;
    for (int j = 0; j < n; ++j) {
      float sv = dot32_lds(q, Ks + j * DH);
      if (brow) sv += brow[j];
      float pj = expf(sv - m) * inv;
      const float4* v4 = reinterpret_cast<const float4*>(qkv + (row0 + (int64_t)j * p.d.st) * p.RW + 2 * p.HD + h * DH);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float4 t = v4[e];
        o[4 * e] = fmaf(pj, t.x, o[4 * e]); o[4 * e + 1] = fmaf(pj, t.y, o[4 * e + 1]);
        o[4 * e + 2] = fmaf(pj, t.z, o[4 * e + 2]); o[4 * e + 3] = fmaf(pj, t.w, o[4 * e + 3]);
      }
    }
    store_row32(out + (row0 + (int64_t)i * p.d.st) * p.HD + h * DH, o);
  }
}

// backward. Phase A (thread = query row i): p_ij, dS_ij, dQ_i ; phase B (thread = key row j): dK_j, dV_j from the P / dS
// matrices and the rotated Q rows left in LDS. delta_i = <dO_i, O_i> uses the saved forward output.
__global__ __launch_bounds__(ATT_BWD_THREADS) void attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ rcos,
                                                                    const float* __restrict__ rsin, const float* __restrict__ bias,
                                                                    const float* __restrict__ fout, const float* __restrict__ dout,
                                                                    float* __restrict__ dqkv, float* __restrict__ dbias, AttnP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n = p.d.n_tok, n1 = n + 1;
  const int item_lds = 2 * p.kst + 2 * n * n1;       // K, Q, P, dS per item
  float* dBs = smem + p.ipb * item_lds;              // [heads][n][n] when dbias
  const int il = threadIdx.x / n;
  const int i = threadIdx.x - il * n;
  const bool slot_ok = il < p.ipb;
  float* Ks = smem + (slot_ok ? il : 0) * item_lds;
  float* Qs = Ks + p.kst;
  float* Ps = Qs + p.kst;
  float* Ss = Ps + n * n1;
  if (dbias)
    for (int e = threadIdx.x; e < p.d.heads * n * n; e += ATT_BWD_THREADS) dBs[e] = 0.f;
  const int64_t ngroups = (p.n_items + p.ipb - 1) / p.ipb;
  for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int64_t item = grp * p.ipb + il;
    const bool active = slot_ok && item < p.n_items;
    const AmItem w = am_item(p.d, item, active);
    const int h = w.h;
    const int64_t row0 = w.row0, row = row0 + (int64_t)i * p.d.st;
    float q[DH];
    __syncthreads();                                  // previous group's phase B is done with the LDS matrices
    if (active) {
      float k[DH];
      load_row32(qkv + row * p.RW + p.HD + h * DH, k);
      load_row32(qkv + row * p.RW + h * DH, q);
#pragma unroll
      for (int e = 0; e < DH; ++e) q[e] *= p.scale;
      if (rcos) {
        rotate32(k, rcos + i * DH, rsin + i * DH, false);
        rotate32(q, rcos + i * DH, rsin + i * DH, false);
      }
      store_row32(Ks + i * DH, k);
      store_row32(Qs + i * DH, q);
    }
    __syncthreads();
    if (active) {
      float go[DH], dq[DH];
      load_row32(dout + row * p.HD + h * DH, go);
      float delta = 0.f;
      {
        const float4* o4 = reinterpret_cast<const float4*>(fout + row * p.HD + h * DH);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float4 t = o4[e];
          delta = fmaf(go[4 * e], t.x, delta); delta = fmaf(go[4 * e + 1], t.y, delta);
          delta = fmaf(go[4 * e + 2], t.z, delta); delta = fmaf(go[4 * e + 3], t.w, delta);
        }
      }
      const float* brow = bias ? bias + ((int64_t)h * n + i) * n : nullptr;
      float m = -INFINITY, l = 0.f;
      for (int j = 0; j < n; ++j) {
        float sv = dot32_lds(q, Ks + j * DH);
        if (brow) sv += brow[j];
        float mn = fmaxf(m, sv);
        l = l * expf(m - mn) + expf(sv - mn);
        m = mn;
      }
      const float inv = 1.0f / l;
#pragma unroll
      for (int e = 0; e < DH; ++e) dq[e] = 0.f;
      for (int j = 0; j < n; ++j) {
        const float4* k4 = reinterpret_cast<const float4*>(Ks + j * DH);
        const float4* v4 = reinterpret_cast<const float4*>(qkv + (row0 + (int64_t)j * p.d.st) * p.RW + 2 * p.HD + h * DH);
        float sv = 0.f, dp = 0.f;
        float4 kk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          kk[e] = k4[e];
          float4 t = v4[e];
          sv = fmaf(q[4 * e], kk[e].x, sv); sv = fmaf(q[4 * e + 1], kk[e].y, sv); sv = fmaf(q[4 * e + 2], kk[e].z, sv); sv = fmaf(q[4 * e + 3], kk[e].w, sv);
          dp = fmaf(go[4 * e], t.x, dp); dp = fmaf(go[4 * e + 1], t.y, dp); dp = fmaf(go[4 * e + 2], t.z, dp); dp = fmaf(go[4 * e + 3], t.w, dp);
        }
        if (brow) sv += brow[j];
        float pj = expf(sv - m) * inv;
        float ds = pj * (dp - delta);
        Ps[i * n1 + j] = pj;
        Ss[i * n1 + j] = ds;
        if (dbias) atomicAdd(&dBs[(h * n + i) * n + j], ds);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          dq[4 * e] = fmaf(ds, kk[e].x, dq[4 * e]); dq[4 * e + 1] = fmaf(ds, kk[e].y, dq[4 * e + 1]);
          dq[4 * e + 2] = fmaf(ds, kk[e].z, dq[4 * e + 2]); dq[4 * e + 3] = fmaf(ds, kk[e].w, dq[4 * e + 3]);
        }
      }
      if (rcos) rotate32(dq, rcos + i * DH, rsin + i * DH, true);
#pragma unroll
      for (int e = 0; e < DH; ++e) dq[e] *= p.scale;
      store_row32(dqkv + row * p.RW + h * DH, dq);
    }
    __syncthreads();
    if (active) {   // phase B: this thread owns key/value row j = i
      float dk[DH], dv[DH];
#pragma unroll
      for (int e = 0; e < DH; ++e) { dk[e] = 0.f; dv[e] = 0.f; }
      for (int r = 0; r < n; ++r) {
        float ds = Ss[r * n1 + i], pj = Ps[r * n1 + i];
        const float4* q4 = reinterpret_cast<const float4*>(Qs + r * DH);
        const float4* g4 = reinterpret_cast<const float4*>(dout + (row0 + (int64_t)r * p.d.st) * p.HD + h * DH);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float4 a = q4[e], b = g4[e];
          dk[4 * e] = fmaf(ds, a.x, dk[4 * e]); dk[4 * e + 1] = fmaf(ds, a.y, dk[4 * e + 1]);
          dk[4 * e + 2] = fmaf(ds, a.z, dk[4 * e + 2]); dk[4 * e + 3] = fmaf(ds, a.w, dk[4 * e + 3]);
          dv[4 * e] = fmaf(pj, b.x, dv[4 * e]); dv[4 * e + 1] = fmaf(pj, b.y, dv[4 * e + 1]);
          dv[4 * e + 2] = fmaf(pj, b.z, dv[4 * e + 2]); dv[4 * e + 3] = fmaf(pj, b.w, dv[4 * e + 3]);
        }
      }
      if (rcos) rotate32(dk, rcos + i * DH, rsin + i * DH, true);
      store_row32(dqkv + row * p.RW + p.HD + h * DH, dk);
      store_row32(dqkv + row * p.RW + 2 * p.HD + h * DH, dv);
    }
  }
  if (dbias) {         // dbias: this block's partial [heads][n][n] (plain stores; attn_dbias_reduce_kernel sums the blocks in index order)
    __syncthreads();
    float* part = dbias + (size_t)blockIdx.x * p.d.heads * n * n;
    for (int e = threadIdx.x; e < p.d.heads * n * n; e += ATT_BWD_THREADS) part[e] = dBs[e];
  }
}

// Backward over MANY tokens (129 .. 576; no rotation, no bias): the mid spatial attention of a model applied to a finer grid than it
// was built for (the space super-resolution model on 80 x 80 tensors attends over 20 x 20 = 400 tokens; the reference trains it on
// <= 40 x 40, data_2d.py:182-183, but nothing in its code stops a fine-tune at the sampling size). The n x n matrices P and dS do not
// fit LDS any more, so nothing is stored: one block per (unit, head) item;
//   phase A, thread = query row i: K and V rows in LDS; softmax statistics (m_i, 1 / l_i), delta_i = <dO_i, O_i>, dQ_i;
//   phase B, thread = key row j (k_j, v_j in registers): the rows q_i, dO_i stream from global memory as wave-broadcast loads (every
//   thread reads the same row: one line per load) and P_ij / dS_ij are recomputed from the statistics phase A left in LDS.
#define ATT_BIG_THREADS 256
#define ATT_BIG_MAXTOK 576
__global__ __launch_bounds__(ATT_BIG_THREADS) void attn_bwd_big_kernel(const float* __restrict__ qkv, const float* __restrict__ fout,
                                                                        const float* __restrict__ dout, float* __restrict__ dqkv, AttnP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n = p.d.n_tok;
  float* Ks = smem;                                   // [n][32]
  float* Vs = Ks + n * DH;                            // [n][32]
  float* Ms = Vs + n * DH;                            // [n] row maximum
  float* Ls = Ms + n;                                 // [n] 1 / row sum
  float* Dl = Ls + n;                                 // [n] delta
  for (int64_t item = blockIdx.x; item < p.n_items; item += gridDim.x) {
    const AmItem w = am_item(p.d, item);
    const int h = w.h;
    const int64_t row0 = w.row0;
    __syncthreads();                                  // the previous item's phase B has finished with the statistics
    for (int j = threadIdx.x; j < n; j += ATT_BIG_THREADS) {
      float k[DH], v[DH];
      const int64_t row = row0 + (int64_t)j * p.d.st;
      load_row32(qkv + row * p.RW + p.HD + h * DH, k);
      load_row32(qkv + row * p.RW + 2 * p.HD + h * DH, v);
      store_row32(Ks + j * DH, k);
      store_row32(Vs + j * DH, v);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += ATT_BIG_THREADS) {
      const int64_t row = row0 + (int64_t)i * p.d.st;
      float q[DH], go[DH], dq[DH];
      load_row32(qkv + row * p.RW + h * DH, q);
#pragma unroll
      for (int e = 0; e < DH; ++e) q[e] *= p.scale;
      load_row32(dout + row * p.HD + h * DH, go);
      float delta = 0.f;
      {
        const float4* o4 = reinterpret_cast<const float4*>(fout + row * p.HD + h * DH);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float4 t = o4[e];
          delta = fmaf(go[4 * e], t.x, delta); delta = fmaf(go[4 * e + 1], t.y, delta);
          delta = fmaf(go[4 * e + 2], t.z, delta); delta = fmaf(go[4 * e + 3], t.w, delta);
        }
      }
      float m = -INFINITY, l = 0.f;
      for (int j = 0; j < n; ++j) {
        const float sv = dot32_lds(q, Ks + j * DH);
        const float mn = fmaxf(m, sv);
        l = l * expf(m - mn) + expf(sv - mn);
        m = mn;
      }
      const float inv = 1.0f / l;
#pragma unroll
      for (int e = 0; e < DH; ++e) dq[e] = 0.f;
      for (int j = 0; j < n; ++j) {
        const float4* k4 = reinterpret_cast<const float4*>(Ks + j * DH);
        const float sv = dot32_lds(q, Ks + j * DH);
        const float dp = dot32_lds(go, Vs + j * DH);
        const float ds = expf(sv - m) * inv * (dp - delta);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float4 kk = k4[e];
          dq[4 * e] = fmaf(ds, kk.x, dq[4 * e]); dq[4 * e + 1] = fmaf(ds, kk.y, dq[4 * e + 1]);
          dq[4 * e + 2] = fmaf(ds, kk.z, dq[4 * e + 2]); dq[4 * e + 3] = fmaf(ds, kk.w, dq[4 * e + 3]);
        }
      }
#pragma unroll
      for (int e = 0; e < DH; ++e) dq[e] *= p.scale;
      store_row32(dqkv + row * p.RW + h * DH, dq);
      Ms[i] = m; Ls[i] = inv; Dl[i] = delta;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += ATT_BIG_THREADS) {
      float k[DH], v[DH], dk[DH], dv[DH];
      load_row32(Ks + j * DH, k);
      load_row32(Vs + j * DH, v);
#pragma unroll
      for (int e = 0; e < DH; ++e) { dk[e] = 0.f; dv[e] = 0.f; }
      for (int i = 0; i < n; ++i) {
        const int64_t row = row0 + (int64_t)i * p.d.st;
        const float4* q4 = reinterpret_cast<const float4*>(qkv + row * p.RW + h * DH);
        const float4* g4 = reinterpret_cast<const float4*>(dout + row * p.HD + h * DH);
        float4 qq[8], gg[8];
        float sv = 0.f, dp = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float4 a = q4[e];
          a.x *= p.scale; a.y *= p.scale; a.z *= p.scale; a.w *= p.scale;      // the same scaled q row phase A and the forward use
          qq[e] = a; gg[e] = g4[e];
          sv = fmaf(a.x, k[4 * e], sv); sv = fmaf(a.y, k[4 * e + 1], sv); sv = fmaf(a.z, k[4 * e + 2], sv); sv = fmaf(a.w, k[4 * e + 3], sv);
          dp = fmaf(gg[e].x, v[4 * e], dp); dp = fmaf(gg[e].y, v[4 * e + 1], dp); dp = fmaf(gg[e].z, v[4 * e + 2], dp); dp = fmaf(gg[e].w, v[4 * e + 3], dp);
        }
        const float pj = expf(sv - Ms[i]) * Ls[i];
        const float ds = pj * (dp - Dl[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          dk[4 * e] = fmaf(ds, qq[e].x, dk[4 * e]); dk[4 * e + 1] = fmaf(ds, qq[e].y, dk[4 * e + 1]);
          dk[4 * e + 2] = fmaf(ds, qq[e].z, dk[4 * e + 2]); dk[4 * e + 3] = fmaf(ds, qq[e].w, dk[4 * e + 3]);
          dv[4 * e] = fmaf(pj, gg[e].x, dv[4 * e]); dv[4 * e + 1] = fmaf(pj, gg[e].y, dv[4 * e + 1]);
          dv[4 * e + 2] = fmaf(pj, gg[e].z, dv[4 * e + 2]); dv[4 * e + 3] = fmaf(pj, gg[e].w, dv[4 * e + 3]);
        }
      }
      const int64_t row = row0 + (int64_t)j * p.d.st;
      store_row32(dqkv + row * p.RW + p.HD + h * DH, dk);
      store_row32(dqkv + row * p.RW + 2 * p.HD + h * DH, dv);
    }
  }
}

// Sum of the per-block relative-position-bias gradient partials in block order: E = heads * n * n outputs, each the sum of nb terms.
// (Global float atomics summed them in arrival order: the gradient of relative_attention_bias differed from run to run in its last
// bits, and with it every bit-reproducibility check of a training step.) 64 outputs per block, four partial sums per output.
#define DBR_EL 8                     // outputs per block
#define DBR_CH (256 / DBR_EL)        // partial chains per output
__global__ __launch_bounds__(256) void attn_dbias_reduce_kernel(const float* __restrict__ part, int nb, float* __restrict__ dbias, int E) {
  // 8 outputs per block (E / 8 = 288 blocks for 4 heads x 24 x 24), 32 chains per output with four independent sums each: the 768
  // partials of an output are 6 rounds of loads per thread (64 outputs per block and 4 chains were 192 dependent rounds on 36 blocks:
  // 50 us per launch). The order of every sum is fixed by the indices alone.
  __shared__ float red[DBR_CH][DBR_EL];
  const int el = threadIdx.x & (DBR_EL - 1), q = threadIdx.x / DBR_EL;
  const int e = blockIdx.x * DBR_EL + el;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (e < E) {
    int b = q;
    for (; b + 3 * DBR_CH < nb; b += 4 * DBR_CH) {
      a0 += part[(size_t)b * E + e]; a1 += part[(size_t)(b + DBR_CH) * E + e];
      a2 += part[(size_t)(b + 2 * DBR_CH) * E + e]; a3 += part[(size_t)(b + 3 * DBR_CH) * E + e];
    }
    for (; b < nb; b += DBR_CH) a0 += part[(size_t)b * E + e];
  }
  red[q][el] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (q == 0 && e < E) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < DBR_CH; ++k) t += red[k][el];
    dbias[e] = t;
  }
}

// ------------------------------------------------------------------------------------------------ n_tok <= 32: one wave per item
// With at most 32 tokens the score matrix is ONE 32x32 MFMA tile (v_mfma_f32_32x32x2_f32: exact fp32 products and sums).
// Everything is kept transposed so that the softmax axis lies inside a lane:
//   S^T[j][i] = sum_d K[j][d] Q[i][d]     row operand K (lane = key j), column operand Q (lane = query i)
//   -> accumulator: lane (i, hh) holds keys j = 8*(e>>2) + 4*hh + (e&3), e = 0..15: max / sum over e and the partner lane.
//   O^T[d][i] = sum_j V[j][d] P[i][j]     the reduction index runs over the keys in exactly the order the accumulator holds
//   them (step m <-> e = m), so P^T feeds the second MFMA without moving data; V is read as coalesced 128-byte rows.
// The backward needs P and dS with the roles of the lanes swapped (lane = key) for dK / dV: two 32x33 tiles per wave in LDS.
#ifndef ATT_BWD_BLOCKS_PER_CU
#define ATT_BWD_BLOCKS_PER_CU 3      /* 4 (128 registers, 22 spilled): 457 / 139 / 70 us vs 458 / 126 / 75 at hw = 1600 / 400 / 100: no gain */
#endif

// NT: the token count as a compile-time constant (24 frames: every temporal attention of the base models) or 0 = p.d.n_tok. With a
// constant n every row / key guard below folds (row groups are 8 rows, keys come in runs of 4 per lane half): the generic kernel spends
// 85 predicated regions and ~90 selects per item on them -- it is bound by instruction issue (~8 K cycles per item and SIMD), not by memory.
template <int NT>
__global__ __launch_bounds__(64 * AM_WAVES, 4) void attn_fwd_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ rcos,
                                                                          const float* __restrict__ rsin, const float* __restrict__ bias,
                                                                          float* __restrict__ out, AttnP p) {
  __shared__ __attribute__((aligned(16))) float tiles[AM_WAVES][2][32 * AM_TS];
  const int n = NT ? NT : p.d.n_tok;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  const bool tok = li < n;
  // planes of out for the to_out projection instead of the fp32 tensor (the MFMA backward does not read out): rows of P sum to 1,
  // so |out| <= max|v| <= max|qkv|
  float fps = 1.0f;
  if (p.pl_hi && p.pl_lo) {
    fps = scale_from_amax(amax_record_read(p.rec_qkv));
    if (blockIdx.x == 0 && threadIdx.x == 0) p.pl_scale[0] = fps;
  }
  float am = 0.f;
  float* Tq = tiles[wave][0];
  float* Tk = tiles[wave][1];
  for (int64_t item = (int64_t)blockIdx.x * AM_WAVES + wave; item < p.n_items; item += (int64_t)gridDim.x * AM_WAVES) {
    const AmItem w = am_item(p.d, item);
    const int h = w.h;
    const int64_t rowl = w.row0 + (int64_t)(tok ? li : 0) * p.d.st;
    const float* qb = am_uniform(qkv + w.row0 * p.RW + h * DH);          // q of token 0 of this item; k at + HD, v at + 2 HD
    const unsigned tstride = (unsigned)(p.d.st * p.RW);
    am_stage_rows(Tq, qb, tstride, rcos, rsin, p.scale, n, lane);
    am_stage_rows(Tk, qb + p.HD, tstride, rcos, rsin, 1.0f, n, lane);
    float va[16];
    am_col16(qb, tstride, 0, (unsigned)(2 * p.HD + li), n, hh, 1.0f, va);
    __builtin_amdgcn_wave_barrier();
    float qs[16], ks[16];
    am_sel(Tq, li, hh, qs);
    am_sel(Tk, li, hh, ks);
    f32x16 sT = am_mfma16(ks, qs, tf_zero());
    am_softmax(sT, bias ? bias + ((int64_t)h * n + (tok ? li : 0)) * n : nullptr, n, hh, tok);
    const f32x16 oT = am_mfma16(va, sT, tf_zero());
    if (tok) {      // (fp32 or planes: see am_store_row)
      float* orow = out + rowl * p.HD + h * DH;
      float4 vv[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        vv[e4] = am_quarter(oT, e4);
        if (!p.pl_hi) *reinterpret_cast<float4*>(orow + 8 * e4 + 4 * hh) = vv[e4];
        am = amax4(am, vv[e4]);
      }
      if (p.pl_hi) am_store_row_planes(p.pl_hi, p.pl_lo, rowl * p.HD + h * DH, hh, vv, fps);      // instead of out
    }
    __builtin_amdgcn_wave_barrier();      // the next item overwrites the tiles
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * AM_WAVES + wave);
}

// 32 < n_tok <= 64 (the super-resolution model attends over 48 frames): the same one-wave-per-(unit, head) formulation with keys and
// queries in two 32-wide tiles each. Q and K of all 64 rows are staged once ([64][AM_TS] per wave and operand); per query tile the two
// score tiles (32 MFMA steps), one softmax over both, and the two P V products into one accumulator (32 steps).
__global__ __launch_bounds__(64 * AM_WAVES, 2) void attn_fwd_mfma64_kernel(const float* __restrict__ qkv, const float* __restrict__ rcos,
                                                                            const float* __restrict__ rsin, const float* __restrict__ bias,
                                                                            float* __restrict__ out, AttnP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n = p.d.n_tok;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  float fps = 1.0f;                                  // (as in attn_fwd_mfma_kernel; a shared function costs this kernel 13 vector instructions)
  if (p.pl_hi && p.pl_lo) {
    fps = scale_from_amax(amax_record_read(p.rec_qkv));
    if (blockIdx.x == 0 && threadIdx.x == 0) p.pl_scale[0] = fps;
  }
  float am = 0.f;
  float* Tq = smem + wave * (2 * 64 * AM_TS);
  float* Tk = Tq + 64 * AM_TS;
  for (int64_t item = (int64_t)blockIdx.x * AM_WAVES + wave; item < p.n_items; item += (int64_t)gridDim.x * AM_WAVES) {
    const AmItem w = am_item(p.d, item);
    const int h = w.h;
    const int64_t row0 = w.row0;
    const float* qb = am_uniform(qkv + row0 * p.RW + h * DH);
    const unsigned tstride = (unsigned)(p.d.st * p.RW);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const float* rc = rcos ? rcos + half * 32 * DH : nullptr;
      const float* rs = rsin ? rsin + half * 32 * DH : nullptr;
      am_stage_rows(Tq + half * 32 * AM_TS, qb + (unsigned)(half * 32) * tstride, tstride, rc, rs, p.scale, n - half * 32, lane);
      am_stage_rows(Tk + half * 32 * AM_TS, qb + (unsigned)(half * 32) * tstride + p.HD, tstride, rc, rs, 1.0f, n - half * 32, lane);
    }
    // V elements of both key tiles: step m of tile jt needs V[32 jt + key(m, hh)][d = li]
    float va[2][16];      // (am_col16 per tile changes the address code of this kernel: 30 vector instructions)
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const int j = 32 * jt + tf_key(m, hh);
        va[jt][m] = j < n ? qb[(unsigned)j * tstride + (unsigned)(2 * p.HD + li)] : 0.f;
      }
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
      const int qi = 32 * it + li;                     // this lane's query
      const bool tok = qi < n;
      if (32 * it >= n) break;
      float qs[16];
      am_sel(Tq + it * 32 * AM_TS, li, hh, qs);
      f32x16 sT[2];
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        float ks[16];
        am_sel(Tk + jt * 32 * AM_TS, li, hh, ks);
        sT[jt] = am_mfma16(ks, qs, tf_zero());
      }
      // softmax over the 64 keys of query qi: 32 in this lane (two tiles x 16), 32 in lane ^ 32; 1 / sum applied at the operand.
      // The masked maximum stays inline: as am_masked_max over two tiles the bias adds compile to 170 more vector instructions.
      const float* brow = bias ? bias + ((int64_t)h * n + (tok ? qi : 0)) * n : nullptr;
      float mx = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = 32 * jt + tf_key(e, hh);
          float v = sT[jt][e];
          if (brow && tok && j < n) v += brow[j];
          v = j < n ? v : -INFINITY;
          sT[jt][e] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float inv = 1.0f / am_exp_sum<2>(sT, mx);
      f32x16 oT = tf_zero();
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int m = 0; m < 16; ++m) oT = __builtin_amdgcn_mfma_f32_32x32x2f32(va[jt][m], sT[jt][m] * inv, oT, 0, 0, 0);
      // both lanes of a pair (l, l + 32) hold the same query, so `tok` is uniform over the pair (am_store_row_planes needs that)
      if (tok) {      // (fp32 or planes: see am_store_row)
        const int64_t rowl = row0 + (int64_t)qi * p.d.st;
        float* orow = out + rowl * p.HD + h * DH;
        float4 vv[4];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          vv[e4] = am_quarter(oT, e4);
          if (!p.pl_hi) *reinterpret_cast<float4*>(orow + 8 * e4 + 4 * hh) = vv[e4];
          am = amax4(am, vv[e4]);
        }
        if (p.pl_hi) am_store_row_planes(p.pl_hi, p.pl_lo, rowl * p.HD + h * DH, hh, vv, fps);
      }
    }
    __builtin_amdgcn_wave_barrier();      // the next item overwrites the tiles
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * AM_WAVES + wave);
}

// n_tok > 64 without rotation and bias (the mid spatial attention: 100 tokens at the bench size, 400 in the super-resolution model): one wave
// per (unit, head, tile of 32 queries), the keys walked in tiles of 32 with an online softmax -- the thread-per-row kernel took 89 us for the
// 768 items of a sampling step and 614 us for the super-resolution model's 384 items of 400 tokens. No LDS: every operand of the two exact-fp32
// products of a tile is loaded straight into the accumulator layout -- a lane owns one token and the feature runs 8 c + 4 hh + (0..3), which is
// what S^T = K Q^T wants of q and k (four 16-byte loads of the token's row each), and v column d = li of the 16 keys of its lane half (coalesced
// 128-byte rows); P^T feeds O^T += V^T P^T in place; the running maximum and sum of a query live in its lane pair.
__global__ __launch_bounds__(64 * AM_WAVES, 3) void attn_fwd_mfma_tiled_kernel(const float* __restrict__ qkv, float* __restrict__ out, AttnP p) {
  const int n = p.d.n_tok, ntile = (n + 31) >> 5;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  const int64_t nwork = p.n_items * ntile;
  const unsigned tstride = (unsigned)(p.d.st * p.RW);
  float am = 0.f;
  for (int64_t wk = (int64_t)blockIdx.x * AM_WAVES + wave; wk < nwork; wk += (int64_t)gridDim.x * AM_WAVES) {
    const int64_t item = wk / ntile;
    const int it = (int)(wk - item * ntile);
    const AmItem w = am_item(p.d, item);
    const int h = w.h;
    const float* qb = am_uniform(qkv + w.row0 * p.RW + h * DH);          // q of token 0 of this item; k at + HD, v at + 2 HD
    const int qi = 32 * it + li;
    const bool tok = qi < n;
    float qs[16];
    am_row16(qb + (unsigned)qi * tstride, hh, tok, p.scale, qs);
    f32x16 oT = tf_zero();
    float m_run = -INFINITY, l_run = 0.f;
#pragma unroll 1
    for (int jt = 0; jt < ntile; ++jt) {
      const int kj = 32 * jt + li;
      float ks[16], va[16];
#pragma unroll
      for (int c = 0; c < 4; ++c) {      // (am_row16 with HD in the pointer: other address code, 10 vector instructions)
        const float4 v4 = kj < n ? *reinterpret_cast<const float4*>(qb + (unsigned)kj * tstride + (unsigned)(p.HD + 8 * c + 4 * hh)) : make_float4(0.f, 0.f, 0.f, 0.f);
        ks[4 * c] = v4.x; ks[4 * c + 1] = v4.y; ks[4 * c + 2] = v4.z; ks[4 * c + 3] = v4.w;
      }
      am_col16(qb, tstride, 32 * jt, (unsigned)(2 * p.HD + li), n, hh, 1.0f, va);
      f32x16 sT = am_mfma16(ks, qs, tf_zero());
      // the online update: the running maximum joins the tile's before the exponentials are taken
      const float mx = am_masked_max(sT, nullptr, 32 * jt, n, hh, tok);
      const float m_new = fmaxf(m_run, mx);                       // finite: every key tile holds at least one key
      const float corr = expf(m_run - m_new);                     // (0 for the first tile)
      l_run = l_run * corr + am_exp_sum<1>(&sT, m_new);
      m_run = m_new;
#pragma unroll
      for (int e = 0; e < 16; ++e) oT[e] *= corr;
      oT = am_mfma16(va, sT, oT);
    }
    if (tok) {
      const float inv = 1.0f / l_run;
#pragma unroll
      for (int e = 0; e < 16; ++e) oT[e] *= inv;
      am_store_row(oT, out + (w.row0 + (int64_t)qi * p.d.st) * p.HD + h * DH, hh, am);
    }
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * AM_WAVES + wave);
}

// The backward of the same case (n_tok > 64, no rotation, no bias), one block of four waves per (unit, head) item, nothing n x n stored and
// every product on the exact-fp32 matrix instruction with operands loaded straight into the layout the product wants (rows of q / k / v / dO as
// four 16-byte loads of a token's features, or column d = li of 16 tokens):
//   phase A, a wave per tile of 32 queries: pass 1 over the key tiles for the softmax statistics (m_i, 1 / l_i); delta_i = <dO_i, O_i>; pass 2:
//     S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T - delta), dQ^T += K^T dS^T (dS^T feeds the product in place); statistics to LDS;
//   phase B, a wave per tile of 32 keys, over the query tiles: S = Q K^T, dP = dO V^T, P and dS from the statistics, dV^T += dO^T P, dK^T += Q^T dS.
// The thread-per-row kernel (attn_bwd_big_kernel: 246 us for the 768 items of 100 tokens of a training step) remains for rotation / bias.
// STAGED (n <= 128, the training case): q (scaled), k, v, dO of the item are staged once in LDS tiles [128][36] and every operand is read from
// there (a global round trip per product stage of a tile left the matrix pipe idle: 107 us; staged: see DESIGN.md); larger n reads global memory.
#define ATT_TILED_MAXTOK 576
#define ATT_TILED_STAGE 128
#define ATT_TILED_TS 36
template <bool STAGED>
__global__ __launch_bounds__(64 * AM_WAVES, 2) void attn_bwd_mfma_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ fout,
                                                                                const float* __restrict__ dout, float* __restrict__ dqkv, AttnP p) {
  __shared__ __attribute__((aligned(16))) float Ms[STAGED ? ATT_TILED_STAGE : ATT_TILED_MAXTOK], Ls[STAGED ? ATT_TILED_STAGE : ATT_TILED_MAXTOK],
      Dl[STAGED ? ATT_TILED_STAGE : ATT_TILED_MAXTOK];
  __shared__ __attribute__((aligned(16))) float Stg[STAGED ? 4 * ATT_TILED_STAGE * ATT_TILED_TS : 4];      // q | k | v | dO
  const int n = p.d.n_tok, ntile = (n + 31) >> 5;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  const unsigned tq = (unsigned)(p.d.st * p.RW), to = (unsigned)(p.d.st * p.HD);
  float am = 0.f;
  for (int64_t item = blockIdx.x; item < p.n_items; item += gridDim.x) {
    const AmItem w = am_item(p.d, item);
    const int h = w.h;
    const int64_t row0 = w.row0;
    const float* qb = am_uniform(qkv + row0 * p.RW + h * DH);           // q of token 0; k at + HD, v at + 2 HD
    const float* gb = am_uniform(dout + row0 * p.HD + h * DH);
    const float* ob = am_uniform(fout + row0 * p.HD + h * DH);
    float* db = dqkv + row0 * p.RW + h * DH;
    // row `t` of a [token][feature] operand as the 16 values (features 8 c + 4 hh + 0..3) a lane feeds to a product over the features
    // (STAGED: `base` is matched to its LDS tile -- q, k, v at column offsets 0, HD, 2 HD of qkv; dO -- and rows beyond n hold zeros)
    auto tile_of = [&](const float* base, unsigned col0) -> const float* {
      return Stg + (base == gb ? 3 : col0 == 0 ? 0 : col0 == (unsigned)p.HD ? 1 : 2) * (ATT_TILED_STAGE * ATT_TILED_TS);
    };
    auto row16 = [&](const float* base, unsigned stride, int t, unsigned col0, float mul, float (&v)[16]) {
      if (STAGED) {
        am_row16(tile_of(base, col0) + t * ATT_TILED_TS, hh, true, 1.0f, v);
        return;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 v4 = t < n ? *reinterpret_cast<const float4*>(base + (unsigned)t * stride + col0 + 8 * c + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[4 * c] = v4.x * mul; v[4 * c + 1] = v4.y * mul; v[4 * c + 2] = v4.z * mul; v[4 * c + 3] = v4.w * mul;
      }
    };
    // column d = li of the 16 tokens t0 + tf_key(m, hh): what a lane feeds to a product over the tokens
    auto col16 = [&](const float* base, unsigned stride, int t0, unsigned col0, float mul, float (&v)[16]) {
      if (STAGED) {
        const float* T = tile_of(base, col0) + t0 * ATT_TILED_TS + li;
#pragma unroll
        for (int m = 0; m < 16; ++m) v[m] = T[tf_key(m, hh) * ATT_TILED_TS];
        return;
      }
      am_col16(base, stride, t0, col0 + li, n, hh, mul, v);
    };
    __syncthreads();                                  // the previous item's phase B has finished with the statistics (and the tiles)
    if (STAGED) {                                     // 4 tiles x 128 rows x 8 chunks of 16 bytes; q scaled here; rows beyond n zero
      for (int i = threadIdx.x; i < 4 * ATT_TILED_STAGE * 8; i += 64 * AM_WAVES) {
        const int tl = i >> 10, r = (i >> 3) & (ATT_TILED_STAGE - 1), ch = i & 7;
        float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) v4 = tl < 3 ? *reinterpret_cast<const float4*>(qb + (unsigned)r * tq + (unsigned)(tl * p.HD + 4 * ch)) : *reinterpret_cast<const float4*>(gb + (unsigned)r * to + 4 * ch);
        if (tl == 0) { v4.x *= p.scale; v4.y *= p.scale; v4.z *= p.scale; v4.w *= p.scale; }
        *reinterpret_cast<float4*>(Stg + (tl * ATT_TILED_STAGE + r) * ATT_TILED_TS + 4 * ch) = v4;
      }
      __syncthreads();
    }
    // ------------------------------------------------------------------ phase A
#pragma unroll 1
    for (int it = wave; it < ntile; it += AM_WAVES) {
      const int qi = 32 * it + li;
      float qs[16], gs[16];
      row16(qb, tq, qi, 0, p.scale, qs);
      row16(gb, to, qi, 0, 1.0f, gs);
      float delta = 0.f;
      {
#pragma unroll
        for (int c = 0; c < 4; ++c) {                 // (the forward output: always from global memory)
          const float4 o4 = qi < n ? *reinterpret_cast<const float4*>(ob + (unsigned)qi * to + 8 * c + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
          delta = fmaf(gs[4 * c], o4.x, delta); delta = fmaf(gs[4 * c + 1], o4.y, delta);
          delta = fmaf(gs[4 * c + 2], o4.z, delta); delta = fmaf(gs[4 * c + 3], o4.w, delta);
        }
        delta += __shfl_xor(delta, 32);
      }
      float m_run = -INFINITY, l_run = 0.f;
#pragma unroll 1
      for (int jt = 0; jt < ntile; ++jt) {
        float ks[16];
        row16(qb, tq, 32 * jt + li, p.HD, 1.0f, ks);
        f32x16 sT = tf_zero();
#pragma unroll
        for (int m = 0; m < 16; ++m) sT = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[m], qs[m], sT, 0, 0, 0);
        const float mx = am_masked_max(sT, nullptr, 32 * jt, n, hh, true);
        const float m_new = fmaxf(m_run, mx);
        float l = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) l += expf(sT[e] - m_new);
        l += __shfl_xor(l, 32);
        l_run = l_run * expf(m_run - m_new) + l;
        m_run = m_new;
      }
      const float inv_l = 1.0f / l_run;
      f32x16 dqT = tf_zero();
#pragma unroll 1
      for (int jt = 0; jt < ntile; ++jt) {
        f32x16 sT = tf_zero(), dpT = tf_zero();
        {
          float ks[16], vs[16];
          row16(qb, tq, 32 * jt + li, p.HD, 1.0f, ks);
          row16(qb, tq, 32 * jt + li, 2 * p.HD, 1.0f, vs);
#pragma unroll
          for (int m = 0; m < 16; ++m) sT = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[m], qs[m], sT, 0, 0, 0);
#pragma unroll
          for (int m = 0; m < 16; ++m) dpT = __builtin_amdgcn_mfma_f32_32x32x2f32(vs[m], gs[m], dpT, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pe = 32 * jt + tf_key(e, hh) < n ? expf(sT[e] - m_run) * inv_l : 0.f;
          sT[e] = pe * (dpT[e] - delta);              // dS^T
        }
        __builtin_amdgcn_sched_barrier(0);
        {
          float kc[16];
          col16(qb, tq, 32 * jt, p.HD, 1.0f, kc);
          dqT = am_mfma16(kc, sT, dqT);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (qi < n) {
#pragma unroll
        for (int e = 0; e < 16; ++e) dqT[e] *= p.scale;
        am_store_row(dqT, db + (unsigned)qi * tq, hh, am);
        if (hh == 0) { Ms[qi] = m_run; Ls[qi] = inv_l; Dl[qi] = delta; }
      }
    }
    __syncthreads();
    // ------------------------------------------------------------------ phase B
#pragma unroll 1
    for (int jt = wave; jt < ntile; jt += AM_WAVES) {
      const int kj = 32 * jt + li;
      float kb[16], vb[16];
      row16(qb, tq, kj, p.HD, 1.0f, kb);
      row16(qb, tq, kj, 2 * p.HD, 1.0f, vb);
      f32x16 dkT = tf_zero(), dvT = tf_zero();
#pragma unroll 1
      for (int it = 0; it < ntile; ++it) {
        f32x16 S = tf_zero(), dP = tf_zero();
        {
          float qa[16], ga[16];
          row16(qb, tq, 32 * it + li, 0, p.scale, qa);
          row16(gb, to, 32 * it + li, 0, 1.0f, ga);
#pragma unroll
          for (int m = 0; m < 16; ++m) S = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m], kb[m], S, 0, 0, 0);
#pragma unroll
          for (int m = 0; m < 16; ++m) dP = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[m], vb[m], dP, 0, 0, 0);
        }
        // rows of S are the queries 32 it + 8 c + 4 hh + (0..3): their statistics, four at a time
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int r0 = 32 * it + 8 * c + 4 * hh;
          float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), l4 = m4, d4 = m4;
          if (r0 < n) {                                // (n is a multiple of 4 or the tail rows read statistics nobody wrote: masked below)
            m4 = *reinterpret_cast<const float4*>(Ms + r0); l4 = *reinterpret_cast<const float4*>(Ls + r0); d4 = *reinterpret_cast<const float4*>(Dl + r0);
          }
          const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ll[4] = {l4.x, l4.y, l4.z, l4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int e = 4 * c + j;
            const float pe = r0 + j < n ? expf(S[e] - mm[j]) * ll[j] : 0.f;
            S[e] = pe;                                 // P
            dP[e] = pe * (dP[e] - dd[j]);              // dS
          }
        }
        __builtin_amdgcn_sched_barrier(0);             // (the column loads stay behind the row operands: registers)
        {
          float gc[16];
          col16(gb, to, 32 * it, 0, 1.0f, gc);
#pragma unroll
          for (int m = 0; m < 16; ++m) dvT = __builtin_amdgcn_mfma_f32_32x32x2f32(gc[m], S[m], dvT, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
          float qc[16];
          col16(qb, tq, 32 * it, 0, p.scale, qc);
#pragma unroll
          for (int m = 0; m < 16; ++m) dkT = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[m], dP[m], dkT, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (kj < n) {
        float* dr = db + (unsigned)kj * tq;
        am_store_row(dkT, dr + p.HD, hh, am);
        am_store_row(dvT, dr + 2 * p.HD, hh, am);
      }
    }
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * AM_WAVES + wave);
}


template <int NT>
__global__ __launch_bounds__(64 * AM_WAVES, ATT_BWD_BLOCKS_PER_CU) void attn_bwd_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ rcos,
                                                                       const float* __restrict__ rsin, const float* __restrict__ bias,
                                                                       const float* __restrict__ fout, const float* __restrict__ dout,
                                                                       float* __restrict__ dqkv, float* __restrict__ dbias, AttnP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n = NT ? NT : p.d.n_tok;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, hh = lane >> 5;
  constexpr int WAVE_LDS = 2 * 32 * AM_TS + 32;
  float* Ta = smem + wave * WAVE_LDS;                // two staged operand tiles (q, k then v, dO), then P^T / dS^T ([j][i]) in the same
  float* Tb = Ta + 32 * AM_TS;                       // storage once the staged operands have been consumed; delta[32]
  float* dl = Tb + 32 * AM_TS;
  float* Pt = Ta;
  float* St = Tb;
  float* dBs = smem + AM_WAVES * WAVE_LDS;            // [heads][n][n] when dbias
  // Relative-position-bias gradient = sum of dS over the units. With heads == AM_WAVES a wave always works on the head `wave`
  // (item = 4 (block + k grid) + wave), so it sums its items' dS tiles in REGISTERS, in item order; otherwise in LDS. With heads a multiple
  // of AM_WAVES the four waves of a block never hold the same head, so each (head, i, j) has ONE writer, which adds its items in order.
  // With any other head count two waves can meet on a head, and the order of their additions would differ from run to run: there
  // (p.db_slices) every wave owns a partial [heads][n][n] of its own and the block adds the four in wave order at the end.
  const bool db_regs = dbias && p.d.heads == AM_WAVES;
  float* dBw = dBs + (p.db_slices ? (size_t)wave * p.d.heads * n * n : 0);
  f32x16 dbacc = tf_zero();
  if (dbias && !db_regs) {
    for (int e = threadIdx.x; e < (p.db_slices ? AM_WAVES : 1) * p.d.heads * n * n; e += 64 * AM_WAVES) dBs[e] = 0.f;
    __syncthreads();
  }
  const bool tok = li < n;
  float am = 0.f;                                    // max |dqkv| this lane has stored
  // Planes output: with A = max|qkv|, G = max|dout|, P row sums 1:  |dV| <= n G;  |dP| <= 32 G A;  sum_j |dS_ij| <= 2 * 32 G A and
  // sum_i |dS_ij| <= n * that;  |dK| <= sqrt2 * scale * n * 64 G A^2 (the rotation keeps pair norms), |dQ| the same without n.
  // A bound this loose (2^10 and more above the true maximum) still leaves the planes ~2^-28 max|dqkv| accurate: DESIGN.md.
  float ps = 1.0f;
  if (p.pl_hi && p.pl_lo) {
    const float A = amax_record_read(p.rec_qkv), G = amax_record_read(p.rec_dout);
    ps = scale_from_amax(1.01f * fmaxf((float)n * G, 1.4143f * p.scale * (float)n * 64.f * G * A * A));
    if (blockIdx.x == 0 && threadIdx.x == 0) p.pl_scale[0] = ps;
  }
  for (int64_t item = (int64_t)blockIdx.x * AM_WAVES + wave; item < p.n_items; item += (int64_t)gridDim.x * AM_WAVES) {
    const AmItem w = am_item(p.d, item);
    const int h = w.h;
    const int64_t row0 = w.row0;
    const float* qb = am_uniform(qkv + row0 * p.RW + h * DH);          // q of token 0 of this item; k at + HD, v at + 2 HD
    const float* gb = am_uniform(dout + row0 * p.HD + h * DH);
    const float* fb = am_uniform(fout + row0 * p.HD + h * DH);
    float* db = const_cast<float*>(am_uniform(dqkv + row0 * p.RW + h * DH));
    const int64_t pbase = row0 * p.RW + h * DH;                        // the same element offset inside the planes
    const unsigned lrow = (unsigned)(tok ? li : 0);
    // key / query index of step m for this lane = 8*(m>>2) + (m&3) + hz with hz = 4*hh, made opaque per item: otherwise the
    // compiler hoists all 48 per-lane row offsets (as 64-bit pairs) out of the item loop and the kernel needs 270 registers
    unsigned hz = 4u * (unsigned)hh;
    asm volatile("" : "+v"(hz));
    const unsigned tstride = (unsigned)(p.d.st * p.RW), gstride = (unsigned)(p.d.st * p.HD);
    f32x16 pT, dsT;
    // Phase order (round 2): V / dO first, Q / K second, so that the scaled + rotated Q and K tiles are still in LDS when the dQ and dK
    // products need their columns. Round 1 staged Q / K first and re-read K, Q and dO column-wise from global memory for the three
    // gradient products, re-applying the rotation per element (two table loads each); now only dO is re-read. Still two tiles per wave.
    {
      // dP^T[j][i] = sum_d V[j][d] dO[i][d]
      am_stage_rows(Ta, qb + 2 * p.HD, tstride, nullptr, nullptr, 1.0f, n, lane);
      am_stage_rows(Tb, gb, gstride, nullptr, nullptr, 1.0f, n, lane);
      __builtin_amdgcn_wave_barrier();
      dsT = tf_zero();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {          // four steps at a time: bounded live registers (the kernel runs at 128 VGPRs)
        float va[4], gg[4];
        am_sel4(Ta, li, hh, g4, va);
        am_sel4(Tb, li, hh, g4, gg);
        dsT = am_mfma4(va, gg, dsT);
      }
    }
    {
      __builtin_amdgcn_wave_barrier();                 // every lane has taken its V / dO values: the tiles may be overwritten
      am_stage_rows<2>(Ta, qb, tstride, rcos, rsin, p.scale, n, lane);
      am_stage_rows<2>(Tb, qb + p.HD, tstride, rcos, rsin, 1.0f, n, lane);
      __builtin_amdgcn_wave_barrier();
      pT = tf_zero();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float qa[4], kb[4];
        am_sel4(Ta, li, hh, g4, qa);
        am_sel4(Tb, li, hh, g4, kb);
        pT = am_mfma4(kb, qa, pT);
      }
      am_softmax(pT, bias ? bias + ((int64_t)h * n + (tok ? li : 0)) * n : nullptr, n, hh, tok);
      // delta_i = <dO_i, O_i> = sum_j P_ij dP_ij: both factors are in this lane's accumulators (16 keys here, 16 in lane ^ 32; masked
      // keys have P = 0) -- the forward output is not read at all (round 1 re-read it: 157 MB per level-0 launch)
      float delta = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) delta = fmaf(pT[e], dsT[e], delta);
      delta += __shfl_xor(delta, 32);
#pragma unroll
      for (int e = 0; e < 16; ++e) dsT[e] = pT[e] * (dsT[e] - delta);
    }
    // dQ^T[d][i] = sum_j K[j][d] dS^T[j][i]: K columns from the staged (rotated) tile, dS^T straight from the accumulator
    {
      f32x16 acc = tf_zero();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float ka[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = 4 * g4 + q;
          const unsigned j = (unsigned)(8 * (m >> 2) + (m & 3)) + hz;
          ka[q] = Tb[j * AM_TS + (unsigned)li];        // rows >= n are zero-filled by the staging
        }
        const float dg[4] = {dsT[4 * g4], dsT[4 * g4 + 1], dsT[4 * g4 + 2], dsT[4 * g4 + 3]};
        acc = am_mfma4(ka, dg, acc);
      }
      if (tok) {
        float* drow = db + lrow * tstride;
        float4 gqv[4];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int d0 = 8 * e4 + 4 * hh;
          float4 gq = am_unrotate4(make_float4(acc[4 * e4], acc[4 * e4 + 1], acc[4 * e4 + 2], acc[4 * e4 + 3]), rcos ? rcos + li * DH : nullptr, rsin ? rsin + li * DH : nullptr, d0);
          gq = make_float4(gq.x * p.scale, gq.y * p.scale, gq.z * p.scale, gq.w * p.scale);
          gqv[e4] = gq;
          if (!p.pl_hi) *reinterpret_cast<float4*>(drow + d0) = gq;
          am = amax4(am, gq);
        }
        if (p.pl_hi) am_store_row_planes(p.pl_hi, p.pl_lo, pbase + (int64_t)(lrow * tstride), hh, gqv, ps);
      }
    }
    // dS with the lane roles swapped (lane = key) goes through LDS, over the K tile every lane has finished with; the
    // relative-position-bias gradient is dS itself
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = tf_key(e, hh);
      St[j * AM_TS + li] = dsT[e];
      if (db_regs) dbacc[e] += dsT[e];                 // entries with li >= n or j >= n are never written out
      else if (dbias && tok && j < n) atomicAdd(&dBw[(h * n + li) * n + j], dsT[e]);      // (one writer per address: see above)
    }
    __builtin_amdgcn_wave_barrier();
    // dK^T[d][j] = sum_i Q[i][d] dS[i][j]: Q columns from the staged (scaled, rotated) tile
    {
      f32x16 dk = tf_zero();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float qa[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = 4 * g4 + q;
          const unsigned i = (unsigned)(8 * (m >> 2) + (m & 3)) + hz;
          qa[q] = Ta[i * AM_TS + (unsigned)li];
        }
        // this lane's row of dS, four consecutive queries as ONE 16-byte read (four ds_read_b32 at a row stride of 36 floats were 2-way
        // bank-conflicted: 36 li mod 64 takes 16 values for 32 lanes)
        const float4 sb4 = *reinterpret_cast<const float4*>(St + li * AM_TS + 8 * g4 + hz);
        const float sb[4] = {sb4.x, sb4.y, sb4.z, sb4.w};
        dk = am_mfma4(qa, sb, dk);
      }
      if (tok) {
        float* drow = db + (lrow * tstride + (unsigned)p.HD);
        float4 gkv[4];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int d0 = 8 * e4 + 4 * hh;
          const float4 gk = am_unrotate4(make_float4(dk[4 * e4], dk[4 * e4 + 1], dk[4 * e4 + 2], dk[4 * e4 + 3]), rcos ? rcos + li * DH : nullptr, rsin ? rsin + li * DH : nullptr, d0);
          gkv[e4] = gk;
          if (!p.pl_hi) *reinterpret_cast<float4*>(drow + d0) = gk;
          am = amax4(am, gk);
        }
        if (p.pl_hi) am_store_row_planes(p.pl_hi, p.pl_lo, pbase + (int64_t)(lrow * tstride + (unsigned)p.HD), hh, gkv, ps);
      }
    }
    // P with the lane roles swapped, over the Q tile; dV^T[d][j] = sum_i dO[i][d] P[i][j] (dO columns are the one global re-read left)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < 16; ++e) Pt[tf_key(e, hh) * AM_TS + li] = pT[e];
    __builtin_amdgcn_wave_barrier();
    {
      f32x16 dv = tf_zero();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float ga[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = 4 * g4 + q;
          const unsigned i = (unsigned)(8 * (m >> 2) + (m & 3)) + hz;
          ga[q] = i < (unsigned)n ? gb[i * gstride + (unsigned)li] : 0.f;
        }
        const float4 pb4 = *reinterpret_cast<const float4*>(Pt + li * AM_TS + 8 * g4 + hz);
        const float pb[4] = {pb4.x, pb4.y, pb4.z, pb4.w};
        dv = am_mfma4(ga, pb, dv);
      }
      if (tok) {
        float* drow = db + (lrow * tstride + (unsigned)(2 * p.HD));
        float4 gvv[4];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const float4 gv = make_float4(dv[4 * e4], dv[4 * e4 + 1], dv[4 * e4 + 2], dv[4 * e4 + 3]);
          gvv[e4] = gv;
          if (!p.pl_hi) *reinterpret_cast<float4*>(drow + 8 * e4 + 4 * hh) = gv;
          am = amax4(am, gv);
        }
        if (p.pl_hi) am_store_row_planes(p.pl_hi, p.pl_lo, pbase + (int64_t)(lrow * tstride + (unsigned)(2 * p.HD)), hh, gvv, ps);
      }
    }
    __builtin_amdgcn_wave_barrier();      // the next item overwrites this wave's tiles
  }
  if (p.amax_rec) wave_amax_emit(am, p.amax_rec, (int)blockIdx.x * AM_WAVES + wave);
  if (dbias) {         // dbias: this block's partial [heads][n][n]; attn_dbias_reduce_kernel sums the blocks in index order
    float* part = dbias + (size_t)blockIdx.x * p.d.heads * n * n;
    if (db_regs) {
      if (tok) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = tf_key(e, hh);
          if (j < n) part[(wave * n + li) * n + j] = dbacc[e];
        }
      }
    } else {
      __syncthreads();
      const int E = p.d.heads * n * n;
      for (int e = threadIdx.x; e < E; e += 64 * AM_WAVES) part[e] = p.db_slices ? (dBs[e] + dBs[E + e]) + (dBs[2 * E + e] + dBs[3 * E + e]) : dBs[e];
    }
  }
}

#define ATT_MFMA64_LDS ((size_t)AM_WAVES * 2 * 64 * AM_TS * sizeof(float))       // 73.7 KB: two blocks per CU
#define ATT_MFMA64_MAXBLOCKS 4096
#define ATT_ROWS_MAXLDS (160 * 1024)
static void attn_fwd_mfma64_launch(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out,
                                   const AttnP& p, int nb, hipStream_t st) {
  static bool done = false;      // once per process
  if (!done) { am_dyn_lds((const void*)attn_fwd_mfma64_kernel, ATT_MFMA64_LDS); done = true; }
  attn_fwd_mfma64_kernel<<<(unsigned)nb, 64 * AM_WAVES, ATT_MFMA64_LDS, st>>>(qkv, rot_cos, rot_sin, bias, out, p);
}
// Grid of the one-wave-per-item kernels: exactly the blocks that are RESIDENT together (blocks per CU x CUs), each wave walking over
// its items with a grid stride. The first versions launched up to 4096 / 2048 blocks: several rounds of the resident set with the last
// one partly empty (2048 blocks on 768 slots = 2.67 rounds), and waves with 3 or 4 items each (a 28 % imbalance at the 40 x 40
// level); with 768 / 1024 blocks every wave gets 12-17 items, i.e. at most one item of imbalance.
static int64_t attn_grid(int64_t items, int blocks_per_cu) {
  int64_t nb = (items + AM_WAVES - 1) / AM_WAVES;
  const int64_t cap = (int64_t)blocks_per_cu * wdno_num_cus();
  return nb > cap ? cap : nb;
}
static int attn_fill(AttnP& p, const wdno_attn_desc* d, float scale, int threads) {
  if (!d || d->n_uo <= 0 || d->n_ui <= 0 || d->n_tok <= 0 || d->heads <= 0) return WDNO_EINVAL;
  p.d = *d; p.scale = scale; p.HD = d->heads * DH; p.RW = 3 * p.HD;
  p.ipb = threads / d->n_tok;
  if (p.ipb < 1) p.ipb = 1;
  p.kst = d->n_tok * DH + 8;          // +8 floats: items start on different 32-byte LDS slots
  p.n_items = (int64_t)d->n_uo * d->n_ui * d->heads;
  p.amax_rec = nullptr; p.db_slices = 0;
  p.pl_hi = p.pl_lo = nullptr; p.rec_qkv = p.rec_dout = nullptr; p.pl_scale = nullptr;
  return WDNO_OK;
}

// ---- what a call launches: the ONE place that decides it (the launch paths below and the plan queries of wdno_hip.h both ask here)
static int attn_plan_refuse(wdno_attn_plan& pl, int rc) {
  pl = wdno_attn_plan{WDNO_ATTN_NONE, 0, 0, 0, 0, 0, 0, rc};
  return rc;
}
static void attn_plan_set(wdno_attn_plan& pl, int family, int64_t grid, int ipb, int64_t work, size_t lds) {
  pl = wdno_attn_plan{family, (int)grid, ipb, (int)cdiv64(work, grid * ipb), 0, 0, (int)lds, WDNO_OK};
}
static int attn_mfma_family(int n) { return n == 24 && wdno_debug_mode != WDNO_DBG_ATTN_GENERIC_NTOK ? WDNO_ATTN_MFMA24 : WDNO_ATTN_MFMA; }
static int attn_fwd_choose(const wdno_attn_desc* d, bool rot, bool bias, bool planes, wdno_attn_plan& pl) {
  if (!d || d->n_uo <= 0 || d->n_ui <= 0 || d->n_tok <= 0 || d->heads <= 0) return attn_plan_refuse(pl, WDNO_EINVAL);
  const int n = d->n_tok;
  const int64_t items = (int64_t)d->n_uo * d->n_ui * d->heads;
  const bool rows_mode = wdno_debug_mode == WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV;
  if (planes ? n > 64 : n > 1024) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
  if (n <= 32 && (planes || !rows_mode)) {                       // one 32x32 MFMA tile per (unit, head): one wave per item
    attn_plan_set(pl, attn_mfma_family(n), attn_grid(items, 4), AM_WAVES, items, 0);
    return WDNO_OK;
  }
  if (n <= 64 && (planes || !rows_mode)) {                       // two 32-wide tiles of keys and of queries per item
    int64_t nb = cdiv64(items, AM_WAVES);
    if (nb > ATT_MFMA64_MAXBLOCKS) nb = ATT_MFMA64_MAXBLOCKS;
    attn_plan_set(pl, WDNO_ATTN_MFMA64, nb, AM_WAVES, items, ATT_MFMA64_LDS);
    return WDNO_OK;
  }
  if (!rot && !bias && !rows_mode && wdno_debug_mode != WDNO_DBG_ATTN_FWD_ROWS) {      // key tiles with an online softmax, one wave per tile of 32 queries (WDNO_DBG_ATTN_FWD_ROWS: thread per row)
    const int64_t work = items * ((n + 31) / 32);
    attn_plan_set(pl, WDNO_ATTN_TILED, attn_grid(work, 3), AM_WAVES, work, 0);
    return WDNO_OK;
  }
  int ipb = ATT_THREADS / n;
  if (ipb < 1) ipb = 1;
  const size_t lds = (size_t)ipb * (n * DH + 8) * sizeof(float);
  const int64_t blocks = cdiv64(items, ipb);
  if (lds > ATT_ROWS_MAXLDS || blocks > 0x7fffffff) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
  attn_plan_set(pl, WDNO_ATTN_ROWS, blocks, ipb, items, lds);
  return WDNO_OK;
}
// LDS floats of the thread-per-row backward: K, Q, P, dS per item slot and the block's bias-gradient partial
static size_t attn_bwd_rows_lds(int n, int heads, int ipb, bool dbias) {
  return ((size_t)ipb * (2 * (n * DH + 8) + 2 * n * (n + 1)) + (dbias ? (size_t)heads * n * n : 0)) * sizeof(float);
}
static int attn_bwd_choose(const wdno_attn_desc* d, bool rot, bool bias, bool dbias, bool planes, bool has_out, wdno_attn_plan& pl) {
  if (!d || d->n_uo <= 0 || d->n_ui <= 0 || d->n_tok <= 0 || d->heads <= 0) return attn_plan_refuse(pl, WDNO_EINVAL);
  const int n = d->n_tok;
  const int64_t items = (int64_t)d->n_uo * d->n_ui * d->heads;
  const bool rows_mode = wdno_debug_mode == WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV;
  if (planes && (n > 32 || rows_mode)) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
  // one wave per item on MFMA tiles (WDNO_DBG_ROW_ATTN_AND_REG_STAGED_CONV: thread-per-row kernel below); 116 registers and 9 KB of LDS per wave, so four
  // waves per SIMD hide its five dependent load phases (0.94 vs 1.17 ms at the 40 x 40 level)
  if (n <= 32 && !rows_mode) {
    const bool in_lds = dbias && d->heads != AM_WAVES;            // (heads == AM_WAVES: the partial lives in registers)
    const size_t base = (size_t)AM_WAVES * (2 * 32 * AM_TS + 32) * sizeof(float), one = (size_t)d->heads * n * n * sizeof(float);
    // heads % AM_WAVES != 0: a partial per wave, so that no two waves add to one address (attn_bwd_mfma_kernel); one shared partial where four do not fit
    // (from 9 heads on at 32 tokens: two waves of a block then add to one address in arrival order, reported as dbias_in_lds = 2)
    const bool per_wave = in_lds && d->heads % AM_WAVES != 0 && base + AM_WAVES * one <= ATT_ROWS_MAXLDS;
    const int arrays = !in_lds ? 0 : (per_wave ? AM_WAVES : 1);
    if (base + arrays * one > ATT_ROWS_MAXLDS) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
    attn_plan_set(pl, attn_mfma_family(n), attn_grid(items, ATT_BWD_BLOCKS_PER_CU), AM_WAVES, items, base + arrays * one);
    pl.dbias_partials = dbias ? pl.grid : 0;
    pl.dbias_in_lds = !in_lds ? 0 : (per_wave ? AM_WAVES : (d->heads % AM_WAVES == 0 ? 1 : 2));
    return WDNO_OK;
  }
  // more than 64 tokens without rotation / bias (the mid spatial block): key / query tiles on the exact-fp32 matrix instruction (WDNO_DBG_ATTN_BWD_ROWS: thread per row)
  if (n > 64 && n <= ATT_TILED_MAXTOK && !rot && !bias && !dbias && has_out && !rows_mode && wdno_debug_mode != WDNO_DBG_ATTN_BWD_ROWS) {
    const int64_t cap = 2LL * wdno_num_cus();
    attn_plan_set(pl, n <= ATT_TILED_STAGE ? WDNO_ATTN_TILED_STAGED : WDNO_ATTN_TILED_UNSTAGED, items > cap ? cap : items, 1, items, 0);
    return WDNO_OK;
  }
  // 129 .. 576 tokens: nothing n x n is stored (attn_bwd_big_kernel) -- and 64 .. 128 tokens too when the kernel takes the case (no rotation, no bias):
  // the thread-per-row kernel keeps P and dS (2 n^2 floats: 81 KB at the mid block's 100 tokens) in LDS, one block per CU; 27 KB and five blocks per CU
  // here: 305 -> 246 us for the mid spatial attention of the smoke U-Net
  if (n > ATT_BWD_THREADS || (n >= 64 && !rot && !bias && !dbias)) {
    if (n > ATT_BIG_MAXTOK || rot || bias || dbias) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
    const int64_t cap = 4LL * wdno_num_cus();
    attn_plan_set(pl, WDNO_ATTN_BIG, items > cap ? cap : items, 1, items, ((size_t)2 * n * DH + 3 * n) * sizeof(float));
    return WDNO_OK;
  }
  // thread per row: 128 / n items per block, fewer where their matrices and the bias-gradient partial do not fit the 160 KB of LDS together
  // (64 tokens, 4 heads, a bias gradient: 164 992 bytes at two items, 115 264 at one)
  int ipb = ATT_BWD_THREADS / n;
  if (ipb < 1) ipb = 1;
  if (dbias && ipb > d->heads) ipb = d->heads;             // the items of a block hold different heads: one writer per address of the partial, in item order
  while (ipb > 1 && attn_bwd_rows_lds(n, d->heads, ipb, dbias) > ATT_ROWS_MAXLDS) --ipb;
  const size_t lds = attn_bwd_rows_lds(n, d->heads, ipb, dbias);
  if (lds > ATT_ROWS_MAXLDS) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
  const int64_t groups = cdiv64(items, ipb);
  int64_t blocks = groups;
  if (dbias && blocks > 1024) blocks = 1024;               // one dbias partial per block (grid-stride over the groups)
  if (blocks > 0x7fffffff) return attn_plan_refuse(pl, WDNO_EUNSUPPORTED);
  attn_plan_set(pl, WDNO_ATTN_ROWS, blocks, ipb, items, lds);
  pl.dbias_partials = dbias ? pl.grid : 0;
  pl.dbias_in_lds = dbias;
  return WDNO_OK;
}
extern "C" int wdno_attn_fwd_plan(const wdno_attn_desc* d, int has_rot, int has_bias, int want_dbias, int planes, wdno_attn_plan* out) {
  (void)want_dbias;
  if (!out) return WDNO_EINVAL;
  attn_fwd_choose(d, has_rot != 0, has_bias != 0, planes != 0, *out);
  return WDNO_OK;
}
extern "C" int wdno_attn_bwd_plan(const wdno_attn_desc* d, int has_rot, int has_bias, int want_dbias, int planes, wdno_attn_plan* out) {
  if (!out) return WDNO_EINVAL;
  attn_bwd_choose(d, has_rot != 0, has_bias != 0, want_dbias != 0, planes != 0, true, *out);
  return WDNO_OK;
}

extern "C" int wdno_attn_fwd(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out,
                             const wdno_attn_desc* d, float scale, wdno_stream_t s) {
  return wdno_attn_fwd_amax(qkv, rot_cos, rot_sin, bias, out, nullptr, d, scale, s);
}
// the thread-per-row kernels do not track the amax of what they write: a sweep over the result fills the record instead
static int attn_amax_sweep(int rc, const float* t, const wdno_attn_desc* d, int width, float* amax_rec, wdno_stream_t s) {
  if (rc != WDNO_OK || !amax_rec) return rc;
  return wdno_amax_record(t, (int64_t)d->n_uo * d->n_ui * d->n_tok * width, amax_rec, s);
}
// the forward launch of a plan (p.amax_rec and the plane fields are the caller's)
static int attn_fwd_launch(const wdno_attn_plan& pl, const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out,
                           AttnP& p, wdno_stream_t s) {
  switch (pl.family) {
    case WDNO_ATTN_MFMA24: attn_fwd_mfma_kernel<24><<<(unsigned)pl.grid, 64 * AM_WAVES, 0, as_stream(s)>>>(qkv, rot_cos, rot_sin, bias, out, p); break;
    case WDNO_ATTN_MFMA: attn_fwd_mfma_kernel<0><<<(unsigned)pl.grid, 64 * AM_WAVES, 0, as_stream(s)>>>(qkv, rot_cos, rot_sin, bias, out, p); break;
    case WDNO_ATTN_MFMA64: attn_fwd_mfma64_launch(qkv, rot_cos, rot_sin, bias, out, p, pl.grid, as_stream(s)); break;
    case WDNO_ATTN_TILED: attn_fwd_mfma_tiled_kernel<<<(unsigned)pl.grid, 64 * AM_WAVES, 0, as_stream(s)>>>(qkv, out, p); break;
    case WDNO_ATTN_ROWS:
      p.ipb = pl.items_per_block;
      if (pl.lds_bytes > 64 * 1024) am_dyn_lds((const void*)attn_fwd_kernel, pl.lds_bytes);
      attn_fwd_kernel<<<(unsigned)pl.grid, ATT_THREADS, (size_t)pl.lds_bytes, as_stream(s)>>>(qkv, rot_cos, rot_sin, bias, out, p);
      break;
    default: return WDNO_EUNSUPPORTED;
  }
  return wdno_check_launch();
}
// the one body of the forward entry points: fills AttnP, asks the plan. planes: out delivered ONLY as fp16 planes for the to_out projection
// (MFMA paths only: n_tok <= 64; `out` is not written; out_lo == NULL: one bf16 plane)
static int attn_fwd_run(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out, float* amax_rec,
                        const wdno_attn_desc* d, float scale, wdno_stream_t s, bool planes, void* out_hi = nullptr, void* out_lo = nullptr,
                        float* out_scale = nullptr, const float* rec_qkv = nullptr) {
  AttnP p;
  int rc = attn_fill(p, d, scale, ATT_THREADS);
  if (rc) return rc;
  wdno_attn_plan pl;
  rc = attn_fwd_choose(d, rot_cos != nullptr, bias != nullptr, planes, pl);
  if (rc) return rc;
  if (planes) {
    if (!out_hi || (out_lo && (!out_scale || !rec_qkv))) return WDNO_EUNSUPPORTED;
    p.pl_hi = (_Float16*)out_hi; p.pl_lo = (_Float16*)out_lo; p.rec_qkv = rec_qkv; p.pl_scale = out_scale;
  } else if (pl.family == WDNO_ATTN_ROWS) {
    return attn_amax_sweep(attn_fwd_launch(pl, qkv, rot_cos, rot_sin, bias, out, p, s), out, d, p.HD, amax_rec, s);
  }
  p.amax_rec = amax_rec;
  return attn_fwd_launch(pl, qkv, rot_cos, rot_sin, bias, out, p, s);
}
extern "C" int wdno_attn_fwd_amax(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out,
                                  float* amax_rec, const wdno_attn_desc* d, float scale, wdno_stream_t s) {
  return attn_fwd_run(qkv, rot_cos, rot_sin, bias, out, amax_rec, d, scale, s, false);
}
extern "C" int wdno_attn_fwd_planes(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out,
                                    void* out_hi, void* out_lo, float* out_scale, float* amax_rec, const float* rec_qkv,
                                    const wdno_attn_desc* d, float scale, wdno_stream_t s) {
  return attn_fwd_run(qkv, rot_cos, rot_sin, bias, out, amax_rec, d, scale, s, true, out_hi, out_lo, out_scale, rec_qkv);
}
// blocks of the backward launch with a bias gradient (= number of dbias partials) and the workspace that holds them; none for a shape the
// backward refuses (the launch paths return that refusal before they look at the workspace)
static int64_t attn_bwd_blocks(const wdno_attn_desc* d) {
  wdno_attn_plan pl;
  return attn_bwd_choose(d, true, true, true, false, true, pl) ? 0 : pl.grid;
}
extern "C" size_t wdno_attn_bwd_ws_bytes(const wdno_attn_desc* d) {
  if (!d || d->n_tok <= 0 || d->heads <= 0) return 0;
  return (size_t)attn_bwd_blocks(d) * d->heads * d->n_tok * d->n_tok * sizeof(float);
}
static int attn_dbias_reduce(const float* part, int64_t nb, float* dbias, const wdno_attn_desc* d, wdno_stream_t s) {
  const int E = d->heads * d->n_tok * d->n_tok;
  attn_dbias_reduce_kernel<<<(unsigned)((E + DBR_EL - 1) / DBR_EL), 256, 0, as_stream(s)>>>(part, (int)nb, dbias, E);
  return wdno_check_launch();
}
extern "C" int wdno_attn_bwd(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out,
                             const float* dout, float* dqkv, float* dbias, const wdno_attn_desc* d, float scale, void* ws, size_t ws_bytes,
                             wdno_stream_t s) {
  return wdno_attn_bwd_amax(qkv, rot_cos, rot_sin, bias, out, dout, dqkv, dbias, nullptr, d, scale, ws, ws_bytes, s);
}
// the backward launch of a plan; part = the workspace of the dbias partials or NULL
static int attn_bwd_launch(const wdno_attn_plan& pl, const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias,
                           const float* out, const float* dout, float* dqkv, float* part, AttnP& p, wdno_stream_t s) {
  const unsigned nb = (unsigned)pl.grid;
  const size_t lds = (size_t)pl.lds_bytes;
  p.db_slices = pl.dbias_in_lds == AM_WAVES;
  if ((pl.family == WDNO_ATTN_MFMA24 || pl.family == WDNO_ATTN_MFMA) && pl.lds_bytes > 64 * 1024)
    am_dyn_lds(pl.family == WDNO_ATTN_MFMA24 ? (const void*)attn_bwd_mfma_kernel<24> : (const void*)attn_bwd_mfma_kernel<0>, lds);
  switch (pl.family) {
    case WDNO_ATTN_MFMA24: attn_bwd_mfma_kernel<24><<<nb, 64 * AM_WAVES, lds, as_stream(s)>>>(qkv, rot_cos, rot_sin, bias, out, dout, dqkv, part, p); break;
    case WDNO_ATTN_MFMA: attn_bwd_mfma_kernel<0><<<nb, 64 * AM_WAVES, lds, as_stream(s)>>>(qkv, rot_cos, rot_sin, bias, out, dout, dqkv, part, p); break;
    case WDNO_ATTN_TILED_STAGED: attn_bwd_mfma_tiled_kernel<true><<<nb, 64 * AM_WAVES, 0, as_stream(s)>>>(qkv, out, dout, dqkv, p); break;
    case WDNO_ATTN_TILED_UNSTAGED: attn_bwd_mfma_tiled_kernel<false><<<nb, 64 * AM_WAVES, 0, as_stream(s)>>>(qkv, out, dout, dqkv, p); break;
    case WDNO_ATTN_BIG:
      am_dyn_lds((const void*)attn_bwd_big_kernel, lds);      // always
      attn_bwd_big_kernel<<<nb, ATT_BIG_THREADS, lds, as_stream(s)>>>(qkv, out, dout, dqkv, p);
      break;
    case WDNO_ATTN_ROWS:
      p.ipb = pl.items_per_block;
      if (pl.lds_bytes > 64 * 1024) am_dyn_lds((const void*)attn_bwd_kernel, lds);
      attn_bwd_kernel<<<nb, ATT_BWD_THREADS, lds, as_stream(s)>>>(qkv, rot_cos, rot_sin, bias, out, dout, dqkv, part, p);
      break;
    default: return WDNO_EUNSUPPORTED;
  }
  return wdno_check_launch();
}
// the one body of the backward entry points. planes: dqkv as fp16 planes for the qkv projection's gradient kernels (MFMA path only:
// n_tok <= 32; dqkv_lo == NULL: one bf16 plane, no scale); the plan is then never one of the two families that need the amax sweep
static int attn_bwd_run(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out, const float* dout,
                        float* dqkv, float* dbias, float* amax_rec, const wdno_attn_desc* d, float scale, void* ws, size_t ws_bytes,
                        wdno_stream_t s, bool planes, void* dqkv_hi = nullptr, void* dqkv_lo = nullptr, float* dqkv_scale = nullptr,
                        const float* rec_qkv = nullptr, const float* rec_dout = nullptr) {
  AttnP p;
  int rc = attn_fill(p, d, scale, ATT_BWD_THREADS);
  if (rc) return rc;
  wdno_attn_plan pl;
  rc = attn_bwd_choose(d, rot_cos != nullptr, bias != nullptr, dbias != nullptr, planes, out != nullptr, pl);
  if (rc) return rc;
  if (planes && (!dqkv_hi || (dqkv_lo && (!dqkv_scale || !rec_qkv || !rec_dout)))) return WDNO_EUNSUPPORTED;
  if (dbias && (!ws || ws_bytes < wdno_attn_bwd_ws_bytes(d))) return WDNO_EWORKSPACE;
  float* part = dbias ? (float*)ws : nullptr;           // the kernels write per-block partials; the reduce below writes dbias
  const bool sweep = pl.family == WDNO_ATTN_BIG || pl.family == WDNO_ATTN_ROWS;      // these two do not track the amax of what they write
  if (!sweep) p.amax_rec = amax_rec;
  if (planes) { p.pl_hi = (_Float16*)dqkv_hi; p.pl_lo = (_Float16*)dqkv_lo; p.rec_qkv = rec_qkv; p.rec_dout = rec_dout; p.pl_scale = dqkv_scale; }
  rc = attn_bwd_launch(pl, qkv, rot_cos, rot_sin, bias, out, dout, dqkv, part, p, s);
  if (sweep) rc = attn_amax_sweep(rc, dqkv, d, p.RW, amax_rec, s);
  return (rc || !dbias) ? rc : attn_dbias_reduce(part, pl.dbias_partials, dbias, d, s);
}
extern "C" int wdno_attn_bwd_amax(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out,
                                  const float* dout, float* dqkv, float* dbias, float* amax_rec, const wdno_attn_desc* d, float scale,
                                  void* ws, size_t ws_bytes, wdno_stream_t s) {
  return attn_bwd_run(qkv, rot_cos, rot_sin, bias, out, dout, dqkv, dbias, amax_rec, d, scale, ws, ws_bytes, s, false);
}
extern "C" int wdno_attn_bwd_planes(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out,
                                    const float* dout, void* dqkv_hi, void* dqkv_lo, float* dqkv_scale, float* dbias,
                                    const float* rec_qkv, const float* rec_dout, const wdno_attn_desc* d, float scale, void* ws, size_t ws_bytes,
                                    wdno_stream_t s) {
  return attn_bwd_run(qkv, rot_cos, rot_sin, bias, out, dout, nullptr, dbias, nullptr, d, scale, ws, ws_bytes, s, true, dqkv_hi, dqkv_lo,
                      dqkv_scale, rec_qkv, rec_dout);
}
