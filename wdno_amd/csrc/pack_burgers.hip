// pack_burgers.hip -- the U-Net input of the Burgers wavelet models for a batch, from the coefficient levels the offline transform stores, in ONE
// launch that writes every element of state [B][C][pad_t][pad_x] = value / rescaler[c], C = 8 + 8 has_low + has_cond (include/wdno_hip.h:
// wdno_pack_burgers_state states the contract). It replaces get_wavelet_super_preprocess of ddpm_burgers/data_burgers_1d.py per batch: cat + pad
// of the eight sub-bands of (u, f), the repeated last row and the nearest-upsampled coarser level of the super-resolution models, the division,
// and for the condition channel a full 2-D IDWT of both fields of which two rows of u are kept, then their 1-D DWT.
//
// grid = (4, C, B): a workgroup of 256 threads owns pad_t / 4 rows of one (sample, channel) plane -- one stripe of the condition channel --, so
// the branch on the channel is uniform; a thread decodes (row, float4 column) from its index with one multiply-high and issues one aligned
// 16-byte store per item. Loads are as wide as the level's rows allow (template FV = floats per fine load, CV per coarse load: nx = 60 / 30 / 15
// on the real levels take 16 / 8 / 4 bytes); wdno_pack_burgers_plan_query names the form.
//
// A workgroup of the condition channel forms ONE band of ONE row of u in LDS: the periodized 2-D synthesis restricted to the output row n (0 or
// ori_t - 1) -- W pass over the L / 2 coefficient rows K = q - i of both H bands into S1, then the H pass down each column --, then the
// periodized 1-D analysis of that row along x, divided, as a finished row of pad_x floats that is stored pad_t / 4 times. Every sum runs in the
// order of the transform kernels (W pass: dw_pair_term, H pass: dw_column of dwt_tiles.h, i = 0, 1, .. with the low band before the high band;
// analysis: m = 0 .. L - 1 as analysis_kernel of dwt.hip), all with fmaf. Store-bound: C pad_t pad_x floats per sample, once.
#include "common.h"
#include "fastdiv.h"

namespace {

constexpr int NT = 256;
constexpr int MAXL = 16;

struct PackBurgersP {
  const float* fine; const float* coarse; const int64_t* idx; const float* resc; float* out;
  int64_t fine_sim, coarse_sim;          // elements between consecutive samples of the two levels
  int nt, nx, nt_c, nx_c, pad_t, pad_x, C, ori_t, has_low, cond_u0, cond_uT, L;
  FastDiv dW4, dNW;
  float taps[4 * MAXL];                  // dec_lo, dec_hi, rec_lo, rec_hi as filter_bank() has them
};

struct Plan { int fine_vec, coarse_vec, lds_bytes, C, rc; };

// four consecutive floats of a row of which `rem` (> 0) are left from src on
template <int FV>
__device__ __forceinline__ void load4(const float* __restrict__ src, int rem, float* v) {
  if (FV == 4) {                         // rows of a multiple of four floats: rem >= 4
    const float4 a = *reinterpret_cast<const float4*>(src);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else if (FV == 2) {                  // rows of an even number of floats: rem is even
    const float2 a = *reinterpret_cast<const float2*>(src);
    v[0] = a.x; v[1] = a.y;
    if (rem >= 4) {
      const float2 bb = reinterpret_cast<const float2*>(src)[1];
      v[2] = bb.x; v[3] = bb.y;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < rem) v[e] = src[e];
  }
}

template <int FV, int CV>
__global__ __launch_bounds__(NT) void pack_burgers_state_kernel(PackBurgersP p) {
  extern __shared__ __align__(16) float lds[];           // condition channel only: band [pad_x], u [2 nx], S1 [2][L / 2][2 nx]
  __shared__ float tp[4 * MAXL];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int W4 = p.pad_x >> 2, rep = p.pad_t >> 2;
  const int row0 = (int)blockIdx.x * rep, n4 = rep * W4;
  const int64_t sim = p.idx ? p.idx[b] : b;
  const float r = p.resc[c];
  float4* const out = reinterpret_cast<float4*>(p.out + (((size_t)b * p.C + c) * p.pad_t + row0) * p.pad_x);
  if (c < 8) {                             // the level's own sub-bands; super-resolution models: row nt repeats row nt - 1
    const float* const src = p.fine + sim * p.fine_sim + (int64_t)c * p.nt * p.nx;
    const int hmax = p.has_low ? p.nt + 1 : p.nt;
    for (int i = tid; i < n4; i += NT) {
      const int hl = fd_div(i, p.dW4), w0 = (i - hl * W4) * 4, h = row0 + hl;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (h < hmax && w0 < p.nx) load4<FV>(src + min(h, p.nt - 1) * p.nx + w0, p.nx - w0, v);
      out[i] = make_float4(v[0] / r, v[1] / r, v[2] / r, v[3] / r);
    }
  } else if (p.has_low && c < 16) {        // the next-coarser level, nearest x2 on rows and columns (upsample_coef)
    const float* const src = p.coarse + sim * p.coarse_sim + (int64_t)(c - 8) * p.nt_c * p.nx_c;
    for (int i = tid; i < n4; i += NT) {
      const int hl = fd_div(i, p.dW4), w0 = (i - hl * W4) * 4, h = row0 + hl;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      const int j = w0 >> 1;                 // (w0 a multiple of 4: j even)
      if (h < 2 * p.nt_c && j < p.nx_c) {
        const float* const row = src + (h >> 1) * p.nx_c + j;
        if (CV == 2) {                       // rows of an even number of floats: j + 1 < nx_c
          const float2 a = *reinterpret_cast<const float2*>(row);
          v[0] = v[1] = a.x; v[2] = v[3] = a.y;
        } else {
          v[0] = v[1] = row[0];
          if (j + 1 < p.nx_c) v[2] = v[3] = row[1];
        }
      }
      out[i] = make_float4(v[0] / r, v[1] / r, v[2] / r, v[3] / r);
    }
  } else {                                 // the u0 / uT condition: stripe s = blockIdx.x
    const int s = blockIdx.x, NW = 2 * p.nx, HL = p.L >> 1, off = HL - 1;
    float* const band = lds;
    float* const u = lds + p.pad_x;
    float* const S1 = u + NW;
    const bool on = s < 2 ? p.cond_u0 != 0 : p.cond_uT != 0;
    if (on) {
      if (tid < 4 * MAXL) tp[tid] = p.taps[tid];
      __syncthreads();
      const float* const rlo = tp + 2 * MAXL;
      const float* const rhi = tp + 3 * MAXL;
      const int n = s < 2 ? 0 : p.ori_t - 1;
      const int qh = (n + off) >> 1, rh = (n + off) & 1;
      const int plane = p.nt * p.nx;
      const float* const ub = p.fine + sim * p.fine_sim;             // field u: bands [bw 2 + bh] (tensor_to_coef)
      // W pass: S1[bh][i][w] = the synthesis along x of coefficient row K = (qh - i) mod nt of the band pair (bh, bh + 2)
      for (int it = tid; it < 2 * HL * NW; it += NT) {
        const int ri = fd_div(it, p.dNW), w = it - ri * NW;
        const int bh = ri >= HL ? 1 : 0, i = ri - bh * HL;
        int K = (qh - i) % p.nt;
        K = K < 0 ? K + p.nt : K;
        const float* const cl = ub + bh * plane + K * p.nx;
        const float* const ch = cl + 2 * plane;
        const int rw = (w + off) & 1;
        int kk = ((w + off) >> 1) % p.nx;
        float acc = 0.f;
        for (int k = 0; k < HL; ++k) {
          acc = fmaf(cl[kk], rlo[rw + 2 * k], acc);
          acc = fmaf(ch[kk], rhi[rw + 2 * k], acc);
          kk = kk == 0 ? p.nx - 1 : kk - 1;
        }
        S1[it] = acc;
      }
      __syncthreads();
      // H pass: row n of u
      for (int w = tid; w < NW; w += NT) {
        float acc = 0.f;
        for (int i = 0; i < HL; ++i) {
          acc = fmaf(S1[i * NW + w], rlo[rh + 2 * i], acc);
          acc = fmaf(S1[(HL + i) * NW + w], rhi[rh + 2 * i], acc);
        }
        u[w] = acc;
      }
      __syncthreads();
      // analysis along x: the low (s even) or high band, nx coefficients, zero beyond
      const float* const f = tp + (s & 1) * MAXL;
      for (int j = tid; j < p.pad_x; j += NT) {
        float acc = 0.f;
        if (j < p.nx) {
          int jj = (2 * j - off) % NW;
          jj = jj < 0 ? jj + NW : jj;
          for (int m = 0; m < p.L; ++m) {
            acc = fmaf(f[p.L - 1 - m], u[jj], acc);
            jj = jj + 1 == NW ? 0 : jj + 1;
          }
        }
        band[j] = acc / r;
      }
    } else {
      for (int j = tid; j < p.pad_x; j += NT) band[j] = 0.f / r;
    }
    __syncthreads();
    for (int i = tid; i < n4; i += NT) {
      const int hl = fd_div(i, p.dW4), w4 = i - hl * W4;
      out[i] = reinterpret_cast<const float4*>(band)[w4];
    }
  }
}

// The argument rules and the launch form, for the entry and the query alike. align: the addresses of fine | coarse | state OR-ed.
Plan plan_of(int64_t fine_sim, int64_t coarse_sim, int64_t B, int nt, int nx, int nt_c, int nx_c, int pad_t, int pad_x, int ori_t, int ori_x,
             int has_low, int cond_u0, int cond_uT, int L, uintptr_t fine_a, uintptr_t coarse_a, uintptr_t state_a) {
  Plan pl = {0, 0, 0, 0, WDNO_EINVAL};
  const bool flags = (has_low == 0 || has_low == 1) && (cond_u0 == 0 || cond_u0 == 1) && (cond_uT == 0 || cond_uT == 1);
  if (!flags || B <= 0 || nt <= 0 || nx <= 0 || pad_t <= 0 || pad_x <= 0 || fine_sim < 8ll * nt * nx) return pl;
  if (has_low && (nt_c <= 0 || nx_c <= 0 || coarse_sim < 8ll * nt_c * nx_c)) return pl;
  if (nt > pad_t || nx > pad_x) return pl;                                             // the box
  if (has_low && nt + 1 > pad_t) return pl;                                            // the repeated row
  if (has_low && (2 * nt_c > pad_t || 2 * nx_c > pad_x)) return pl;                    // the doubled coarse block
  if (ori_t < 1 || ori_t > 2 * nt) return pl;
  if (state_a & 15) return pl;
  pl.rc = WDNO_EUNSUPPORTED;
  if ((pad_t & 3) || (pad_x & 3) || ori_x != 2 * nx || L < 2 || L > MAXL || (L & 1)) return pl;
  if (pad_t > 4096 || pad_x > 4096 || B > 65535) return pl;                            // fd_div range; grid
  const int64_t lds = 4ll * (pad_x + 2 * nx + (int64_t)L * 2 * nx);
  if (lds > 64 * 1024) return pl;
  pl.fine_vec = (!(nx & 3) && !(fine_sim & 3) && !(fine_a & 15)) ? 4 : (!(nx & 1) && !(fine_sim & 1) && !(fine_a & 7)) ? 2 : 1;
  pl.coarse_vec = (has_low && !(nx_c & 1) && !(coarse_sim & 1) && !(coarse_a & 7)) ? 2 : 1;
  pl.lds_bytes = (cond_u0 || cond_uT) ? (int)lds : 0;
  pl.C = 8 + 8 * has_low + ((cond_u0 || cond_uT) ? 1 : 0);
  pl.rc = WDNO_OK;
  return pl;
}

template <int FV>
void launch(const Plan& pl, const PackBurgersP& p, dim3 grid, hipStream_t st) {
  if (pl.coarse_vec == 2) pack_burgers_state_kernel<FV, 2><<<grid, NT, (size_t)pl.lds_bytes, st>>>(p);
  else pack_burgers_state_kernel<FV, 1><<<grid, NT, (size_t)pl.lds_bytes, st>>>(p);
}

}  // namespace

extern "C" int wdno_pack_burgers_plan_query(int64_t fine_sim_stride, int64_t coarse_sim_stride, int64_t B, int nt, int nx, int nt_c, int nx_c,
                                            int pad_t, int pad_x, int ori_t, int ori_x, int has_low, int cond_u0, int cond_uT, int L,
                                            unsigned align_mask, wdno_pack_burgers_plan* out) {
  WDNO_REQUIRE(out);
  const Plan pl = plan_of(fine_sim_stride, coarse_sim_stride, B, nt, nx, nt_c, nx_c, pad_t, pad_x, ori_t, ori_x, has_low, cond_u0, cond_uT, L,
                          align_mask, align_mask, align_mask);
  *out = wdno_pack_burgers_plan{pl.fine_vec, pl.coarse_vec, pl.rc ? 0 : 4, pl.C, pl.rc ? 0 : (int)B, pl.lds_bytes, pl.rc, 0};
  return WDNO_OK;
}

extern "C" int wdno_pack_burgers_state(const float* fine, int64_t fine_sim_stride, const float* coarse, int64_t coarse_sim_stride, const int64_t* idx,
                                       const float* rescaler, float* state, int64_t B, int nt, int nx, int nt_c, int nx_c, int pad_t, int pad_x,
                                       int ori_t, int ori_x, int has_low, int cond_u0, int cond_uT, const float* dec_lo_host,
                                       const float* dec_hi_host, const float* rec_lo_host, const float* rec_hi_host, int L, wdno_stream_t s) {
  WDNO_REQUIRE(fine && rescaler && state && (coarse || !has_low));
  const bool has_cond = cond_u0 || cond_uT;
  WDNO_REQUIRE(!has_cond || (dec_lo_host && dec_hi_host && rec_lo_host && rec_hi_host));
  const Plan pl = plan_of(fine_sim_stride, coarse_sim_stride, B, nt, nx, nt_c, nx_c, pad_t, pad_x, ori_t, ori_x, has_low, cond_u0, cond_uT, L,
                          reinterpret_cast<uintptr_t>(fine), reinterpret_cast<uintptr_t>(coarse), reinterpret_cast<uintptr_t>(state));
  if (pl.rc) return pl.rc;
  PackBurgersP p;
  p.fine = fine; p.coarse = coarse; p.idx = idx; p.resc = rescaler; p.out = state;
  p.fine_sim = fine_sim_stride; p.coarse_sim = coarse_sim_stride;
  p.nt = nt; p.nx = nx; p.nt_c = nt_c; p.nx_c = nx_c; p.pad_t = pad_t; p.pad_x = pad_x; p.C = pl.C; p.ori_t = ori_t;
  p.has_low = has_low; p.cond_u0 = cond_u0; p.cond_uT = cond_uT; p.L = L;
  p.dW4 = make_fastdiv(pad_x >> 2); p.dNW = make_fastdiv(2 * nx);
  for (int m = 0; m < 4 * MAXL; ++m) p.taps[m] = 0.f;
  if (has_cond)
    for (int m = 0; m < L; ++m) {
      p.taps[m] = dec_lo_host[m]; p.taps[MAXL + m] = dec_hi_host[m];
      p.taps[2 * MAXL + m] = rec_lo_host[m]; p.taps[3 * MAXL + m] = rec_hi_host[m];
    }
  const dim3 grid(4, (unsigned)pl.C, (unsigned)B);
  const hipStream_t st = as_stream(s);
  if (pl.fine_vec == 4) launch<4>(pl, p, grid, st);
  else if (pl.fine_vec == 2) launch<2>(pl, p, grid, st);
  else launch<1>(pl, p, grid, st);
  return wdno_check_launch();
}
