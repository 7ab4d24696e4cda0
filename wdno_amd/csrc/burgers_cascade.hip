// burgers_cascade.hip -- the hand-off between two levels of the zero-shot super-resolution cascade (evaluate, burgers/eval_ddpm_burgers.py:306-338)
// as ONE launch that writes every element of the super level's condition source src [B][17][P_t][P_x] in network units:
//   channels 8..15  low: the previous level's returned block x_prev [B][8][h0][w0] (the sample times RESCALER), read in place through its
//                   strides, nearest x2 on rows and columns (upsample_coef), zero beyond (2 h0, 2 w0), / RESCALER[8 + c] (IEEE division: the
//                   reference's (x r) / r bit for bit). 2 h0 is the fine block's height plus one: the ps[0] + 1 rows the sampler copies
//   channel 16      the u0 / uT condition (test_util.py:185-196): four stripes of P_t / 4 rows -- the low band of u(t = 0), its high band, the
//                   low band of u(t = T), its high band --, each the one-level periodized 1-D analysis along x of that row of the level's
//                   target, / RESCALER[16], the same on every row of its stripe, n_x / 2 columns and zero beyond. The two target rows are
//                   read in place through sample, row and column strides; a stripe whose flag is off is zero
//   channels 0..7   zero
// It replaces upsample_coef, the pad, the division, get_target(is_wave=True), two slices and two divisions, and the zeroed tensor and three
// copies of GaussianDiffusion._sampling_setup. include/wdno_hip.h states the contract; wdno_amd/burgers/cascade.py: plan() checks the integers.
//
// grid = (row tiles, 17, B): a workgroup of 256 threads owns `tile` rows of one (sample, channel) plane, so the branch on the channel is
// uniform; a thread decodes (row, float4 column) from its index with one multiply-high and issues one aligned 16-byte store per item. A
// workgroup of channel 16 first forms the four bands -- 2 n_x outputs of L taps -- in LDS as finished rows of P_x floats (zero beyond the
// band, zero for a stripe that is off), then stores them row by row: cheaper than a second launch and a round trip through memory. The
// analysis sums run m = 0 .. L - 1 with fmaf, the order of analysis_kernel (dwt.hip). Store-bound: 17 P_t P_x floats per sample, once.
#include "common.h"
#include "fastdiv.h"

namespace {

constexpr int L = 10;
constexpr int NT = 256;
constexpr int C = 17;

struct CasP {
  const float* prev; const float* tgt; const float* resc; float* out;
  int64_t pss, tss, trs, tcs;             // sample stride of prev; sample, row, column strides of the target (elements)
  int pcs, prs;                           // channel and row strides of prev
  int h0, w0, n_t, n_x, P_t, P_x, tile;
  int cond_u0, cond_uT;
  FastDiv dW4, dPx;
  float lo[L], hi[L];                     // dec_lo, dec_hi as filter_bank() has them: the sum reads tap L - 1 - m
};

__global__ __launch_bounds__(NT) void burgers_cascade_kernel(CasP p) {
  extern __shared__ __align__(16) float band[];          // [4][P_x], channel 16 only
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int W4 = p.P_x >> 2;
  const int row0 = (int)blockIdx.x * p.tile, rows = min(p.tile, p.P_t - row0);
  const int n4 = rows * W4;
  float4* const out = reinterpret_cast<float4*>(p.out + (((size_t)b * C + c) * p.P_t + row0) * p.P_x);
  if (c >= 8 && c < 16) {                  // low
    const float r = p.resc[c];
    const float* const src = p.prev + (size_t)b * p.pss + (size_t)(c - 8) * p.pcs;
    for (int i = tid; i < n4; i += NT) {
      const int hl = fd_div(i, p.dW4), w = (i - hl * W4) * 4, h = row0 + hl;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (h < 2 * p.h0) {
        const float* const row = src + (size_t)(h >> 1) * p.prs;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (w + e < 2 * p.w0) v[e] = row[(w + e) >> 1] / r;
      }
      out[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else if (c == C - 1) {                 // the u0 / uT condition
    const float r = p.resc[c];
    const int nx = p.n_x >> 1;
    for (int i = tid; i < 4 * p.P_x; i += NT) {
      const int s = fd_div(i, p.dPx), j = i - s * p.P_x;
      float acc = 0.f;
      if (j < nx && ((s < 2) ? p.cond_u0 : p.cond_uT)) {
        const float* const x = p.tgt + (size_t)b * p.tss + (s < 2 ? (size_t)0 : (size_t)(p.n_t - 1) * p.trs);
        const bool high = s & 1;
        int jj = 2 * j - (L / 2 - 1);
        jj = jj < 0 ? jj + p.n_x : jj;
#pragma unroll
        for (int m = 0; m < L; ++m) {
          acc = fmaf(high ? p.hi[L - 1 - m] : p.lo[L - 1 - m], x[(size_t)jj * p.tcs], acc);
          jj = jj + 1 == p.n_x ? 0 : jj + 1;
        }
        acc = acc / r;
      }
      band[i] = acc;
    }
    __syncthreads();
    const int rep = p.P_t >> 2;
    int s0 = 0;
    for (int q = rep; q <= row0; q += rep) ++s0;        // the stripe of the tile's first row: at most three steps
    for (int i = tid; i < n4; i += NT) {
      const int hl = fd_div(i, p.dW4), w4 = i - hl * W4, h = row0 + hl;
      int s = s0;
      while ((s + 1) * rep <= h) ++s;
      out[i] = reinterpret_cast<const float4*>(band + s * p.P_x)[w4];
    }
  } else {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = tid; i < n4; i += NT) out[i] = z;
  }
}

int validate(const wdno_burgers_cascade_desc* d) {
  if (!d) return WDNO_EINVAL;
  if (d->mode != 0 || d->L != L) return WDNO_EUNSUPPORTED;
  WDNO_REQUIRE(d->C == C && d->B > 0 && d->B <= 65535);
  WDNO_REQUIRE(d->P_t >= 4 && d->P_x >= 4 && !(d->P_t & 3) && !(d->P_x & 3) && d->P_x <= 2048);
  WDNO_REQUIRE((int64_t)C * d->P_t * d->P_x < ((int64_t)1 << 31));
  WDNO_REQUIRE(d->h0 >= 1 && d->w0 >= 1 && d->h1 >= 1 && d->w1 >= 1);
  WDNO_REQUIRE(2 * d->h0 == d->h1 + 1 && 2 * d->w0 == d->w1 && 2 * d->h0 <= d->P_t && 2 * d->w0 <= d->P_x);
  WDNO_REQUIRE(d->n_t >= 2 && d->n_x >= L && d->n_x == 2 * d->w1);
  WDNO_REQUIRE(d->prev_row_stride >= d->w0 && (int64_t)d->prev_chan_stride >= (int64_t)d->h0 * d->prev_row_stride &&
               d->prev_sample_stride >= (int64_t)8 * d->prev_chan_stride);
  WDNO_REQUIRE(d->tgt_sample_stride >= 0 && d->tgt_row_stride >= 0 && d->tgt_col_stride >= 1);
  WDNO_REQUIRE(d->tile >= 1 && d->tile <= d->P_t && d->ntile == (d->P_t + d->tile - 1) / d->tile && d->ntile <= 65535);
  WDNO_REQUIRE((int64_t)d->tile * (d->P_x >> 2) < ((int64_t)1 << 20) && d->lds_bytes == 16 * d->P_x);      // fd_div range; [4][P_x] floats
  WDNO_REQUIRE((d->cond_u0 == 0 || d->cond_u0 == 1) && (d->cond_uT == 0 || d->cond_uT == 1) && d->reserved == 0);
  return WDNO_OK;
}

}  // namespace

extern "C" int wdno_burgers_cascade_conditions(const float* x_prev, const float* u_target, const float* rescaler, float* src,
                                               const wdno_burgers_cascade_desc* d, const float* filt, wdno_stream_t s) {
  WDNO_REQUIRE(x_prev && u_target && rescaler && src && d && filt);
  const int rc = validate(d);
  if (rc) return rc;
  WDNO_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0);
  CasP p;
  p.prev = x_prev; p.tgt = u_target; p.resc = rescaler; p.out = src;
  p.pss = d->prev_sample_stride; p.tss = d->tgt_sample_stride; p.trs = d->tgt_row_stride; p.tcs = d->tgt_col_stride;
  p.pcs = d->prev_chan_stride; p.prs = d->prev_row_stride;
  p.h0 = d->h0; p.w0 = d->w0; p.n_t = d->n_t; p.n_x = d->n_x; p.P_t = d->P_t; p.P_x = d->P_x; p.tile = d->tile;
  p.cond_u0 = d->cond_u0; p.cond_uT = d->cond_uT;
  p.dW4 = make_fastdiv(d->P_x >> 2);
  p.dPx = make_fastdiv(d->P_x);
  for (int m = 0; m < L; ++m) { p.lo[m] = filt[m]; p.hi[m] = filt[L + m]; }
  burgers_cascade_kernel<<<dim3((unsigned)d->ntile, C, (unsigned)d->B), NT, (size_t)d->lds_bytes, as_stream(s)>>>(p);
  return wdno_check_launch();
}
