/* wdno_hip.h -- C ABI of libwdno_hip.so: hand-written gfx950 (MI355X) kernels for the WDNO hot path.
 *
 * The reference (AI4Science-WestlakeU/wdno) has no FFI of its own: its hot path is stock torch.nn + three
 * third-party wavelet packages. Each entry point below therefore cites the reference *operator* it replaces
 * (file:line relative to the reference root). INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a device pointer to contiguous fp32 unless stated; int64 for timestep indices;
 *   - "CL" = channels-last activations [N, (D,) H, W, C]; API layout = the reference's own tensor layout;
 *   - every call enqueues on `stream` and returns immediately: 0 on success, <0 = WDNO_E* (wdno_strerror);
 *   - no call allocates, synchronises or throws. Workspaces are caller-provided (size queried by *_ws_bytes).
 */
#ifndef WDNO_HIP_H
#define WDNO_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* wdno_stream_t; /* hipStream_t */

enum { WDNO_OK = 0, WDNO_EINVAL = -1, WDNO_ELAUNCH = -2, WDNO_EUNSUPPORTED = -3, WDNO_EWORKSPACE = -4 };

/* "amax record": WDNO_AMAX_FLOATS floats in device memory (WDNO_AMAX_SLOTS slots, one per 64-byte line so that the atomic
 * updates of a launch do not serialise), zeroed by the caller, whose maximum is max|x| of one tensor. The
 * fp32-equivalent convolutions scale their fp16 split by it. wdno_amax_record fills one with a sweep over x; the *_amax
 * forms of the kernels that WRITE activation tensors (group norm, layer norm, concat, add) fill one for their output on
 * the way (amax_rec may be NULL: not wanted), which saves that sweep. */
#define WDNO_AMAX_SLOTS 64
#define WDNO_AMAX_STRIDE 16
#define WDNO_AMAX_FLOATS (WDNO_AMAX_SLOTS * WDNO_AMAX_STRIDE)
const char* wdno_strerror(int code);
int wdno_version(void);
/* last hip error string seen by the library on this thread (diagnostics only) */
const char* wdno_last_hip_error(void);
/* diagnostics only: the library-wide debug mode (0 = production). One integer that switches kernel selection for A/B measurements and tests;
 * wdno_amd/csrc/debug_modes.h lists every value. WDNO_EINVAL, and the mode stays as it was, for a value that is not listed there. */
int wdno_set_debug(int mode);

/* ------------------------------------------------------------------------------------------------ wavelets
 * Separable single-level filter banks. mode: 0 = periodization, 1 = zero padding. Filters: 4 x L floats
 * (dec_lo, dec_hi, rec_lo, rec_hi) on the HOST (copied into kernel arguments; L <= 16).
 *
 * wdno_dwt_fwd : x [n_img, dims...] -> coef [n_img, 2^nd, out dims...] with sub-bands stacked on axis 1 in
 *   pywt order (letters over axes slowest..fastest, a before d): 1-D (lo,hi); 2-D (LL,'da','ad','dd') =
 *   coef_to_tensor order burgers/wave_trans.py:43-62 ; 3-D 'aaa'..'ddd' = smoke/wave_trans_2d.py:55-58.
 *   Replaces pytorch_wavelets.DWTForward/DWT1DForward (burgers/wave_trans.py:94-107, data_burgers_1d.py:72)
 *   and ptwt.wavedec3 (smoke/wave_trans_2d.py:129). The packed output may be strided/padded:
 *   coef element (img, band, i0,i1,i2) lives at img*cs_img + band*cs_band + i0*cs0 + i1*cs1 + i2.
 * wdno_dwt_inv : the inverse (DWTInverse / DWT1DInverse / ptwt.waverec3), reading coef with the same strides.
 * wdno_dwt_inv_adjoint : d(loss)/d(coef) given d(loss)/d(x) for x = wdno_dwt_inv(coef)  (guidance back-prop,
 *   burgers/ddpm_burgers/model_utils.py:35-50, smoke/inference_2d.py:30-66).
 * wdno_dwt_fwd_adjoint : d(loss)/d(x) given d(loss)/d(coef) for coef = wdno_dwt_fwd(x).
 */
typedef struct {
  int nd;             /* 1, 2 or 3 transformed axes (the trailing ones) */
  int mode;           /* 0 periodization, 1 zero */
  int L;              /* filter length */
  int n_img;          /* product of all leading dims */
  int in_dims[3];     /* signal extent along each transformed axis (unused leading entries = 1) */
  int out_dims[3];    /* coefficient extent along each axis */
  int64_t cs_img, cs_band, cs0, cs1;   /* coefficient tensor strides (elements); innermost stride is 1.
                                          the signal tensor x is contiguous [n_img, in_dims...] */
} wdno_dwt_desc;
size_t wdno_dwt_ws_bytes(const wdno_dwt_desc* d);
int wdno_dwt_fwd(const float* x, float* coef, const wdno_dwt_desc* d, const float* filters_host, void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_dwt_inv(const float* coef, float* x, const wdno_dwt_desc* d, const float* filters_host, void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_dwt_fwd_adjoint(const float* dcoef, float* dx, const wdno_dwt_desc* d, const float* filters_host, void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_dwt_inv_adjoint(const float* dx, float* dcoef, const wdno_dwt_desc* d, const float* filters_host, void* ws, size_t ws_bytes, wdno_stream_t s);
/* 3-D zero-mode analysis whose coefficients go straight into a larger, differently ordered tensor, divided by a per-channel constant (the smoke
 * task's network input: smoke/ddpm/data_2d.py:156-221 does cat + pad + permute + `/ RESCALER` on the transform's output; here the transform's store
 * does it). Image i = (outer, inner) = (i / img_inner, i % img_inner) is stored at state + outer * cs_outer + inner * d->cs_img + band * d->cs_band +
 * k0 * d->cs0 + k1 * d->cs1 + k2, as value / rescaler[inner * 8 + band] (IEEE division: the bits of torch's `coef / RESCALER`). Rows are written
 * row_w columns wide (row_w >= out_dims[2], row_w % 4 == 0; 0 / rescaler beyond the coefficients; all strides % 4 == 0, state 16-byte aligned:
 * aligned 16-byte stores). One fused launch;
 * WDNO_EUNSUPPORTED for anything it does not take (nd != 3, mode != zero, filters longer than 10 taps, rows too wide for LDS): the caller then
 * transforms into a coefficient tensor (wdno_dwt_fwd) and packs (wdno_pack_smoke_fields). Nothing but the rows [k0 < out_dims[0]][k1 < out_dims[1]] of
 * the 8 channels of an image is written: wdno_pack_smoke_fields(coef = NULL, ...) fills the rest of the state. */
int wdno_dwt_fwd_packed(const float* x, float* state, const wdno_dwt_desc* d, const float* filters_host, int img_inner, int64_t cs_outer, int row_w,
                        const float* rescaler, wdno_stream_t s);
/* What the wavelet entry points above launch for a descriptor (nothing is launched; the launch path asks the same code, and the query
 * honours wdno_set_debug modes 11 and 45 and WDNO_DWT_LDS_KB exactly as the launch does). entry: WDNO_DWT_ENTRY_*.
 * family: WDNO_DWT_PER_AXIS (one analysis_kernel / synthesis_kernel launch per axis through the workspace of wdno_dwt_ws_bytes) or the ONE
 * fused kernel: WDNO_DWT_ANALYSIS / WDNO_DWT_ANALYSIS_PACKED (dwt_analysis_fused_kernel), WDNO_DWT_SYNTHESIS2 (dwt_synthesis2_kernel, 2-D, staged
 * rows), WDNO_DWT_SYNTHESIS_FUSED (dwt_synthesis_fused_kernel), WDNO_DWT_SYNTHESIS3_STREAM (dwt_synthesis3_stream_kernel); -1 when rc != WDNO_OK.
 * variant: PMAX (1, 2) of dwt_synthesis2_kernel, WMAX (4, 8) of the stream kernel, 0 otherwise. For a fused kernel nh = rows per tile
 * (coefficient rows of an analysis, q rows of a synthesis), tiles_h, tiles_t, blocks = n_img * tiles_t * tiles_h and lds_bytes = the dynamic LDS
 * of the launch; all 0 for the per-axis passes. rc = the code the entry point would return given the workspace of wdno_dwt_ws_bytes.
 * WDNO_DWT_ENTRY_FWD_PACKED: the arguments of wdno_dwt_fwd_packed that are not in the descriptor are taken as img_inner = 1, cs_outer = 0, an
 * aligned state and the narrowest legal row_w (out_dims[2] rounded up to 4). None of them enters the tile choice, so family, nh, tiles, blocks and
 * lds_bytes are those of the launch; the descriptor's own strides are tested as the launch tests them (any of cs_img, cs_band, cs0, cs1 not a
 * multiple of 4: WDNO_EUNSUPPORTED), but a launch can still refuse with WDNO_EUNSUPPORTED where the plan says WDNO_OK: for a misaligned state or
 * cs_outer, a row_w that is below out_dims[2] or no multiple of 4, or a row_w so wide that an item index leaves the 32-bit division range.
 * Returns WDNO_EINVAL only for out == NULL or an entry that is not listed. */
enum { WDNO_DWT_ENTRY_FWD = 0, WDNO_DWT_ENTRY_INV = 1, WDNO_DWT_ENTRY_INV_ADJOINT = 2, WDNO_DWT_ENTRY_FWD_ADJOINT = 3, WDNO_DWT_ENTRY_FWD_PACKED = 4 };
enum { WDNO_DWT_PER_AXIS = 0, WDNO_DWT_ANALYSIS = 1, WDNO_DWT_ANALYSIS_PACKED = 2, WDNO_DWT_SYNTHESIS2 = 3, WDNO_DWT_SYNTHESIS_FUSED = 4,
       WDNO_DWT_SYNTHESIS3_STREAM = 5 };
typedef struct { int family, variant, nh, tiles_h, tiles_t, blocks, lds_bytes, rc; } wdno_dwt_plan;
int wdno_dwt_plan_query(const wdno_dwt_desc* d, int entry, wdno_dwt_plan* out);
/* nearest x2 up-sampling of coefficient tensors (burgers/ddpm_burgers/wavelet_utils.py:5-16,
 * smoke/ddpm/wave_utils.py:1-14): in [outer, a, mid, b, c] -> out [outer, a*fa, mid, b*fb, c*fc]. */
int wdno_upsample_coef(const float* in, float* out, int64_t outer, int a, int mid, int b, int c, int fa, int fb, int fc, wdno_stream_t s);
/* Dataset packing of the smoke task for a batch, one launch (smoke/ddpm/data_2d.py:156-221, Smoke_wave.__getitem__ of a base-resolution model):
 *   state[b][f][c][h][w] = value / rescaler[c],   state [B][pad_t][8 F + 2][pad_x][pad_x]
 *   c <  8 F    : coef[sim][c / 8][c % 8][f][h][w] inside the [nt][nx][nx] box, 0 in the padding           (coef [.][F][8][nt][nx][nx])
 *   c == 8 F    : init_coef[sim][f / (pad_t / 4)][h][w] inside [nx][nx], 0 outside                          (the 4 sub-bands of the DWT of rho(t = 0))
 *   c == 8 F + 1: smokeout[sim][h >= pad_x / 2][f] for f < nt, 0 beyond                                     (smokeout [.][2][nt])
 * sim = idx[b] (device int64; NULL: b) selects the simulation inside resident stores whose per-simulation strides (in elements) are given --
 * the stores may hold the files exactly as the offline transform wrote them ([5][4][nx][nx] initial coefficients: field 0 is read).
 * IEEE division: bit-identical to the torch formulation. pad_t % 4 == 0, pad_x % 4 == 0. */
int wdno_pack_smoke_state(const float* coef, int64_t coef_sim_stride, const float* init_coef, int64_t init_sim_stride, const float* smokeout,
                          int64_t so_sim_stride, const int64_t* idx, const float* rescaler, float* state, int64_t B, int F, int nt, int nx,
                          int pad_t, int pad_x, wdno_stream_t s);
/* The same with the two condition channels transformed inside the launch from the physical inputs (the online pipeline fields -> DWT -> state,
 * smoke/wave_trans_2d.py:150-170 + data_2d.py:156-221): rho0 [.][H0][W0] = the density field at t = 0 (e.g. a view into the fields tensor),
 * curve [.][T0] = the smoke-out curve; zero-mode analysis with the decomposition filters (host arrays of L <= 16 taps).
 * coef == NULL: the rows [f < nt][h < nx] of the 8 F channels are left untouched (wdno_dwt_fwd_packed wrote them pad_x wide, already divided); the
 * zero rows / frames around them and the two condition channels are written -- together the two launches produce the same bits as the one-tensor form. */
int wdno_pack_smoke_fields(const float* coef, int64_t coef_sim_stride, const float* rho0, int64_t rho0_sim_stride, const float* curve,
                           int64_t curve_sim_stride, const float* dec_lo_host, const float* dec_hi_host, int L, const float* rescaler,
                           float* state, int64_t B, int F, int nt, int nx, int pad_t, int pad_x, int H0, int W0, int T0, wdno_stream_t s);
/* The two-level state of the super-resolution models for a batch, one launch (Smoke_wave.__getitem__ with is_super_model):
 *   state[b][f][c][h][w] = value / rescaler[c],   state [B][pad_t][16 F + 2][pad_x][pad_x]; everything not listed is 0
 *   c <  8 F          : fine (level l, [.][F][8][nt][nx][nx]) with one replicated border coefficient
 *                       time : fine[c][clamp(f - 1, 0, nt - 1)][h][w]                                  for f < nt + 2, h, w < nx
 *                       space: fine[c][f][clamp(h - 1, 0, nx - 1)][clamp(w - 1, 0, nx - 1)]            for f < nt, h, w < nx + 2
 *   8 F <= c < 16 F   : coarse (level l + 1, [.][F][8][nt_c][nx_c][nx_c]), nearest x2 (upsample_coef), cc = c - 8 F
 *                       time : coarse[cc][f >> 1][h][w]                                                for f < nt + 2, h, w < nx
 *                       space: coarse[cc][f][h >> 1][w >> 1]                                           for f < nt, h, w < nx + 2
 *   c == 16 F, 16 F + 1: the two condition channels of wdno_pack_smoke_state, from level l, without the border offset
 * sim = idx[b] (NULL: b) and the per-simulation strides as in wdno_pack_smoke_state. IEEE division: bit-identical to the torch formulation.
 * WDNO_EINVAL unless (time) nt + 2 == 2 nt_c, nx_c == nx, nt + 2 <= pad_t, nx <= pad_x / (space) nx + 2 == 2 nx_c, nt_c == nt, nx + 2 <= pad_x,
 * nt <= pad_t, and for another `kind`; WDNO_EUNSUPPORTED unless pad_t % 4 == 0 and pad_x % 4 == 0. Nothing is launched then. */
enum { WDNO_PACK_SUPER_TIME = 0, WDNO_PACK_SUPER_SPACE = 1 };
int wdno_pack_smoke_super_state(const float* fine, int64_t fine_sim_stride, const float* coarse, int64_t coarse_sim_stride,
                                const float* init_coef, int64_t init_sim_stride, const float* smokeout, int64_t so_sim_stride,
                                const int64_t* idx, const float* rescaler, float* state, int64_t B, int F, int nt, int nx, int nt_c,
                                int nx_c, int kind, int pad_t, int pad_x, wdno_stream_t s);
/* Dataset packing of the Burgers wavelet models for a batch, one launch (get_wavelet_super_preprocess of burgers/ddpm_burgers/data_burgers_1d.py:
 * 40-88) that writes every element of
 *   state[b][c][h][w] = value / rescaler[c],   state [B][C][pad_t][pad_x], C = 8 + 8 has_low + (cond_u0 | cond_uT); everything not listed is 0
 *   c < 8             : fine[sim][c / 4][c % 4][h][w] for h < nt, w < nx                     (fine [.][2][4][nt][nx]: the sub-bands of u, then of f)
 *                       has_low: row h == nt repeats row nt - 1 (the reference's "odd number of timesteps" line)
 *   8 <= c < 16       : has_low: coarse[sim][(c - 8) / 4][(c - 8) % 4][h >> 1][w >> 1] for h < 2 nt_c, w < 2 nx_c   (upsample_coef, not cropped)
 *   c == C - 1        : cond_u0 | cond_uT: four stripes of pad_t / 4 rows, w < nx -- the low band of u(t = 0), its high band, the low band of
 *                       u(t = ori_t - 1), its high band: the one-level periodized 1-D analysis along x of that row of u, the row itself
 *                       synthesised inside the launch from the four sub-bands of u (periodized 2-D synthesis of that output row only). A
 *                       stripe whose flag is off is zero. The sums run in the order of the transform kernels (wdno_dwt_inv, wdno_dwt_fwd).
 * sim = idx[b] (device int64; NULL: b); the per-sample strides of the two levels are in elements. dec_* / rec_*: the wavelet's filters, host
 * arrays of L taps (read only with a condition channel). IEEE division: channels below the condition channel carry the bits of the torch
 * formulation. Returns, without a launch: WDNO_EINVAL when the box (nt <= pad_t, nx <= pad_x), the repeated row (nt + 1 <= pad_t) or the doubled
 * coarse block (2 nt_c <= pad_t, 2 nx_c <= pad_x) does not fit, for ori_t outside [1, 2 nt], strides smaller than a sample, flags other than
 * 0 / 1 or a state that is not 16-byte aligned; WDNO_EUNSUPPORTED unless pad_t % 4 == 0, pad_x % 4 == 0, ori_x == 2 nx, L even and <= 16 (and
 * pad_t, pad_x <= 4096, B <= 65535). Periodization only. Nothing is allocated. */
int wdno_pack_burgers_state(const float* fine, int64_t fine_sim_stride, const float* coarse, int64_t coarse_sim_stride, const int64_t* idx,
                            const float* rescaler, float* state, int64_t B, int nt, int nx, int nt_c, int nx_c, int pad_t, int pad_x,
                            int ori_t, int ori_x, int has_low, int cond_u0, int cond_uT, const float* dec_lo_host, const float* dec_hi_host,
                            const float* rec_lo_host, const float* rec_hi_host, int L, wdno_stream_t s);
/* What that launch does for these integers (nothing is launched, no device is needed; the entry asks the same code): fine_vec / coarse_vec = floats
 * per load of the fine / coarse rows (4: nx % 4 == 0; 2: even rows; 1 otherwise -- strides and addresses permitting; align_mask: the addresses of
 * fine | coarse | state OR-ed), the grid (256 threads per block), the dynamic LDS and C. rc = the code the launch would return short of
 * WDNO_ELAUNCH and the NULL checks; the other fields are 0 then. Returns WDNO_EINVAL only for out == NULL. */
typedef struct { int fine_vec, coarse_vec, grid_x, grid_y, grid_z, lds_bytes, rc, reserved; } wdno_pack_burgers_plan;
int wdno_pack_burgers_plan_query(int64_t fine_sim_stride, int64_t coarse_sim_stride, int64_t B, int nt, int nx, int nt_c, int nx_c, int pad_t,
                                 int pad_x, int ori_t, int ori_x, int has_low, int cond_u0, int cond_uT, int L, unsigned align_mask,
                                 wdno_pack_burgers_plan* out);

/* ------------------------------------------------------------------------------------------------ layout
 * API layout [N, C, S] (S = product of spatial dims) <-> channels-last [N, S, Cp] (Cp >= C, zero padded). */
int wdno_nc_to_cl(const float* src, float* dst, int64_t N, int C, int64_t S, int Cp, wdno_stream_t s);
int wdno_cl_to_nc(const float* src, float* dst, int64_t N, int C, int64_t S, int Cp, wdno_stream_t s);
/* (a | b) delivered only as the fp16 planes [P][Ca + Cb] (lo == NULL: one bf16 plane) of the convolutions that read it -- the up-path
 * torch.cat((x, h.pop()), dim=1) of conv3d.py:340-346 / unet.py:268-274, read by the next ResnetBlock's first convolution and 1 x 1 skip
 * projection only. Scale from the amax records of a and b (left in scale_out[0]). Ca, Cb multiples of 8. */
int wdno_concat2_cl_planes(const float* a, int Ca, const float* b, int Cb, const float* rec_a, const float* rec_b, void* hi, void* lo,
                           float* scale_out, int64_t P, wdno_stream_t s);
int wdno_concat2_cl(const float* a, int Ca, const float* b, int Cb, float* out, int64_t P, wdno_stream_t s);
int wdno_concat2_cl_amax(const float* a, int Ca, const float* b, int Cb, float* out, float* amax_rec, int64_t P, wdno_stream_t s);
int wdno_split2_cl(const float* in, float* a, int Ca, float* b, int Cb, int64_t P, wdno_stream_t s);
/* nearest x2 in H and W of CL [N, H, W, C] (nn.Upsample, burgers/ddpm_burgers/unet.py:35-39) and its adjoint */
int wdno_upsample2x_cl_fwd(const float* in, float* out, int64_t N, int H, int W, int C, wdno_stream_t s);
int wdno_upsample2x_cl_bwd(const float* dout, float* din, int64_t N, int H, int W, int C, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ convolution
 * Implicit-GEMM convolution on MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate).
 * Replaces nn.Conv2d / nn.Conv3d / nn.ConvTranspose3d / nn.Linear forward, data-gradient and weight-gradient
 * (burgers/ddpm_burgers/unet.py:133,162,190-192,233-234,317,336,361,369 ;
 *  smoke/.../video_diffusion_pytorch_conv3d.py:159-163,192,216,238-239,291-292,393,471).
 *
 * Input x is CL [N, D, H, W, C] (C % 4 == 0). Weights are pre-packed as wp[kd][kh][K][kw*C] (innermost run
 * kw*C is contiguous in both x and wp). Output pixel (n, od, oh, ow) reads input rows
 *   d = od*sd - pd + dz, h = oh*sh - ph + dy, w = ow*sw - pw + dx
 * and is stored at physical position (n, od*osd+ood, oh*osh+ooh, ow*osw+oow) of y [N, YD, YH, YW, K]
 * (the placement terms express the 4 parity classes of a stride-2 transposed convolution).
 */
typedef struct {
  int N, D, H, W, C;
  int OD, OH, OW, K;
  int kd, kh, kw;
  int sd, sh, sw;
  int pd, ph, pw;
  int YD, YH, YW;
  int osd, osh, osw, ood, ooh, oow;
} wdno_conv_geom;
/* y = conv(x, wp) (+ bias[K]) (+ residual, same layout as y). bias/residual may be NULL. */
int wdno_conv_fwd(const float* x, const float* wp, const float* bias, const float* residual, float* y,
                  const wdno_conv_geom* g, wdno_stream_t s);
/* fp32-equivalent convolution on the fp16 matrix cores ("3 x fp16 split", conv_h3.hip): an fp32 tensor is pre-split by
 * wdno_amax_record + wdno_split_f16 into two fp16 planes hi, lo [rows][C8] (C8 = C rounded up to 8) and a power-of-two scale;
 * wdno_conv_fwd_f16x3 evaluates ah*bh + ah*bl + al*bh with fp32 accumulation. Same geometry contract as wdno_conv_fwd
 * with g->C = C8; sx / sw are the device scalars written by wdno_split_f16 for the activation / packed-weight operand. */
int wdno_amax(const float* x, int64_t n, float* amax_zeroed, wdno_stream_t s);            /* one float (weights) */
int wdno_amax_record(const float* x, int64_t n, float* rec_zeroed, wdno_stream_t s);     /* an amax record (activations) */
/* amax_rec: the amax record of x (from wdno_amax_record or from the kernel that produced x) */
int wdno_split_f16(const float* x, const float* amax_rec, void* hi, void* lo, float* scale_out, int64_t rows, int C, int C8, wdno_stream_t s);
/* wdno_split_f16 that also returns colsum_out[C8] = sum over rows (the bias gradient when x is dy), in the same pass.
 * WDNO_EUNSUPPORTED unless C8 / 8 is a power of two <= 256 (use wdno_split_f16 + wdno_colsum then).
 * colsum_out == NULL (here and in wdno_cast_bf16_colsum): only the partials are written -- doubles [ws_bytes / (8 C8)][C8] in ws -- and the
 * caller sums them later (wdno_rows_sum_multi, is_double = 1). */
size_t wdno_split_colsum_ws_bytes(int64_t rows, int C8);
int wdno_split_f16_colsum(const float* x, const float* amax_rec, void* hi, void* lo, float* scale_out, float* colsum_out,
                          void* ws, size_t ws_bytes, int64_t rows, int C, int C8, wdno_stream_t s);
/* raw weight [K][C][kd][kh][kw] -> split planes of the packed operand in one launch. mode 0: forward operand
 * [kd][kh][A>=K][kw][B>=C]; mode 1: data-gradient operand [kd][kh][A>=C][kw][B>=K] with flipped taps. amax = max|w| (device).
 * modes 2 + 2 py + px: forward operand of parity class (py, px) of the (1,4,4) / stride (1,2,2) transposed convolution (the stride-1
 * (1,2,2) convolution that produces the output pixels of that parity; Upsample of video_diffusion_pytorch_conv3d.py:96-98), gathered
 * from the ConvTranspose3d weight w[C = in][K = out][1][4][4] itself; kd, kh, kw = 1, 2, 2.
 * modes 10 / 11: the forward operand of a 1 x 1 projection -- to_qkv [A = 384][B = C] / to_out [A = C][B = 128] of a temporal attention block with
 * 4 heads of 32 -- in the FRAGMENT ORDER wdno_tattn_fused_fwd reads at C = 128 / 256 (csrc/attn_fused_wide.hip streams its weights: the 64 lanes of
 * one matrix-operand load then read 1 KB of contiguous memory). Same bytes as mode 0, 16-byte groups permuted (csrc/conv_prep.hip: pack_split_body). */
int wdno_pack_split_weight(const float* w, const float* amax, void* hi, void* lo, float* scale_out, int K, int C, int kd, int kh, int kw,
                           int A, int B, int mode, wdno_stream_t s);
/* Multi-tensor forms of wdno_amax and wdno_pack_split_weight for the per-step refresh of all weights: one launch for any
 * number of items, arguments in a device-resident table (all pointers are device pointers). amax outputs must be zeroed. */
typedef struct { const void* x; int64_t n; void* out; } wdno_amax_item;
typedef struct {
  const void* w; const void* amax; void* hi; void* lo; void* scale_out;
  int K, C, kd, kh, kw, A, B, mode;
} wdno_wsplit_item;
int wdno_amax_multi(const void* table, int n_items, int blocks_per_item, wdno_stream_t s);
int wdno_pack_split_weight_multi(const void* table, int n_items, int blocks_per_item, wdno_stream_t s);
int wdno_conv_fwd_f16x3(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                        const float* bias, const float* residual, float* y, const wdno_conv_geom* g, wdno_stream_t s);
/* the same, and max|y| over the outputs this launch wrote is merged into amax_rec (an amax record, or NULL) */
int wdno_conv_fwd_f16x3_amax(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                             const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g,
                             wdno_stream_t s);
/* Structural zeros of the activation operand, stated by the caller: x[n][d][h][w][c] == 0 for every c < channels at every pixel with d >= d0
 * or h >= h0 or w >= w0 (the zero padding of the wavelet-coefficient channels that p_losses / the sampler impose, smoke/ddpm/diffusion_2d.py:
 * 1008-1033: 18 x 34 x 34 coefficients in a 24 x 40 x 40 tensor). A hint about DATA: results are those of the plain entry points bit for bit
 * (a skipped term is an exact zero); a kernel that can use it -- the 7 x 7 x 7 stem of the smoke U-Net, video_diffusion_pytorch_conv3d.py:393 --
 * does not run the reduction stages of whole 16-channel blocks below `channels` whose source plane or row is >= d0 / h0 for every pixel of a tile. */
typedef struct { int channels, d0, h0, w0; } wdno_zero_box;
int wdno_conv_fwd_f16x3_zbox(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                             const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g,
                             const wdno_zero_box* zb, wdno_stream_t s);
/* single-product (bf16) form with both options: zb may be NULL; y_bf16 != 0: y is bf16 storage [rows][K] (round-to-nearest-even of the fp32
 * result; residual must be NULL) -- mixed-precision activation storage between a convolution and the GroupNorm that is its only reader
 * (burgers/ddpm_burgers/train_diffusion.py:61-62: accelerate mixed precision), read by the wdno_groupnorm_*_t entry points. */
int wdno_conv_fwd_bf16_ex(const void* x16, const void* wp16, const float* bias, const float* residual, void* y, int y_bf16, float* amax_rec,
                          const wdno_conv_geom* g, const wdno_zero_box* zb, wdno_stream_t s);
/* the same with a caller-lent workspace: layers of few pixels x many channels (the 8 x 8 / 16 x 16 levels of the Burgers U-Net, unet.py:150-181)
   cut the reduction of a tile into four runs of stages, one block each; the runs' partial sums go through `ws` and are added in a fixed order.
   wdno_conv_fwd_split_ws_bytes(g): bytes such a geometry wants (0 = it never splits; ws may then be NULL). */
int wdno_conv_fwd_f16x3_ws(const void* xh, const void* xl, const float* sx, const void* wph, const void* wpl, const float* sw,
                           const float* bias, const float* residual, float* y, float* amax_rec, const wdno_conv_geom* g,
                           void* ws, size_t ws_bytes, wdno_stream_t s);
size_t wdno_conv_fwd_split_ws_bytes(const wdno_conv_geom* g);
/* Plan queries: which kernel the entry points above (and the weight-gradient ones below) would launch for a geometry, under the current debug
 * mode. They launch nothing; the launch paths call the same choosing code. CU-dependent choices use the current device's CU count (256 when
 * there is no device). lowp: 0 = (hi, lo) fp16 planes, 1 = single bf16 planes. residual_is_y: the residual operand is y itself (accumulation in place: the
 * only way a residual changes the choice -- the two-block ksplit form adds onto zeroed outputs and is not taken then). split_ws_bytes:
 * the workspace the caller would lend (wdno_conv_fwd_f16x3_ws), 0 = none.
 * lowp < 0 asks about the exact-fp32 entry point wdno_conv_fwd (family WDNO_CONV_FP32, its tile); the same is reported where the split entry
 * points refuse the geometry (C % 8 != 0) and the caller has to run wdno_conv_fwd.
 * uniform: chunked DMA kernels only -- 1 = whole 32-channel blocks (one channel-block index per step), 0 = per-lane channel blocks; the
 * tap-resident kernels always work on whole blocks (1), the others report 0. grid = blocks of the first grid dimension (the register-staged
 * kernels add ksplit as the second); ntiles = pixel tiles x channel tiles. */
enum { WDNO_CONV_FP32 = 0, WDNO_CONV_REG_H3 = 1, WDNO_CONV_CHUNKED_H3D = 2, WDNO_CONV_TAP_H3T = 3, WDNO_CONV_STEM_H3T = 4 };
typedef struct { int family, bm, bn, uniform, tsplit, ksplit, ntiles, grid; } wdno_conv_plan;
int wdno_conv_fwd_plan(const wdno_conv_geom* g, int lowp, int residual_is_y, size_t split_ws_bytes, wdno_conv_plan* out);
/* family: register-staged (conv_wgrad_h3_kernel), chunked DMA (h3d), window (h3w, 3-wide taps on whole 64-channel tiles) or stem (h3s, 7-wide).
 * reduce_tiled: the split reduction into the parameter layout dw[Kn][Cn][..] is the tiled one (Kn / Cn <= 0: g->K / g->C). items = work items
 * of the launch, grid = its blocks (first dimension; the register-staged kernels add `splits` as the second). */
enum { WDNO_WGRAD_REG_H3 = 0, WDNO_WGRAD_CHUNKED_H3D = 1, WDNO_WGRAD_WINDOW_H3W = 2, WDNO_WGRAD_STEM_H3S = 3 };
typedef struct { int family, bm, bn, splits, pix_per_split, splitpair, reduce_tiled, items, grid; } wdno_wgrad_plan;
int wdno_conv_wgrad_plan(const wdno_conv_geom* g, int lowp, int Kn, int Cn, wdno_wgrad_plan* out);
/* weight gradient on the same split planes (g->C = C8 of x, g->K = K8 of dy); dwp [kd][kh][K8][kw*C8] fp32 */
size_t wdno_conv_wgrad_f16x3_ws_bytes(const wdno_conv_geom* g);
/* pixel_table: [N*OD*OH*OW] 16-byte records from wdno_conv_pixel_table (depends on the geometry only; callers cache it) */
int wdno_conv_pixel_table(void* table, const wdno_conv_geom* g, wdno_stream_t s);
int wdno_conv_wgrad_f16x3(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                          const void* pixel_table, float* dwp, void* ws, size_t ws_bytes, const wdno_conv_geom* g, wdno_stream_t s);
/* Same, with the result in the layout of the parameter: dw[Kn][Cn][kd][kh][kw] (Kn <= g->K, Cn <= g->C; channel padding dropped),
 * written by the split reduction itself. ws >= wdno_conv_wgrad_f16x3_ws_bytes(g) always (also when there is one split). */
int wdno_conv_wgrad_f16x3_param(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                                const void* pixel_table, float* dw, int Kn, int Cn, void* ws, size_t ws_bytes,
                                const wdno_conv_geom* g, wdno_stream_t s);
/* The same weight gradient in two steps, for callers that collect the split reductions of a whole backward pass (autograd through every
 * nn.Conv*d of the U-Nets, unet.py:129-259 / conv3d.py:189-230: only the optimiser reads a weight gradient): wdno_conv_wgrad_partials runs the
 * partial-sum kernels into ws ([splits][kd*kh][K8][kw*C8]) and fills `item`; wdno_wgrad_reduce_multi then performs the ordered reductions of any
 * number of items in one launch (items travel by value in the kernel arguments: no table upload, capturable in a HIP graph) -- the same additions
 * in the same order as wdno_conv_wgrad_f16x3_param / _bf16_param, i.e. bit-identical results. ws must stay alive and unmodified in between.
 * xl == NULL (and sx == sdy == NULL): single bf16 planes. `items` is a HOST array. */
#define WDNO_WGRAD_REDUCE_MAX 40
typedef struct wdno_wgrad_reduce_item {
  const float* ws; float* dw;      /* partial sums [splits][n]; destination in the parameter's layout dw[Kn][Cn][kd][kh][kw] */
  int n, splits;                   /* n = kd*kh*K8*kw*C8 */
  int K8, C8, kw, ntap, Kn, Cn;
  int tiled;                       /* which of the two reduction bodies (chosen by the library) */
  int reserved;
} wdno_wgrad_reduce_item;
int wdno_conv_wgrad_partials(const void* xh, const void* xl, const float* sx, const void* dyh, const void* dyl, const float* sdy,
                             const void* pixel_table, float* dw, int Kn, int Cn, void* ws, size_t ws_bytes,
                             const wdno_conv_geom* g, wdno_wgrad_reduce_item* item, wdno_stream_t s);
int wdno_wgrad_reduce_multi(const wdno_wgrad_reduce_item* items, int n_items, wdno_stream_t s);
/* dwp[kd][kh][K][kw*C] = sum over output pixels of dy (x) shifted x. ws: caller workspace. */
size_t wdno_conv_wgrad_ws_bytes(const wdno_conv_geom* g);
int wdno_conv_wgrad(const float* x, const float* dy, float* dwp, void* ws, size_t ws_bytes,
                    const wdno_conv_geom* g, wdno_stream_t s);
/* The sums over rows that END a backward pass -- bias gradients from the column-sum partials of a dy sweep, GroupNorm's d(gamma) / d(beta) from the
 * per-sample pieces -- feed parameters only (nn.Conv*d.bias, nn.GroupNorm.weight / .bias: unet.py:129-181, conv3d.py:189-204), so a caller may
 * collect them and run ONE launch when the backward has returned: out[j] = sum_r part[r * stride + col0 + j], j < ncols, fp64 accumulation in the
 * fixed order of the single-tensor launches they replace (partial_rows_sum: bit-identical). `items` is a HOST array (they travel by value in the
 * kernel arguments); the partial matrices must stay alive and unmodified until the launch has run. */
#define WDNO_ROWS_SUM_MAX 64
typedef struct wdno_rows_sum_item {
  const void* part; float* out;
  int rows, stride, col0, ncols;
  int is_double, reserved;
} wdno_rows_sum_item;
int wdno_rows_sum_multi(const wdno_rows_sum_item* items, int n_items, wdno_stream_t s);
/* out[C] = sum_p in[p][C]  (bias gradients and other per-channel reductions). ws >= wdno_colsum_ws_bytes. */
size_t wdno_colsum_ws_bytes(int64_t P, int C);
int wdno_colsum(const float* in, float* out, int64_t P, int C, void* ws, size_t ws_bytes, wdno_stream_t s);

/* ---- single-product bf16 convolutions (BASELINE.json configs[1]: "bf16 on 1 x MI355X, batch 256"; the reference's knob is
 * Trainer(amp=True, mixed_precision_type=...) burgers/ddpm_burgers/train_diffusion.py:62,71-74). Activations, weights and output
 * gradients are rounded to ONE bf16 plane [rows][C8] (round-to-nearest-even, no scale) and multiplied on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulators; master weights, bias, residual, outputs and all reductions stay fp32.
 * Same geometry contract and packed-weight layout as the f16x3 entry points (pack with wdno_pack_split_weight and lo == NULL,
 * amax == NULL, scale_out == NULL: one bf16 plane in `hi`; wdno_wsplit_item likewise). Accuracy is bf16-class (2^-8 per
 * operand): tests/test_gpu_bf16.py documents the tolerance against the oracle; it cannot meet the fp32 path's 1e-5. */
int wdno_cast_bf16(const float* x, void* out16, int64_t rows, int C, int C8, wdno_stream_t s);
int wdno_cast_bf16_colsum(const float* x, void* out16, float* colsum_out, void* ws, size_t ws_bytes, int64_t rows, int C, int C8, wdno_stream_t s);
int wdno_conv_fwd_bf16(const void* x16, const void* wp16, const float* bias, const float* residual, float* y, float* amax_rec,
                       const wdno_conv_geom* g, wdno_stream_t s);
/* dw[Kn][Cn][kd][kh][kw] (the parameter's layout); workspace size = wdno_conv_wgrad_f16x3_ws_bytes(g) */
int wdno_conv_wgrad_bf16_param(const void* x16, const void* dy16, const void* pixel_table, float* dw, int Kn, int Cn, void* ws,
                               size_t ws_bytes, const wdno_conv_geom* g, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ normalisation
 * GroupNorm (+ optional (scale+1, shift) modulation) + optional SiLU on CL [N, S, C]:
 *   y = act( (GN(x)*gamma + beta) * (ss[n, c] + 1) + ss[n, C + c] ),  ss = [N, 2C] or NULL.
 * burgers/ddpm_burgers/unet.py:139-148 ; smoke/.../video_diffusion_pytorch_conv3d.py:196-204.
 * stats [N, G, 2] (mean, rstd) is written by fwd and read by bwd.
 */
size_t wdno_groupnorm_ws_bytes(int64_t N, int64_t S, int C, int G);
/* Round 3: `stats` of every GroupNorm entry point is a buffer of wdno_groupnorm_stats_floats(N, C, G) floats: the [N][G] (mean, rstd) pairs
 * followed by the per-channel / per-group tables the forward derives from them, which the backward entry points read back (one launch
 * fewer per norm). The forward that wrote it and the backward that reads it must see the same gamma / beta / scale_shift. */
size_t wdno_groupnorm_stats_floats(int64_t N, int C, int G);
int wdno_groupnorm_act_fwd(const float* x, const float* gamma, const float* beta, const float* ss, float* y,
                           float* stats, int64_t N, int64_t S, int C, int G, float eps, int silu,
                           void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_groupnorm_act_fwd_amax(const float* x, const float* gamma, const float* beta, const float* ss, float* y,
                                float* stats, float* amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                void* ws, size_t ws_bytes, wdno_stream_t s);
/* dx, dgamma_beta_partial [N, 2, C] (per-sample; caller sums over N), dss [N, 2C] or NULL */
int wdno_groupnorm_act_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* ss,
                           const float* stats, float* dx, float* dgb_partial, float* dss,
                           int64_t N, int64_t S, int C, int G, int silu, void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_groupnorm_act_bwd_amax(const float* x, const float* dy, const float* gamma, const float* beta, const float* ss,
                                const float* stats, float* dx, float* dgb_partial, float* dss, float* amax_rec,
                                int64_t N, int64_t S, int C, int G, int silu, void* ws, size_t ws_bytes, wdno_stream_t s);
/* The same backward with dx delivered as the fp16 (hi, lo) planes the split convolution kernels read (dx of the norm is the dy of
 * the convolution in front of it, Block.forward: unet.py:80-101, conv3d.py:186-206) -- no fp32 dx, no separate amax / split passes.
 * The scale comes from an upper bound of max|dx| that the per-sample finalize derives from per-channel maxima of the reduction pass
 * (bound_rec: a zeroed amax record, receives the bound). dx_colsum [C] = column sums of dx (the bias gradient of that convolution).
 * C / 8 must be a power of two <= 256 (WDNO_EUNSUPPORTED otherwise: use wdno_groupnorm_act_bwd_amax + wdno_split_f16). */
size_t wdno_groupnorm_bwd_planes_ws_bytes(int64_t N, int64_t S, int C, int G);
/* Forward with y delivered as planes (the output of block1 of a ResnetBlock, read by block2's convolution only: unet.py:103-118,
 * conv3d.py:208-230); scale from the bound max|a| max|x| + max|b| of the folded per-channel affine. Same channel restriction. */
size_t wdno_groupnorm_fwd_planes_ws_bytes(int64_t N, int64_t S, int C, int G);
int wdno_groupnorm_act_fwd_planes(const float* x, const float* gamma, const float* beta, const float* ss, void* y_hi, void* y_lo,
                                  float* y_scale, float* stats, float* bound_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                  void* ws, size_t ws_bytes, wdno_stream_t s);
/* y = act(GroupNorm(x)) + residual as BOTH the fp32 tensor y and its planes: the tail of a ResnetBlock with an identity skip
 * (unet.py:167-176, conv3d.py:286-300: `h + self.res_conv(x)` with res_conv = Identity), whose sum is the next block's skip and the
 * operand of its first convolution. res_rec = amax record of residual (the scale bound is the norm's bound + max|residual|);
 * y_amax_rec (optional) receives the amax record of y. y_hi == NULL: the fp32 sum only (one pass instead of apply + add) for sums
 * whose reader is not a convolution. Workspace: wdno_groupnorm_fwd_planes_ws_bytes. */
int wdno_groupnorm_act_add_fwd_planes(const float* x, const float* gamma, const float* beta, const float* ss, const float* residual,
                                      const float* res_rec, float* y, void* y_hi, void* y_lo, float* y_scale, float* stats,
                                      float* bound_rec, float* y_amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                      void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_groupnorm_act_bwd_planes(const float* x, const float* dy, const float* gamma, const float* beta, const float* ss,
                                  const float* stats, void* dx_hi, void* dx_lo, float* dx_scale, float* dx_colsum,
                                  float* dgb_partial, float* dgb_sum, float* dss, float* bound_rec, int64_t N, int64_t S, int C, int G, int silu,
                                  void* ws, size_t ws_bytes, wdno_stream_t s);
/* dx_colsum == NULL in the two backward entry points: the column sums of dx are left as partials -- doubles [rows][C] at byte offset csp_offset of ws
 * (this call) -- for wdno_rows_sum_multi; likewise dgb_sum == NULL leaves the per-sample pieces dgb_partial [N][2 C] to be summed there. */
int wdno_groupnorm_bwd_planes_tail(int64_t N, int64_t S, int C, int G, size_t* csp_offset, int* rows);
/* The same four entry points for bf16-stored activations (single-product mode): x_bf16 / dy_bf16 != 0 say that x / dy is bf16 storage -- what
 * wdno_conv_fwd_bf16_ex(y_bf16 = 1) wrote. Statistics, affine, activation and every output are computed exactly as above (fp32 / fp64). */
int wdno_groupnorm_act_fwd_amax_t(const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, float* y,
                                  float* stats, float* amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                  void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_groupnorm_act_fwd_planes_t(const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, void* y_hi, void* y_lo,
                                    float* y_scale, float* stats, float* bound_rec, int64_t N, int64_t S, int C, int G, float eps,
                                    int silu, void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_groupnorm_act_add_fwd_planes_t(const void* x, int x_bf16, const float* gamma, const float* beta, const float* ss, const float* residual,
                                        const float* res_rec, float* y, void* y_hi, void* y_lo, float* y_scale, float* stats,
                                        float* bound_rec, float* y_amax_rec, int64_t N, int64_t S, int C, int G, float eps, int silu,
                                        void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_groupnorm_act_bwd_planes_t(const void* x, int x_bf16, const void* dy, int dy_bf16, const float* gamma, const float* beta, const float* ss,
                                    const float* stats, void* dx_hi, void* dx_lo, float* dx_scale, float* dx_colsum,
                                    float* dgb_partial, float* dgb_sum, float* dss, float* bound_rec, int64_t N, int64_t S, int C, int G, int silu,
                                    void* ws, size_t ws_bytes, wdno_stream_t s);
/* dgb_sum (round 3, optional): [2 C] = the sum over the samples of dgb_partial [N][2][C] (d gamma | d beta), produced by the launch that
 * also finishes dx_colsum; NULL = the caller reduces dgb_partial itself. */
/* Channel LayerNorm over C of CL rows [P, C], gain only (unet.py:55-65, conv3d.py:165-174) */
int wdno_layernorm_fwd(const float* x, const float* g, float* y, int64_t P, int C, float eps, wdno_stream_t s);
int wdno_layernorm_fwd_amax(const float* x, const float* g, float* y, float* amax_rec, int64_t P, int C, float eps, wdno_stream_t s);
/* y as fp16 (hi, lo) planes for the to_qkv projection that is its only reader (PreNorm: unet.py:67-78, conv3d.py:176-184); the scale
 * follows from |y| <= sqrt(C) max|g|, no data pass. C must be a multiple of 8. */
int wdno_layernorm_fwd_planes(const float* x, const float* g, void* y_hi, void* y_lo, float* y_scale, int64_t P, int C, float eps,
                              wdno_stream_t s);
size_t wdno_layernorm_bwd_ws_bytes(int64_t P, int C);
int wdno_layernorm_bwd(const float* x, const float* g, const float* dy, float* dx, float* dg, int64_t P, int C,
                       float eps, void* ws, size_t ws_bytes, wdno_stream_t s);
/* the same with dx += add_to (the gradient that reaches x over the skip connection of Residual(PreNorm(fn)), unet.py:18-24,67-78,
 * conv3d.py:131-137,176-184): saves the separate accumulation pass autograd would issue. add_to may be NULL. */
int wdno_layernorm_bwd_add(const float* x, const float* g, const float* dy, const float* add_to, float* dx, float* dg, int64_t P, int C,
                           float eps, void* ws, size_t ws_bytes, wdno_stream_t s);
/* ... and max|dx| left in an amax record (dx is the dy of the projection in front of the next Residual block). amax_rec may be NULL. */
int wdno_layernorm_bwd_add_amax(const float* x, const float* g, const float* dy, const float* add_to, float* dx, float* dg, float* amax_rec,
                                int64_t P, int C, float eps, void* ws, size_t ws_bytes, wdno_stream_t s);
/* What the LayerNorm launches above do for P rows of C channels (nothing is launched; the launch path asks the same code): a row is held
 * by tpr lanes with vpl float4 each (lanes past C / 4 are masked), a block of 256 threads takes rows_per_block = 256 / tpr rows at a time
 * and walks the rows with a stride of blocks * rows_per_block: max_rows_walk = the most rows one row group visits (> 1 beyond 1024
 * blocks). rc = the code the launch would return: WDNO_EINVAL (P <= 0, C < 4), WDNO_EUNSUPPORTED (C % 4 != 0 or C > 1024; the planes
 * form also refuses C % 8 != 0). The other fields are 0 when rc != WDNO_OK. Returns WDNO_EINVAL only for out == NULL. */
typedef struct { int tpr, vpl, rows_per_block, blocks, max_rows_walk, rc; } wdno_ln_plan;
int wdno_layernorm_plan(int64_t P, int C, wdno_ln_plan* out);

/* ------------------------------------------------------------------------------------------------ attention
 * qkv rows are [row][3*heads*32] = (q | k | v), each [heads][32]; outputs are [row][heads*32].
 * Row index of (unit (uo, ui), token j) = uo*so + ui*si + j*st.
 *
 * Softmax attention over <= 1024 tokens (burgers unet.py:240-259 ; smoke conv3d.py:294-353): optional rotary
 * tables rot_cos/rot_sin [n][32] (q and k), optional additive bias [heads][n][n]; q is scaled by `scale`.
 */
typedef struct {
  int n_uo, n_ui, n_tok, heads;
  int64_t so, si, st;
} wdno_attn_desc;
int wdno_attn_fwd(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out,
                  const wdno_attn_desc* d, float scale, wdno_stream_t s);
/* out = the forward result (saved); dqkv (same layout as qkv); dbias [heads][n][n] (written, not accumulated) or NULL.
 * Token limits (WDNO_EUNSUPPORTED beyond; wdno_attn_bwd_plan reports the code without launching): n_tok <= 32 always (matrix kernels);
 * without rotation, bias and bias gradient n_tok <= 576; with rotation or bias above 32 tokens the thread-per-row kernel keeps K, Q, P and dS
 * of its items and the bias-gradient partial in LDS, ((2 + heads_if_dbias) n^2 + 66 n + 16) * 4 bytes <= 160 KB at one item per block:
 * n_tok <= 127 without a bias gradient, and with one n_tok <= 106 / 93 / 77 / 60 at 1 / 2 / 4 / 8 heads. The kernel takes 128 / n_tok items
 * per block where that fits and fewer where it does not (64 tokens, 4 heads and a bias gradient: one item instead of two).
 * The relative-position-bias gradient is DETERMINISTIC: every block leaves its partial sum in the workspace (wdno_attn_bwd_ws_bytes,
 * needed only when dbias != NULL) and a second launch adds the partials in block order; with heads == 4 and n_tok <= 32 a wave sums
 * its items in registers in item order. Inside a block no address of the partial has two writers: the matrix kernel gives every wave a
 * partial of its own when heads % 4 != 0, the thread-per-row kernel takes at most `heads` items per block when there is a bias gradient.
 * THE EXCEPTION: up to 32 tokens with heads % 4 != 0 where four partials do not fit the 160 KB of LDS (from 9 heads on at 32 tokens) the waves
 * share one partial and two of them add to one address in arrival order: dbias may then differ in its last bits between two runs
 * (wdno_attn_bwd_plan reports dbias_in_lds = 2 for such a launch). */
size_t wdno_attn_bwd_ws_bytes(const wdno_attn_desc* d);
int wdno_attn_bwd(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out,
                  const float* dout, float* dqkv, float* dbias, const wdno_attn_desc* d, float scale, void* ws, size_t ws_bytes,
                  wdno_stream_t s);
/* the same with an amax record (or NULL) for the tensor written: out / dqkv */
int wdno_attn_fwd_amax(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out, float* amax_rec,
                       const wdno_attn_desc* d, float scale, wdno_stream_t s);
int wdno_attn_bwd_amax(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out,
                       const float* dout, float* dqkv, float* dbias, float* amax_rec, const wdno_attn_desc* d, float scale,
                       void* ws, size_t ws_bytes, wdno_stream_t s);
/* The same with dqkv delivered as fp16 (hi, lo) planes [rows][3*heads*32] for the gradient kernels of the qkv projection (its only
 * reader: conv3d.py:232-300). The scale is derived in the kernel from the amax records of qkv and dout (an upper bound of max|dqkv|,
 * see csrc/attention.hip) and left in dqkv_scale[0]. n_tok <= 32 only (WDNO_EUNSUPPORTED otherwise). */
int wdno_attn_bwd_planes(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, const float* out,
                         const float* dout, void* dqkv_hi, void* dqkv_lo, float* dqkv_scale, float* dbias,
                         const float* rec_qkv, const float* rec_dout, const wdno_attn_desc* d, float scale, void* ws, size_t ws_bytes,
                         wdno_stream_t s);
/* Forward with out delivered ONLY as the fp16 planes of the to_out projection (|out| <= max|qkv|: scale from rec_qkv); `out` is not
 * written. n_tok <= 64 (WDNO_EUNSUPPORTED beyond). The n_tok <= 32 backward (wdno_attn_bwd*, MFMA path) does not read out: delta =
 * sum_j P dP is formed in registers; for 33..64 tokens the backward does read it, so a caller that needs gradients keeps the fp32 form
 * there (the super-resolution sampler, 48 frames, does not). */
int wdno_attn_fwd_planes(const float* qkv, const float* rot_cos, const float* rot_sin, const float* bias, float* out, void* out_hi,
                         void* out_lo, float* out_scale, float* amax_rec, const float* rec_qkv, const wdno_attn_desc* d, float scale,
                         wdno_stream_t s);
/* What wdno_attn_fwd* / wdno_attn_bwd* would launch (nothing is launched; the launch paths ask the same code, so the library debug modes
 * change the answers as they change the launches). has_rot / has_bias: tables given; want_dbias: dbias != NULL (backward); planes: the
 * *_planes form. family: WDNO_ATTN_*; grid: blocks; items_per_block: (unit, head) items a block holds at a time (waves of the matrix
 * kernels, item slots of the thread-per-row ones; tiled forward: (item, query tile) pairs); max_walk: the most items (pairs, item groups)
 * one wave / block visits with its grid stride; dbias_partials: rows of the workspace the dbias reduce sums (= grid when want_dbias);
 * dbias_in_lds: LDS arrays [heads][n][n] that hold the block's partial: 0 = registers of its waves (heads == 4 on the matrix kernel), 1 = one
 * array whose every address has a single writer (the thread-per-row kernel; the matrix kernel with heads a multiple of 4), 4 = one per wave,
 * added in wave order (the matrix kernel with any other head count), 2 = one array that two waves add to in arrival order (the matrix
 * kernel where heads % 4 != 0 and four arrays do not fit: not reproducible bit for bit); lds_bytes: dynamic LDS;
 * rc: the code the launch would return for these arguments, short of WDNO_EWORKSPACE / WDNO_ELAUNCH. Fields other than rc are 0 and family
 * is WDNO_ATTN_NONE when rc != WDNO_OK. The functions return WDNO_EINVAL only for out == NULL. */
enum { WDNO_ATTN_NONE = -1, WDNO_ATTN_MFMA24 = 0, WDNO_ATTN_MFMA = 1, WDNO_ATTN_MFMA64 = 2, WDNO_ATTN_TILED = 3, WDNO_ATTN_TILED_STAGED = 4,
       WDNO_ATTN_TILED_UNSTAGED = 5, WDNO_ATTN_BIG = 6, WDNO_ATTN_ROWS = 7 };
typedef struct { int family, grid, items_per_block, max_walk, dbias_partials, dbias_in_lds, lds_bytes, rc; } wdno_attn_plan;
int wdno_attn_fwd_plan(const wdno_attn_desc* d, int has_rot, int has_bias, int want_dbias, int planes, wdno_attn_plan* out);
int wdno_attn_bwd_plan(const wdno_attn_desc* d, int has_rot, int has_bias, int want_dbias, int planes, wdno_attn_plan* out);
/* Linear attention (unet.py:203-223 ; conv3d.py:241-258): q softmax over the 32 head channels, k softmax over
 * tokens, ctx = k^T v, out = ctx^T q * scale. units x n_tok rows, contiguous. ws holds k statistics and ctx. */
size_t wdno_linattn_ws_bytes(int64_t units, int heads);
int wdno_linattn_fwd(const float* qkv, float* out, float* kstats /*[units,heads,32,2]*/, float* ctx /*[units,heads,32,32]*/,
                     int64_t units, int n_tok, int heads, float scale, wdno_stream_t s);
int wdno_linattn_bwd(const float* qkv, const float* dout, const float* kstats, const float* ctx, float* dqkv,
                     void* ws, size_t ws_bytes, int64_t units, int n_tok, int heads, float scale, wdno_stream_t s);
int wdno_linattn_fwd_amax(const float* qkv, float* out, float* kstats, float* ctx, float* amax_rec, int64_t units, int n_tok, int heads,
                          float scale, wdno_stream_t s);
int wdno_linattn_bwd_amax(const float* qkv, const float* dout, const float* kstats, const float* ctx, float* dqkv, float* amax_rec,
                          void* ws, size_t ws_bytes, int64_t units, int n_tok, int heads, float scale, wdno_stream_t s);
/* The cuts of a linear-attention call (nothing is launched; the launch paths ask the same code). backward = 0: kstats_chunks = pieces of the
 * token range of the k statistics (n_tok / 64 within 1 .. 16; 0 for the backward, which reads kstats); ctx_chunks = pieces of the token range
 * of the context (the backward: of dctx; 1 when units * heads exceeds 2 x CUs, else at most n_tok / 128 and 16); token_tiles = blocks along the
 * tokens of the per-token kernel (128 tokens each; 64 for the thread-per-token family); family 0 = matrix kernels, 1 = thread per token
 * (debug mode 5). rc: the code the launch would return, WDNO_EWORKSPACE for a backward with ws_bytes below wdno_linattn_ws_bytes. */
typedef struct { int kstats_chunks, ctx_chunks, token_tiles, family, rc; } wdno_la_plan;
int wdno_linattn_plan(int64_t units, int n_tok, int heads, int backward, size_t ws_bytes, wdno_la_plan* out);
/* The same with dqkv delivered as fp16 (hi, lo) planes (see wdno_attn_bwd_planes); the scale bound uses the amax records of qkv and
 * dout and the measured max|dctx| (rec_dctx: a zeroed record the call fills). */
int wdno_linattn_bwd_planes(const float* qkv, const float* dout, const float* kstats, const float* ctx, void* dqkv_hi, void* dqkv_lo,
                            float* dqkv_scale, const float* rec_qkv, const float* rec_dout, float* rec_dctx, void* ws, size_t ws_bytes,
                            int64_t units, int n_tok, int heads, float scale, wdno_stream_t s);
/* Forward with out delivered ONLY as fp16 planes (the backward does not read out); |out| <= scale * max|qkv|. */
int wdno_linattn_fwd_planes(const float* qkv, void* out_hi, void* out_lo, float* out_scale, float* kstats, float* ctx,
                            const float* rec_qkv, int64_t units, int n_tok, int heads, float scale, wdno_stream_t s);

/* The whole temporal-attention block of the smoke U-Net's first level as ONE launch (csrc/attn_fused.hip): replaces
 * Residual(PreNorm(dim, EinopsToAndFrom('b c f h w', 'b (h w) f c', Attention(dim, heads, 32, rotary_emb)))) --
 * smoke/video_diffusion_pytorch/video_diffusion_pytorch_conv3d.py:165-174 (LayerNorm), :277-353 (Attention.forward: to_qkv, scale,
 * rotary, + pos_bias, softmax, to_out), :176-183 / :259-275 (PreNorm, the einops wrapper), Residual's add.
 *   x, y: CL [n_batch, n_tok, hw, C] fp32 (frames before pixels; y = x + to_out(attention(LayerNorm(x)))); gamma [C];
 *   wq_* / wo_*: the packed forward operands (fp16 hi / lo planes + scale) of to_qkv [3*heads*32][C] and to_out [C][heads*32] as
 *   wdno_pack_split_weight writes them; rot_cos / rot_sin [n_tok][32] or NULL; bias [heads][n_tok][n_tok] or NULL;
 *   amax_rec: optional amax record of y; qkv_out: optional [rows][3*heads*32] raw projections for a backward pass that wants them;
 *   rec_v: optional zeroed amax record that receives max|v| (wdno_tattn_fused_bwd: the plane scale of the attention output).
 * wdno_tattn_fused_takes: 1 for the shapes the kernels are built for (C = 64, 4 heads, 24 frames -- the base-resolution model -- or 48 --
 * the super-resolution model of inference_2d.py; 48 frames forward only: qkv_out must be NULL and wdno_tattn_fused_bwd refuses them; C = 128 /
 * 256 with 24 frames -- the deeper levels, csrc/attn_fused_wide.hip -- forward only, qkv_out must be NULL, rec_v is left untouched, and
 * wq_* / wo_* are the operands of pack modes 10 / 11), else 0 (callers then run the block layer by layer). */
int wdno_tattn_fused_takes(int C, int n_tok, int heads);
int wdno_tattn_fused_fwd(const float* x, const float* gamma, float eps, const void* wq_hi, const void* wq_lo, const float* wq_scale,
                         const void* wo_hi, const void* wo_lo, const float* wo_scale, const float* rot_cos, const float* rot_sin,
                         const float* bias, float* y, float* amax_rec, float* qkv_out, float* rec_v,
                         int64_t n_batch, int n_tok, int64_t hw, int C, int heads, float scale, wdno_stream_t s);
/* Backward of the same block as ONE launch + an ordered reduction (csrc/attn_fused_bwd.hip): the backward of conv3d.py:165-174 and
 * :277-353 through autograd in the reference. Only x is needed from the forward: LayerNorm, projections, scores and attention output
 * are recomputed per sequence.
 *   wq_*: the packed FORWARD operand of to_qkv (as in the forward), wo_*: the packed DATA-GRADIENT operand of to_out (W_out^T
 *   [heads*32][C], wdno_pack_split_weight mode 1); dy: gradient of y, CL like x; rec_dy: its amax record; rec_v: the record the forward
 *   launch filled;
 *   dx: gradient of x (the residual path included), amax_rec: optional amax record of dx;
 *   grads: wdno_tattn_fused_bwd_grads() floats = [ dW_qkv [3*heads*32][C] | dW_out [C][heads*32] | dgamma [C] | dbias [heads][n_tok][n_tok] ],
 *   each the sum over the launch's blocks of per-block partials in `ws` (wdno_tattn_fused_bwd_ws_bytes() bytes) taken in block order:
 *   two launches on the same inputs return the same bits. */
size_t wdno_tattn_fused_bwd_ws_bytes(void);
int wdno_tattn_fused_bwd_grads(void);
int wdno_tattn_fused_bwd(const float* x, const float* dy, const float* gamma, float eps, const void* wq_hi, const void* wq_lo,
                         const float* wq_scale, const void* wo_hi, const void* wo_lo, const float* wo_scale, const float* rot_cos,
                         const float* rot_sin, const float* bias, const float* rec_dy, const float* rec_v, float* dx, float* amax_rec,
                         float* grads, void* ws, size_t ws_bytes,
                         int64_t n_batch, int n_tok, int64_t hw, int C, int heads, float scale, wdno_stream_t s);
/* The grids those two calls launch for a shape (no device work; the tests' case matrices ask it which regime a shape reaches). Blocks walk the
 * n_batch * hw sequences with a stride of the grid: ceil(n_batch * hw / grid) passes, the sample advancing by grid / hw and the pixel by
 * grid % hw per step. grid_bwd = 0 where there is no fused backward (48 frames, 128 / 256 channels). WDNO_EUNSUPPORTED for shapes
 * wdno_tattn_fused_takes refuses. */
int wdno_tattn_fused_plan(int C, int n_tok, int64_t n_batch, int64_t hw, int* grid_fwd, int* grid_bwd);

/* The SpatialLinearAttention block of the 64-channel levels FORWARD, for passes that need no gradient (csrc/linattn_fused.hip): replaces
 * Residual(PreNorm(dim, SpatialLinearAttention(dim, heads))) -- smoke/video_diffusion_pytorch/video_diffusion_pytorch_conv3d.py:165-174
 * (LayerNorm), :232-258 (to_qkv, softmax over features / tokens, context, to_out) and Residual's add -- by two passes over the tokens and a
 * merge; the [rows][384] projections are never written.
 *   x, y: CL [units][n_tok][C] fp32 (units = batch * frames, n_tok = H * W); gamma [C]; wq_* / wo_*: packed forward operands of to_qkv
 *   [3*heads*32][C] and to_out [C][heads*32]; bias_out [C] or NULL; amax_rec: optional amax record of y; ws: wdno_lattn_fused_ws_bytes bytes;
 *   ctx_out [units][heads][32][32] / kstat_out [units][heads][2][32] (max over the tokens of k, 1 / Z): optional, what the backward call reads.
 * wdno_lattn_fused_takes: 1 for C = 64, 4 heads, n_tok >= 32. */
int wdno_lattn_fused_takes(int C, int heads, int n_tok);
size_t wdno_lattn_fused_ws_bytes(int64_t units, int n_tok);
int wdno_lattn_fused_fwd(const float* x, const float* gamma, float eps, const void* wq_hi, const void* wq_lo, const float* wq_scale,
                         const void* wo_hi, const void* wo_lo, const float* wo_scale, const float* bias_out, float* y, float* amax_rec,
                         float* ctx_out, float* kstat_out, void* ws, size_t ws_bytes, int64_t units, int n_tok, int C, int heads, float scale,
                         wdno_stream_t s);

/* Backward of the same block (csrc/linattn_fused_bwd.hip): one reduction pass over the tokens (dctx), a merge, one pass that recomputes the
 * projections per token tile and writes dx, and the ordered sum of the per-block weight-gradient partials. Needs x, the ctx / kstat tensors the
 * forward call left, dy with its amax record, the packed forward operand of to_qkv and the packed DATA-GRADIENT operand of to_out (W_out^T).
 *   grads: wdno_lattn_fused_bwd_grads() floats = [ dW_qkv [3*heads*32][C] | dW_out [C][heads*32] | dgamma [C] | db_out [C] ]. */
int wdno_lattn_fused_bwd_grads(void);
size_t wdno_lattn_fused_bwd_ws_bytes(int64_t units, int n_tok);
int wdno_lattn_fused_bwd(const float* x, const float* dy, const float* gamma, float eps, const void* wq_hi, const void* wq_lo,
                         const float* wq_scale, const void* wot_hi, const void* wot_lo, const float* wot_scale, const float* ctx,
                         const float* kstat, const float* rec_dy, float* dx, float* amax_rec, float* grads, void* ws, size_t ws_bytes,
                         int64_t units, int n_tok, int C, int heads, float scale, wdno_stream_t s);
/* The cuts wdno_lattn_fused_fwd / wdno_lattn_fused_bwd make for a shape (no device work): a frame's ceil(n_tok / 32) token tiles go to `chunks`
 * chunks of `tiles_per_chunk` tiles (forward passes and the backward's reduction pass, one block per (frame, chunk); trailing chunks may be
 * short or empty); the backward's last pass cuts them into `chunks2` of `tiles_per_chunk2` and runs the units * chunks2 items on `grid2`
 * persistent blocks -- also the number of partials its ordered reduction sums. */
int wdno_lattn_fused_plan(int64_t units, int n_tok, int* chunks, int* tiles_per_chunk, int* chunks2, int* tiles_per_chunk2, int* grid2);

/* relative-position bias of the temporal attention (conv3d.py:74-112): bias[h][i][j] = W[bucket[i][j]][h] with W [num_buckets, heads]
 * (nn.Embedding weight) and bucket [n, n] int64 (host-built integer table); and dW from d(bias). One launch each. */
int wdno_relpos_bias_fwd(const float* w, const int64_t* bucket, float* out, int n, int heads, wdno_stream_t s);
int wdno_relpos_bias_bwd(const float* dbias, const int64_t* bucket, float* dw, int n, int heads, int num_buckets, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ nn.Linear on a few rows
 * (time-embedding MLPs; conv3d.py:118-133, 286-296; unet.py:151-165). P <= 1024 rows, C % 4 == 0, strides in floats. The weight
 * is the reference's own [K][C] tensor (row stride w_stride), no packing. y [P][Kp] is zero in columns K..Kp-1. The data
 * gradient is the same call on the transposed weight. dw [K][C] contiguous; db [K] or NULL. */
int wdno_linear_rows_fwd(const float* x, int x_stride, const float* w, int w_stride, const float* bias, float* y, int P, int C, int K,
                         int Kp, wdno_stream_t s);
int wdno_linear_rows_wgrad(const float* x, int x_stride, const float* dy, int dy_stride, float* dw, float* db, int P, int C, int K,
                           wdno_stream_t s);

/* All projections of ONE input x [P][C] (contiguous) in one launch: the scale/shift projections of every ResnetBlock read the same
 * activated time embedding (conv3d.py:118-133 `self.mlp`, unet.py:151-165). The layers are a device-resident table; k_start = number of
 * output features of the layers before this one, F = their total. Outputs are concatenations:
 *   y  : block i = [P][K_i] at float offset P * k_start_i          dy: the same layout
 *   dw : [F][C] (rows k_start_i .. + K_i = the gradient of weight i),  db: [F]
 *   dx : [P][C] = sum over all layers; ws of wdno_linear_multi_dgrad_ws_bytes(F, P, C) bytes (partial sums, added in a fixed order). */
typedef struct wdno_linear_item {
  const void* w;        /* [K][C] fp32, contiguous */
  const void* bias;     /* [K] or NULL */
  int K, k_start;
} wdno_linear_item;
int wdno_linear_multi_fwd(const void* table, int n_items, int F, const float* x, float* y, int P, int C, wdno_stream_t s);
int wdno_linear_multi_wgrad(const void* table, int n_items, int F, const float* x, const float* dy, float* dw, float* db, int P, int C,
                            wdno_stream_t s);
size_t wdno_linear_multi_dgrad_ws_bytes(int F, int P, int C);
int wdno_linear_multi_dgrad(const void* table, int n_items, int F, const float* dy, float* dx, int P, int C, void* ws, size_t ws_bytes,
                            wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ pointwise
 * act: 0 = SiLU, 1 = GELU(erf). */
int wdno_act_fwd(const float* x, float* y, int64_t n, int act, wdno_stream_t s);
int wdno_act_bwd(const float* x, const float* dy, float* dx, int64_t n, int act, wdno_stream_t s);
int wdno_add(const float* a, const float* b, float* out, int64_t n, wdno_stream_t s);
int wdno_add_amax(const float* a, const float* b, float* out, float* amax_rec, int64_t n, wdno_stream_t s);
/* out[b, :] = cat(sin(t_b f_k), cos(t_b f_k)); freqs[dim/2] = exp(-k ln(theta)/(dim/2-1)) is a device table built by
 * the caller with the reference's own host arithmetic (unet.py:88-96, conv3d.py:144-151) */
int wdno_sinusoidal_emb(const int64_t* t, const float* freqs, float* out, int B, int dim, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ diffusion operator
 * All tensors in the reference's API layout: smoke [B, F, C, H, W]; Burgers [B, C, H, W] (F = 1).
 * Conditioning predicate descriptor (diffusion_2d.py:1008-1033 ; diffusion_1d.py:276-288, order pad,u0,uT,f,low):
 */
typedef struct {
  int tree;              /* 0 = smoke (wavelet), 1 = Burgers (wavelet) */
  int B, F, C, H, W;
  int cT, cH, cW;        /* padded_shape / coef_shape: valid coefficient extent (smoke: T',H',W'; Burgers: H',W') */
  int cond_pad, cond_a, cond_b, cond_c, cond_low;
  /* smoke  : cond_a = is_condition_control (channels 24:40), init-density channel C-2 is always conditioned;
   * Burgers: cond_a = u0, cond_b = uT, cond_c = f ; u0 rows [0, u_rows), uT rows [H-uT_rows, H) */
  int u_rows, uT_rows;
} wdno_cond_desc;
/* training: x = sqrt_ac[t_b]*x0 + sqrt_1mac[t_b]*noise, then conditions imposed on x (clean values from x0) and the
 * same regions of the target zeroed. x_out and target_out may not alias the inputs. */
int wdno_q_sample_cond(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac,
                       float* x_out, float* target_out, const wdno_cond_desc* c, wdno_stream_t s);
/* sampling: impose the conditions in place; `src` holds the clean values at conditioned positions (same shape as x) */
int wdno_apply_cond(float* x, const float* src, const wdno_cond_desc* c, wdno_stream_t s);
/* loss = sum_e (out-target)^2 * wc[c(e)] * wb[b(e)] * inv_count ; grad = dloss/dout (written if grad != NULL).
 * (diffusion_1d.py:640-645 ; diffusion_2d.py:1045-1050). loss is a device scalar. per_sample = F*C*H*W, inner = H*W; channel of element e = (e / inner) % C. */
int wdno_weighted_mse(const float* out, const float* target, const float* wc, const float* wb, float inv_count,
                      float* loss, float* grad, int64_t B, int64_t per_sample, int C, int64_t inner,
                      void* ws, size_t ws_bytes, wdno_stream_t s);
size_t wdno_weighted_mse_ws_bytes(int64_t n);
/* grad = d(loss)/d(out) * gscale[0] (gscale: device scalar = upstream gradient, NULL -> 1) */
int wdno_weighted_mse_bwd(const float* out, const float* target, const float* wc, const float* wb, float inv_count,
                          const float* gscale, float* grad, int64_t B, int64_t per_sample, int C, int64_t inner, wdno_stream_t s);
/* coefficient tables are the registered buffers [T]; t is per-sample [B].
 * p_sample (diffusion_1d.py:242-258 ; diffusion_2d.py:757-785): x_start = clamp(c1 x - c2 eps), mean = m1 x_start + m2 x,
 * x_next = mean + exp(0.5 logvar) * noise  (noise == NULL -> t == 0 step). */
int wdno_p_sample_update(const float* x, const float* eps, const float* noise, const int64_t* t,
                         const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* pm1, const float* pm2,
                         const float* plogvar, float* x_next, float* x_start, int64_t B, int64_t per_sample, int clamp, wdno_stream_t s);
/* DDIM (diffusion_1d.py:419-435 ; diffusion_2d.py:894-911): x_start = clamp(c1 x - c2 eps); eps' = (c1 x - x_start)/c2;
 * x_next = x_start*sqrt_an + c*eps' + sigma*noise. last step (noise == NULL): x_next = x_start. */
int wdno_ddim_update(const float* x, const float* eps, const float* noise, const int64_t* t,
                     const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, float sqrt_an, float c, float sigma,
                     float* x_next, float* x_start, int64_t B, int64_t per_sample, wdno_stream_t s);
/* the same update with (sqrt_an, c, sigma) read from three device floats: every step of a sampling loop is then the SAME launch,
 * which is what lets one captured HIP graph be replayed for the whole loop (diffusion_1d.py:376-460, diffusion_2d.py:851-933) */
int wdno_ddim_update_dev(const float* x, const float* eps, const float* noise, const int64_t* t,
                         const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* coef_dev,
                         float* x_next, float* x_start, int64_t B, int64_t per_sample, wdno_stream_t s);
/* What the launches above do (nothing is launched, no device is needed; the entry points ask the same code). Every operation has two forms:
 * WDNO_FORM_SCALAR, one element per work item with 64-bit index arithmetic on a grid of grid_x blocks (grid_y = 1), and WDNO_FORM_FLOAT4,
 * four elements per work item with 32-bit index arithmetic, for the loss and the updates with the sample on the grid's y axis (grid_y = B).
 * Blocks have 256 threads and walk the work items with a stride of grid_x * 256. align_mask: the addresses of the tensor operands the entry
 * point is given (not the tables, t or the scalars), OR-ed together; only the low four bits matter, a NULL operand adds nothing.
 *   wdno_cond_plan        : wdno_q_sample_cond (x0 | noise | x_out | target_out) and wdno_apply_cond (x | src). float4 needs W % 4 == 0,
 *                           fewer than 2^31 elements and 16-byte alignment.
 *   wdno_weighted_mse_plan: backward == 0 wdno_weighted_mse, else wdno_weighted_mse_bwd (out | target | grad). float4 needs inner % 4 == 0,
 *                           B <= 2048, 16-byte alignment and, forward, at least B doubles of workspace partials (stream grid of B * per_sample
 *                           not below B); the forward launch is followed by one block that adds the grid_x * grid_y partial sums. ws_bytes
 *                           is read by the forward only.
 *   wdno_update_plan      : wdno_p_sample_update, wdno_ddim_update, wdno_ddim_update_dev (x | eps | noise | x_next | x_start). float4 needs
 *                           per_sample % 4 == 0, B <= 65535 and 16-byte alignment.
 * rc = the code the launch would return for these arguments, short of WDNO_ELAUNCH and of the NULL checks of pointers the query does not see
 * (WDNO_EINVAL, WDNO_EWORKSPACE); the other fields are 0 then. The functions return WDNO_EINVAL only for out == NULL. */
enum { WDNO_FORM_SCALAR = 0, WDNO_FORM_FLOAT4 = 1 };
typedef struct { int form, grid_x, grid_y, rc; } wdno_diffusion_plan;
int wdno_cond_plan(const wdno_cond_desc* c, unsigned align_mask, wdno_diffusion_plan* out);
int wdno_weighted_mse_plan(int64_t B, int64_t per_sample, int C, int64_t inner, size_t ws_bytes, unsigned align_mask, int backward,
                           wdno_diffusion_plan* out);
int wdno_update_plan(int64_t B, int64_t per_sample, unsigned align_mask, wdno_diffusion_plan* out);

/* ------------------------------------------------------------------------------------------------ trainer step
 * Flat-buffer optimiser (train_diffusion.py:117,211-216 ; diffusion_2d.py:1159,1283-1291).
 * wdno_sumsq: out[0] (+)= sum g^2 (double accumulate, device scalar float).
 * wdno_adam_clip_step: g *= min(1, max_norm/(sqrt(sumsq)+1e-6)) then torch.optim.Adam update. */
size_t wdno_sumsq_ws_bytes(int64_t n);
int wdno_sumsq(const float* g, int64_t n, float* out, void* ws, size_t ws_bytes, wdno_stream_t s);
int wdno_adam_clip_step(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq, float max_norm,
                        float grad_scale, float lr, float beta1, float beta2, float eps, int step, wdno_stream_t s);
/* Gradient gather: one launch copies every per-parameter gradient tensor into its span of the flat gradient buffer (items with
 * src == NULL are zero-filled): what DistributedDataParallel's bucket copies / AccumulateGrad's adds do one tensor at a time. The
 * table of n_items wdno_copy_item lives in device memory. */
typedef struct { const void* src; void* dst; int64_t n; } wdno_copy_item;
int wdno_gather_items(const void* table, int n_items, int blocks_per_item, wdno_stream_t s);
/* ema = ema*beta + p*(1-beta)  (ema_pytorch lerp) */
int wdno_ema_update(float* ema, const float* p, int64_t n, float beta, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ Burgers solver
 * burgers_numeric_solve_free (burgers/ddpm_burgers/generate_burgers.py:104-204): the finite-difference solver that scores a designed control
 * (eval_ddpm_burgers.py:203, test_util.py:75,77). u0 [N][nx0] and f [N][nt_f][nxf] are linearly interpolated to s points (l.131-132, torch's
 * align_corners = False rule), then `steps` explicit-Euler steps of u_i += dt (-(1/2) c (u_{i+1}^2 - u_{i-1}^2) + d (u_{i-1} + u_{i+1}) +
 * dm u_i + f[j / f_time]_i) on s interior points with zero ghosts (l.176-186, each point in the reference's operation order, fp32).
 * out [N][num_t + 1][out_cols]: row 0 = the interpolated u0, row r = the state after step r * record_time - 1 (l.191-195), columns
 * 0, sub_s, 2 sub_s, ... (l.200-201; sub_s = 1 without the down-sampling). One launch; one workgroup of `waves` waves per trajectory, each lane
 * holding `points` grid points: waves in {1, 2, 4, 8, 16}, points in {2, 4, 8, 16, 32} (32 only up to 8 waves), 64 waves points >= s.
 * The host computes the integers (l.138-148) and raises the reference's exceptions; WDNO_EINVAL when they are not consistent
 * (f index or record counter past its end). Constants: c = fp32(1 / (2 dx)), d = fp32(visc / dx^2), dm = fp32(-2 visc / dx^2), dx = 1 / (s + 1),
 * dt = fp32(dt) (l.163-165). The result of a trajectory does not depend on (waves, points), N or its index. */
typedef struct {
  int N, s, nx0, nt_f, nxf;
  int steps, record_time, f_time, num_t, sub_s, out_cols;
  int waves, points;
  float c, d, dm, dt;
} wdno_burgers_desc;
int wdno_burgers_solve(const float* u0, const float* f, float* out, const wdno_burgers_desc* d, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ Burgers data-set generation
 * One batch of generate_data_burgers_equation (generate_burgers.py:278-368) in one launch: the solver above on s points (u0 [N][s] dense, no
 * interpolation) with the forcing of make_data_varying_f (l.246-273) formed from its separable parts instead of read from a dense [N][t][s]
 * tensor: ax [N][8][s] = amp_j exp_space_j, tt [N][t][8] = exp_time_j, f[n][iv][g] = sum_j ax[n][j][g] tt[n][iv][j] with j ascending and every
 * fp32 operation separate (the reference's bits), then clamp(f alpha, -10, 10) when `clamp` is set (alpha != 1, l.272-273).
 * u_rec [N][num_t + 1][cols]: the columns 0, sx, 2 sx, ... of u0 and of the recorded rows (trajectory[:, :, ::sx], l.347);
 * f_rec [N][f_rows][cols]: the forcing of the intervals 0, st, 2 st, ... at those columns (f[:, ::st, ::sx], l.346); cols = ceil(s / sx),
 * f_rows = ceil(t / st). steps, record_time, f_time, the constants and (waves, points) as in wdno_burgers_desc, with nt_f = t; the same
 * consistency checks (WDNO_EINVAL). The result of a trajectory does not depend on (waves, points), N or its index, and its u_rec equals
 * wdno_burgers_solve's on the dense forcing bit for bit. */
typedef struct {
  int N, s, t;
  int steps, record_time, f_time, num_t;
  int st, sx, f_rows, cols;
  int waves, points, clamp;
  float c, d, dm, dt, alpha;
} wdno_burgers_generate_desc;
int wdno_burgers_generate(const float* u0, const float* ax, const float* tt, float* u_rec, float* f_rec,
                          const wdno_burgers_generate_desc* d, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ Burgers control-objective guidance
 * The gradient of the control objective of the Burgers evaluation (eval_ddpm_burgers.py:108-147 get_loss_fn_2dconv / get_nablaJ_2dconv,
 * test_util.py:100-126 ddpm_guidance_loss) in closed form, one launch. For a network-unit tensor x [B][C][H][W] (C >= 8):
 *   coef = (x RESCALER)[:, 0:8, :h, :w]   (channels 0-3 = LL, da, ad, dd of u, 4-7 of f: wave_trans.py:30-40)
 *   u_f  = IDWT2(coef)[:, :, :n_t, :n_x]  (H pass, then W pass);  u = u_f[:, 0], f = u_f[:, 1, :n_t - 1]
 *   J    = wu (sum_b mean_x[(u[b,0] - target[b,0])^2 + (1 - condition_f) (u[b,n_t-1] - target[b,1])^2] + wf sum f^2)
 * J is quadratic and the synthesis linear, so with the residual r (2 wu (u - target) / n_x on rows 0 and n_t - 1 of field u, 2 wu wf f
 * on rows < n_t - 1 of field f, 0 elsewhere on the 2h x 2w grid)  g = dJ/dx = RESCALER IDWT2^T(r)  on [:, 0:8, :h, :w] and exactly 0
 * elsewhere (RESCALER once: the reference differentiates with respect to the unscaled x, model_utils.py:35-50).
 *   x_t != NULL (fused mode, one sampling step, diffusion_1d.py:205-227): in = eps, x0 = c1[t_b] x_t - c2[t_b] eps (clamped to [-1, 1]
 *     when clip_x0), out = eps + g(x0) s_table[t_b] -- a product then a sum, two roundings; out = eps bit for bit wherever g is
 *     structurally 0. The reference reads its schedule at t[0] for the whole batch (diffusion_1d.py:222); its samplers pass one t per
 *     batch, so indexing s_table per sample like c1 / c2 is the same thing. t_b is clamped into [0, num_timesteps).
 *   x_t == NULL (gradient mode): in = x0, out = g; t, c1, c2, s_table are not read.
 * target [B][2][n_x]: rows 0 and n_t - 1 of u_target. filt: host pointer to (dec_lo, dec_hi, rec_lo, rec_hi), L taps each, as wdno_dwt_*.
 * Grid: 1 + ntile workgroups per sample -- one for field u (only reconstruction rows 0 and n_t - 1 and the coefficient rows within
 * the filter's reach of them are computed) and ntile column tiles of tw coefficient columns (plus L/2 - 1 halo columns each side, periodic)
 * for field f; every intermediate lives in lds_bytes of LDS (no workspace). No atomics, every sum in a fixed order: a sample's result does
 * not depend on B or its index. `in` and `out` must not overlap (a tile reads its neighbours' halo columns). ntile tw >= w, lds_bytes <= 64 KiB and what the layout needs
 * (wdno_amd/burgers/guidance.py: plan); WDNO_EUNSUPPORTED for anything but mode 0 (periodization) with L = 10 (bior2.4),
 * WDNO_EINVAL for inconsistent integers. */
typedef struct {
  int B, C, H, W;                                  /* the tensors x_t, in, out */
  int sample_stride, chan_stride, row_stride;      /* in elements; columns are contiguous */
  int h, w, n_t, n_x;                              /* coefficient block (padded_shape) and field size (ori_shape): n_t <= 2h, n_x <= 2w */
  int L, mode;
  int ntile, tw, lds_bytes;
  int num_timesteps;                               /* length of c1, c2, s_table */
  int condition_f, clip_x0;
  float wu, wf;
} wdno_burgers_guidance_desc;
int wdno_burgers_guidance(const float* x_t, const float* in, const int64_t* t, const float* c1, const float* c2, const float* s_table,
                          const float* rescaler, const float* target, float* out, const wdno_burgers_guidance_desc* d, const float* filt,
                          wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ smoke control-objective guidance
 * The gradient of the control objective of the smoke inference (smoke/inference_2d.py:30-66) in closed form, at most two launches. For a
 * network-unit tensor x [B][F][C][H][W] (C >= 42), coefficient block (tc, hc, wc) and field size (to, ho, wo):
 *   xs    = x RESCALER;  channel 8 f + band of frames < tc, rows < hc, columns < wc = sub-band band = 4 bt + 2 bh + bw of field f (f < 5)
 *   state = IDWT3(xs)[:, :, :to, :ho, :wo]      (W pass, H pass, T pass; zero mode, L = 6: an axis of v coefficients gives 2 v - 4 samples)
 *   lo, hi = the means of xs[:, k < tc, C - 1] over rows < half and rows >= half;  smoke_out = IDWT1(lo, hi)
 *   J = w_init sum_b mean((state[b, 0, 0] - init_u[b])^2)
 *       + (1 - is_condition_control) (w_energy sum_b mean(state[b, 3:5]^2) - sum_b smoke_out[b, to - 1])
 * J is quadratic in the state and linear in the smoke-out channel, so with the residual r (2 w_init (state - init_u) / (ho wo) on frame 0 of
 * field 0 when has_init_u and w_init != 0; 2 w_energy state / (2 to ho wo) on fields 3 and 4 when not is_condition_control and
 * w_energy != 0; 0 elsewhere on the reconstruction grid)
 *   g = dJ/dxs = IDWT3^T(r) on [:, :tc, 0:40, :hc, :wc]   (exactly 0 for fields 1, 2 and, for field 0, on coefficient frames >= 3)
 *   g[:, k < tc, C - 1, rows < half] = -succ[0][k] / (half W),  g[:, k < tc, C - 1, rows >= half] = -succ[1][k] / ((H - half) W)
 *       (not is_condition_control; succ [2][tc] = d smoke_out[to - 1] / d(lo, hi), two constant vectors the caller computes once)
 * and exactly 0 everywhere else. g is NOT multiplied by RESCALER: the reference differentiates with respect to xs.
 *   x_t != NULL (fused mode, one sampling step, diffusion_2d.py:723-754): in = eps, x0 = c1[t_b] x_t - c2[t_b] eps (clamped to [-1, 1]
 *     when clip_x0), out = eps + g(x0) s_table[t_b] -- a product then a sum, two roundings; out = eps bit for bit wherever g is 0.
 *     t_b is clamped into [0, num_timesteps).
 *   x_t == NULL (gradient mode): in = x0, out = g; t, c1, c2, s_table are not read.
 * rescaler [C]; init_u [B][ho][wo] or NULL; filt: host pointer to (dec_lo, dec_hi, rec_lo, rec_hi), L taps each, as wdno_dwt_*.
 * Launch 1 (skipped when r is 0 everywhere): a workgroup per (sample, field, tile of tn reconstruction frames x hn rows) synthesises fields
 * 3 and 4 in full and frame 0 of field 0 from the coefficients, read in place in the packed state with x0 RESCALER formed on the fly, and
 * writes r, scaled and cropped, to ws: B (2 to ho wo + ho wo) floats (wdno_smoke_guidance_ws_bytes; 0 for a descriptor that is refused).
 * Launch 2: a workgroup per (sample, field, tile of kt coefficient frames x kh rows) turns r into g and writes `out` there; these and
 * ncopy further workgroups per sample share the rest of the tensor (the copy of eps, or zeros, and the smoke-out term). Every intermediate
 * of a tile lives in lds1_bytes / lds2_bytes of LDS. Nothing is allocated; no atomics, every sum in a fixed order: a sample's result does
 * not depend on B or its index. `in` and `out` must not overlap. tn, hn even; lds*_bytes <= 64 KiB and what the layout needs
 * (wdno_amd/smoke/guidance.py: plan). WDNO_EUNSUPPORTED for anything but mode 1 (zero) with L = 6 (bior1.3); WDNO_EINVAL for inconsistent
 * integers: a block larger than the tensor, a crop larger than the reconstruction, tiles or LDS sizes that do not fit. */
typedef struct {
  int B, F, C, H, W;                                            /* the tensors x_t, in, out */
  int sample_stride, frame_stride, chan_stride, row_stride;     /* in elements; columns are contiguous */
  int tc, hc, wc, to, ho, wo;                                   /* coefficient block (shape) and field size (ori_shape): to <= 2 tc - 4, ... */
  int L, mode, half;
  int num_timesteps;                                            /* length of c1, c2, s_table */
  int clip_x0, is_condition_control, has_init_u;
  int tn, hn, kt, kh, ncopy;
  int lds1_bytes, lds2_bytes;
  float w_energy, w_init;
} wdno_smoke_guidance_desc;
size_t wdno_smoke_guidance_ws_bytes(const wdno_smoke_guidance_desc* d);
int wdno_smoke_guidance(const float* x_t, const float* in, const int64_t* t, const float* c1, const float* c2, const float* s_table,
                        const float* rescaler, const float* init_u, const float* succ, float* out, void* ws, size_t ws_bytes,
                        const wdno_smoke_guidance_desc* d, const float* filt, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ smoke control-evaluation solver
 * solver() of smoke/dataset/evaluate_solver.py:135-196 for B simulations in one launch, one workgroup of `threads` (1024 or 512) threads per
 * simulation: num_t (<= 256) frames of { velocity = interior of the previous frame's + 16-cell rim of the control (c1, c2 [B][nt][nx][nx],
 * tiled by time_interval and space_interval), masked; divergence; the masked 5-point system solved by CG in fp32 from x = 0 until
 * max|r| < accuracy or max_iter (<= 500) iterations, with the reference's aliased first iteration (phi/solver/base.py:56-103) and the
 * pressure (the sum of the steps) accumulated in fp64; velocity minus
 * the masked pressure gradient; advection of the density and the set-zero density (linear, coordinates clamped, fp64 weights); the seven
 * fp64 bucket sums and the ratio outs[1] / (sum(outs) + sum(set-zero density)) }. A frame whose masked divergence is below `accuracy`
 * everywhere keeps zero pressure (the reference's loop condition), and the loop also ends when sum(p Ap) is exactly zero.
 * Geometry is data, fp32: fluid_ext, active_ext [129][129] (the masks with their boundary padding), velocity_mask [128][128][2],
 * buckets [8][128][128] (seven bucket masks, then the set-zero mask). init_density [B][nx][nx]; init_velocity [128][128][2], shared.
 * frame_slot [num_t]: the output slot of a frame or -1; density, zero_density [B][n_out][128][128], velocity [B][n_out][128][128][2],
 * ratio [B][num_t] fp64 (every frame). ws: 9 * 128 * 128 floats per simulation, 16-byte aligned. Every sum has a fixed order: a simulation's result does not
 * depend on `threads`, B or its index. WDNO_EINVAL for inconsistent integers, WDNO_EUNSUPPORTED for another `threads`. */
typedef struct {
  int B, nt, nx, time_interval, space_interval;
  int num_t, max_iter, n_out, threads;
  float accuracy;
} wdno_smoke_solve_desc;
int wdno_smoke_solve(const float* init_density, const float* c1, const float* c2, const float* init_velocity, const float* fluid_ext,
                     const float* active_ext, const float* velocity_mask, const float* buckets, const int* frame_slot, float* density,
                     float* zero_density, float* velocity, double* ratio, float* ws, const wdno_smoke_solve_desc* d, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ smoke data-set generator
 * The training-set simulator of smoke/dataset/a_gen_train.py:363-456, 502-696 (and a_gen_test_64 / a_gen_test_128, which differ in recording
 * only) for B scenes in one launch, one workgroup of `threads` (1024 or 512) threads per scene: frames 0..scenelength (<= 256), each with the
 * steps of wdno_smoke_solve (same code, csrc/smoke_flow.h; the advection coordinate idx - v is formed in fp64 here, in fp32 there), but the 16-cell rim of a frame's velocity is the previous frame's projected rim
 * plus noise, fp32(fp64(previous) + noise), or, on the scene's four kick frames, the noise field itself, fp32(noise).
 * scene_i [B][8]: xs0, ys0 (the 11 x 11 block of initial density), the four kick frames, 0, 0. scene_v [B][8]: (vx, vy) of the four kicks.
 * scene_index [B]: the scene's number in the data set. noise_mode 0: `noise` float64 [B][scenelength + 1][128][128][2] is read (rim cells
 * only); noise_mode 1: noise = NULL, the field is 0.1 z (ordinary frame) or v + (|v| / 10) z (kick) in fp32 with z the Box-Muller pair
 * (r cos, r sin; r = sqrt(-2 ln u1), angle 2 pi u2; u = ((x >> 9) + 0.5) 2^-23 of outputs 0 and 1) of Philox4x32-10 with key = seed and
 * counter = (cell 128 i + j, frame, scene_index low, scene_index high): a scene has the same bits in any batch.
 * Bucket rule: on the set-zero density; tested on all cells, summed on the recorded stride; on a kick frame only if the frame is recorded;
 * never at frame 0. Records at frames k * record_scale, cells ::stride (n = 128 / stride, R = scenelength / record_scale + 1):
 * density [B][R][n][n] (never zeroed), velocity, control [B][R][n][n][2] (control: the rim field before the mask, interior 0; velocity
 * record 0 holds component 0 twice, as the reference writes it), smoke [B][R][8] fp64 (seven bucket totals; column 7: the strided sum of
 * the set-zero density after zeroing on an ordinary frame, of the density on a kick frame and at frame 0). ws as for wdno_smoke_solve.
 * wdno_smoke_noise: the noise_mode-1 fields of n <= 65535 (scene_index, frame, is_kick, kick_v (vx, vy)) items, out [n][128][128][2] fp32. */
typedef struct {
  int B, scenelength, record_scale, stride;
  int max_iter, threads, noise_mode;
  float accuracy;
  unsigned long long seed;
} wdno_smoke_generate_desc;
int wdno_smoke_generate(const int* scene_i, const float* scene_v, const long long* scene_index, const double* noise,
                        const float* init_velocity, const float* fluid_ext, const float* active_ext, const float* velocity_mask,
                        const float* buckets, float* density, float* velocity, float* control, double* smoke, float* ws,
                        const wdno_smoke_generate_desc* d, wdno_stream_t s);
int wdno_smoke_noise(const long long* scene_index, const int* frame, const int* is_kick, const float* kick_v, int n,
                     unsigned long long seed, float* out, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ smoke inference: reconstruction and scoring
 * wdno_smoke_reconstruct: the wavelet branch of InferencePipeline.run_base_model (smoke/inference_2d.py:137-152) for the whole batch in one
 * launch. For the sampled state x [B][F][C][H][W] in network units (C >= 42, strides in elements, columns contiguous), rescaler [C], the
 * coefficient block (tc, hc, wc) and the field size (to, ho, wo), with xs = x RESCALER formed on the fly and the coefficients read in place
 * (channel 8 f + band of frames < tc, rows < hc, columns < wc = sub-band band = 4 bt + 2 bh + bw of field f):
 *   pred[b, :, f]  = IDWT3(xs)[f][:to, :ho, :wo]  for f < 5        (zero mode, L = 6: an axis of v coefficients gives 2 v - 4 samples)
 *   pred[b, n, 5]  = IDWT1(lo, hi)[n] in every cell, lo[k], hi[k] = the means of xs[b, k, C - 1] over rows < half and rows >= half (all W
 *                    columns), k < tc; the sums are fp64 of fp32 products, the means rounded to fp32
 * pred [B][to][6][ho][wo] fp32, contiguous. A workgroup per (sample, field, tile of tn frames x hn rows, full width) runs the T, H and W
 * passes with its intermediates in lds_bytes of LDS; cdiv(to, tn) more workgroups per sample write channel 5. Nothing is allocated; no
 * atomics, every sum in a fixed order: a sample's bits do not depend on B or its index. x and pred must not overlap. tn, hn even;
 * lds_bytes <= 64 KiB and what the layout needs (wdno_amd/smoke/reconstruct.py: plan). filt as for wdno_smoke_guidance.
 * WDNO_EUNSUPPORTED for anything but mode 1 (zero) with L = 6 (bior1.3); WDNO_EINVAL for inconsistent integers: a block larger than the
 * tensor, a crop larger than the reconstruction, tiles or an LDS size that do not fit. */
typedef struct {
  int B, F, C, H, W;                                            /* the tensor x */
  int sample_stride, frame_stride, chan_stride, row_stride;     /* in elements; columns are contiguous */
  int tc, hc, wc, to, ho, wo;                                   /* coefficient block (shape) and field size (ori_shape): to <= 2 tc - 4, ... */
  int L, mode, half;
  int tn, hn;
  int lds_bytes;
} wdno_smoke_reconstruct_desc;
int wdno_smoke_reconstruct(const float* x, const float* rescaler, float* pred, const wdno_smoke_reconstruct_desc* d, const float* filt,
                           wdno_stream_t s);

/* wdno_smoke_score: the sums InferencePipeline.multi_evaluate (smoke/inference_2d.py:426-439) takes its metrics from, for one (pred, data)
 * pair in one launch, one workgroup per sample. pred [B][T][6][h][w] fp32, contiguous. data: HOST pointer to six channel entries; channel
 * c of the data at (b, t, row, col) is ptr[b sample_stride + t frame_stride + row row_stride + col col_stride], fp32 or fp64 (is_double);
 * strides in elements, >= 0, a zero stride broadcasts. out [B][5] fp64, every difference formed as (double)pred - (double)data:
 *   out[b][0] = sum (pred - data)^2 over channels 0..2      out[b][1] = sum (pred - data)^2 over channel 5
 *   out[b][2] = sum data^2 over channels 0..2               out[b][3] = sum data^2 over channels 3..4
 *   out[b][4] = data[b, T - 1, 5, 0, 0]
 * Sums 0 and 2 leave out frame 0 of channel 0 (the reference's mask[:, 0, 0] = False). No atomics, a fixed order: a sample's result does
 * not depend on B or its index. Nothing is allocated. WDNO_EINVAL for inconsistent integers, negative strides or misaligned pointers. */
typedef struct {
  const void* ptr;
  long long sample_stride, frame_stride, row_stride, col_stride;
  int is_double, reserved;
} wdno_smoke_score_channel;
int wdno_smoke_score(const float* pred, const wdno_smoke_score_channel* data, double* out, int B, int T, int h, int w, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ smoke inference: the super-resolution cascade
 * wdno_smoke_reconstruct_at: wdno_smoke_reconstruct with the coefficient block read at rows and columns off .. off + hc / wc of the tensor
 * (tensor_to_coef(..., upsample_type='space') of smoke/inference_2d.py:219 is off = 1; hc + off <= H, wc + off <= W). The smoke-out means
 * still run over the whole rows < half and >= half of channel C - 1: the offset moves the coefficient block only. off = 0 is
 * wdno_smoke_reconstruct bit for bit. */
int wdno_smoke_reconstruct_at(const float* x, const float* rescaler, float* pred, const wdno_smoke_reconstruct_desc* d, int off,
                              const float* filt, wdno_stream_t s);

/* wdno_smoke_cascade_conditions: what run_super_model (smoke/inference_2d.py:176-196) hands to the super model's sample() as low,
 * init / RESCALER[-2] and control / RESCALER[24:40], written in one launch as the sampler's condition source
 * src [B][pad_t][82][pad_x][pad_x] (fp32, 16-byte aligned, network units; every element is written):
 *   src[b, f, 40 + c, h, w] = prev[b, f, c, h / 2, w / 2]                      f < t0, h < 2 h0, w < 2 w0, c < 40; 0 beyond. Copied, not rescaled.
 *   src[b, f, 24 + 8 g + band, h, w] = coef[b, g, band, f, clamp(h - 1), clamp(w - 1)] / rescaler[24 + 8 g + band]
 *                                                                             f < t1, h < h1 + 2, w < w1 + 2; 0 / rescaler beyond
 *   src[b, f, 80, h, w] = DWT2(rho0[b])[f % 4][h, w] / rescaler[80]           h < h1, w < w1; 0 / rescaler beyond
 *   every other channel = 0
 * prev: the base level's sample [B][F0][C0 >= 40][H0][W0] with element strides (columns contiguous); coef: the packed zero-mode 3-D analysis
 * [B][2][8][t1][h1][w1] of the fine controls, contiguous; rho0: the fine initial density [B][Hf][Wf] with sample and row strides; DWT2 is the
 * zero-mode analysis with sub-bands in the order Yl, Yh[0][:, 0]'s three, and the frame order f % 4 is the reference's at this level (l.181),
 * not the base level's. rescaler [82]; filt as for wdno_smoke_guidance. Requires 2 h0 == h1 + 2, 2 w0 == w1 + 2, h1 + 2 <= pad_x,
 * w1 + 2 <= pad_x, h1 == (Hf + L - 1) / 2, w1 == (Wf + L - 1) / 2, pad_t % 4 == 0, pad_x % 4 == 0, sample strides < 2^31: WDNO_EINVAL otherwise;
 * WDNO_EUNSUPPORTED for anything but mode 1 (zero), L = 6 (bior1.3), C = 82. Nothing is allocated. */
typedef struct {
  long long prev_sample_stride, rho_sample_stride;
  int prev_frame_stride, prev_chan_stride, prev_row_stride, rho_row_stride;
  int B, F0, C0, H0, W0;
  int t0, h0, w0, t1, h1, w1, Hf, Wf;
  int pad_t, pad_x, C, L, mode;
} wdno_smoke_cascade_desc;
int wdno_smoke_cascade_conditions(const float* prev, const float* coef, const float* rho0, const float* rescaler, float* src,
                                  const wdno_smoke_cascade_desc* d, const float* filt, wdno_stream_t s);

/* wdno_smoke_score_super: the sums of the four comparisons of InferencePipeline.multi_evaluate's super-resolution branch in simulation mode
 * (smoke/inference_2d.py:405-439) in one launch, a workgroup per (sample, comparison). pred [B][T][6][n][n] fp32, contiguous; data: six
 * channel entries as for wdno_smoke_score, describing the data at its FULL resolution N x N; n == N or 2 n == N, N even. out [B][4][5] fp64,
 * the five sums of wdno_smoke_score per comparison, over the comparison's own grid:
 *   0 base     pred at stride 2 n / N   against data at stride 2          (N / 2 cells a side)
 *   1 current  pred                     against data at stride N / n      (n cells a side)
 *   2 linear   pred interpolated bilinearly (align_corners = False) to N cells a side, against data
 *   3 nearest  pred[h n / N, w n / N] against data
 * The interpolated tensors are never built: for N == 2 n the bilinear value is formed in fp64 from the four neighbours with the weights
 * 0.25 / 0.75 and the edge clamp of F.interpolate; for N == n comparisons 2 and 3 read pred itself. */
int wdno_smoke_score_super(const float* pred, const wdno_smoke_score_channel* data, double* out, int B, int T, int n, int N, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ Burgers evaluation: reconstruction and scoring
 * wdno_burgers_reconstruct: the wavelet branch of diffuse_2dconv (eval_ddpm_burgers.py:185-195) for the whole batch in one launch. For the
 * sampled state x [B][C][H][W] in network units (C >= 8, strides in elements, columns contiguous), rescaler [>= 8], the coefficient block
 * (h, w) and the field size (n_t, n_x), with the coefficients read in place and x RESCALER formed on the fly:
 *   u_f = IDWT2((x RESCALER)[:, 0:8, :h, :w])[:, :, :n_t, :n_x]   (channels 0-3 = LL, da, ad, dd of u, 4-7 of f; H pass, then W pass;
 *                                                                   periodization, L = 10: an axis of v coefficients gives 2 v samples)
 *   u = u_f[:, 0]  [B][n_t][n_x],   f = u_f[:, 1, :n_t - 1]  [B][n_t - 1][n_x],   fp32, contiguous, each written once.
 * Nothing outside the block is read. A workgroup per (sample, field, tile of tn reconstruction rows, full width) runs both passes with its
 * intermediates in lds_bytes of LDS (8 tn w bytes); the arithmetic and its order are those of wdno_burgers_guidance's residual. Nothing is
 * allocated; no atomics, every sum in a fixed order: a sample's bits do not depend on B or its index. x, u and f must not overlap. tn even,
 * (ntile - 1) tn < n_t <= ntile tn, lds_bytes <= 64 KiB (wdno_amd/burgers/reconstruct.py: plan). filt as for wdno_burgers_guidance.
 * WDNO_EUNSUPPORTED for anything but mode 0 (periodization) with L = 10 (bior2.4); WDNO_EINVAL for inconsistent integers: a block larger
 * than the tensor, a crop larger than the reconstruction, an LDS size or strides that do not fit. Nothing is written then. */
typedef struct {
  int B, C, H, W;                                  /* the tensor x */
  long long sample_stride;                         /* in elements; columns are contiguous */
  int chan_stride, row_stride;
  int h, w, n_t, n_x;                              /* coefficient block (padded_shape) and field size (ori_shape): n_t <= 2h, n_x <= 2w */
  int L, mode;
  int tn, ntile, lds_bytes, reserved;
} wdno_burgers_reconstruct_desc;
int wdno_burgers_reconstruct(const float* x, const float* rescaler, float* u, float* f, const wdno_burgers_reconstruct_desc* d,
                             const float* filt, wdno_stream_t s);

/* wdno_burgers_score: the sums and order statistics behind mse_deviation and the two metric(..., evaluate=True) calls of diffuse_2dconv
 * (eval_ddpm_burgers.py:220-230, test_util.py:79-98) for one batch in one launch, one workgroup per sample. u [B][n_t][n_x] and
 * f [B][n_t - 1][n_x] fp32 contiguous (as wdno_burgers_reconstruct writes them); x_gt and u_target fp32 views of [B][n_t][n_x sub]:
 * element (b, r, c) at ptr[b sample_stride + r row_stride + c col_stride], strides in elements, >= 0. With t = u_target[b, n_t - 1, :],
 * the candidates c0 = u[b, n_t - 1] with every value repeated sub times and c1 = x_gt[b, n_t - 1, :], every difference formed as
 * (double)a - (double)b and accumulated in fp64, out [B][14] fp64:
 *   out[b][0]           sum over rows 1 .. n_t - 1 and columns j of (u[b, r, j] - x_gt[b, r, j sub])^2
 *   out[b][1 + 5 k ..]  for candidate k: sum (c - t)^2 over the columns ::sub | sum (c - t)^2 | sum |c - t| | lower median of (c - t)^2 |
 *                       lower median of |c - t|   (the element of rank (n - 1) / 2 of the sorted row, torch's median; exact selection)
 *   out[b][11]          sum f^2        out[b][12] sum t^2        out[b][13] sum |t|
 * lds_bytes = 16 n_x sub (the two fp64 rows the medians are selected from), n_x sub <= 3840. No atomics, a fixed order: a sample's row
 * does not depend on B or its index. Nothing is allocated. WDNO_EINVAL for inconsistent integers, negative strides or misaligned
 * pointers. */
typedef struct {
  int B, n_t, n_x, sub;
  long long gt_sample_stride, gt_row_stride, gt_col_stride;      /* x_gt */
  long long ut_sample_stride, ut_row_stride, ut_col_stride;      /* u_target */
  int lds_bytes, reserved;
} wdno_burgers_score_desc;
int wdno_burgers_score(const float* u, const float* f, const float* x_gt, const float* u_target, double* out,
                       const wdno_burgers_score_desc* d, wdno_stream_t s);

/* ------------------------------------------------------------------------------------------------ Burgers evaluation: the super-resolution cascade
 * wdno_burgers_cascade_conditions: the hand-off between two levels of evaluate()'s cascade (eval_ddpm_burgers.py:306-338; test_util.py:185-196)
 * in one launch that writes EVERY element of the super level's condition source src [B][17][P_t][P_x] (fp32, contiguous, 16-byte aligned,
 * network units), in place of upsample_coef, the pad, the division, get_target(is_wave=True), its slices and divisions, and the zeroed tensor
 * and three copies of GaussianDiffusion._sampling_setup:
 *   src[b, 8 + c, i, j] = x_prev[b, c, i / 2, j / 2] / rescaler[8 + c]        i < 2 h0, j < 2 w0, c < 8; 0 beyond. One IEEE division: with
 *                                                                            x_prev = sample * rescaler the reference's (x r) / r bit for bit
 *   src[b, 16, i, j]    = band(i / (P_t / 4))[j] / rescaler[16]              j < n_x / 2; 0 beyond, and 0 where the stripe's flag is off
 *   src[b, 0..7]        = 0
 * x_prev: the previous level's returned block [B][8][h0][w0] with element strides (columns contiguous). 2 h0 = h1 + 1 is one row more than
 * the fine block (h1, w1): the ps[0] + 1 rows the sampler copies. band(0), band(1) are the low and high band of the one-level periodized
 * analysis (L = 10) of u_target[b, 0, :n_x], band(2), band(3) those of u_target[b, n_t - 1, :n_x] (flags cond_u0 / cond_uT), with
 * band[k] = sum_m dec[L - 1 - m] u[(2 k + m - (L / 2 - 1)) mod n_x], accumulated in fp32 in the order m = 0 .. L - 1. u_target is read in
 * place: element (b, r, c) at u_target[b tgt_sample_stride + r tgt_row_stride + c tgt_col_stride], strides in elements. rescaler [17]; filt
 * as for wdno_burgers_guidance. A workgroup per (tile of `tile` rows, channel, sample); lds_bytes = 16 P_x. Requires 2 h0 == h1 + 1,
 * 2 w0 == w1 == n_x / 2, 2 h0 <= P_t, 2 w0 <= P_x, P_t % 4 == 0, P_x % 4 == 0, P_x <= 2048, n_x >= L, ntile == ceil(P_t / tile), C == 17:
 * WDNO_EINVAL otherwise; WDNO_EUNSUPPORTED for anything but mode 0 (periodization) with L = 10 (bior2.4). Nothing is written then, and nothing
 * is allocated. No atomics, a fixed order: a sample's bits do not depend on B or its index. */
typedef struct {
  long long prev_sample_stride;                                 /* x_prev, in elements; columns are contiguous */
  long long tgt_sample_stride, tgt_row_stride, tgt_col_stride;  /* u_target */
  int prev_chan_stride, prev_row_stride;
  int B, C, h0, w0, h1, w1;                                     /* previous block, fine block */
  int n_t, n_x;                                                 /* the level's target: rows 0 and n_t - 1, columns 0 .. n_x - 1 are read */
  int P_t, P_x;
  int tile, ntile;
  int cond_u0, cond_uT;
  int L, mode;
  int lds_bytes, reserved;
} wdno_burgers_cascade_desc;
int wdno_burgers_cascade_conditions(const float* x_prev, const float* u_target, const float* rescaler, float* src,
                                    const wdno_burgers_cascade_desc* d, const float* filt, wdno_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* WDNO_HIP_H */
