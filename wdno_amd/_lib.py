"""ctypes binding of libwdno_hip.so (the C ABI declared in include/wdno_hip.h).

The product path has NO fallback: if the shared library is missing or a call returns an error, a RuntimeError is
raised. Nothing in this package computes on the CPU.
"""
import contextlib
import ctypes as C
import os

import torch  # noqa: F401  -- must be imported first: libwdno_hip.so has to bind to the HIP runtime instance torch already loaded

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libwdno_hip.so')

P = C.c_void_p
I = C.c_int
L = C.c_int64
F = C.c_float
Z = C.c_size_t


class DwtDesc(C.Structure):
    _fields_ = [('nd', I), ('mode', I), ('L', I), ('n_img', I), ('in_dims', I * 3), ('out_dims', I * 3),
                ('cs_img', L), ('cs_band', L), ('cs0', L), ('cs1', L)]


class ConvGeom(C.Structure):
    _fields_ = [(k, I) for k in ('N', 'D', 'H', 'W', 'C', 'OD', 'OH', 'OW', 'K', 'kd', 'kh', 'kw', 'sd', 'sh', 'sw',
                                 'pd', 'ph', 'pw', 'YD', 'YH', 'YW', 'osd', 'osh', 'osw', 'ood', 'ooh', 'oow')]


class AttnDesc(C.Structure):
    _fields_ = [('n_uo', I), ('n_ui', I), ('n_tok', I), ('heads', I), ('so', L), ('si', L), ('st', L)]


class CondDesc(C.Structure):
    _fields_ = [(k, I) for k in ('tree', 'B', 'F', 'C', 'H', 'W', 'cT', 'cH', 'cW', 'cond_pad', 'cond_a', 'cond_b',
                                 'cond_c', 'cond_low', 'u_rows', 'uT_rows')]


class WgradReduceItem(C.Structure):          # include/wdno_hip.h: wdno_wgrad_reduce_item
    _fields_ = [('ws', C.c_void_p), ('dw', C.c_void_p), ('n', I), ('splits', I), ('K8', I), ('C8', I), ('kw', I), ('ntap', I), ('Kn', I), ('Cn', I),
                ('tiled', I), ('reserved', I)]


class ConvPlan(C.Structure):                 # include/wdno_hip.h: wdno_conv_plan
    _fields_ = [(k, I) for k in ('family', 'bm', 'bn', 'uniform', 'tsplit', 'ksplit', 'ntiles', 'grid')]


class AttnPlan(C.Structure):                 # include/wdno_hip.h: wdno_attn_plan
    _fields_ = [(k, I) for k in ('family', 'grid', 'items_per_block', 'max_walk', 'dbias_partials', 'dbias_in_lds', 'lds_bytes', 'rc')]


ATTN_FAMILIES = ('mfma24', 'mfma', 'mfma64', 'tiled', 'tiled_staged', 'tiled_unstaged', 'big', 'rows')      # WDNO_ATTN_*; -1: none


class LinAttnPlan(C.Structure):              # include/wdno_hip.h: wdno_la_plan
    _fields_ = [(k, I) for k in ('kstats_chunks', 'ctx_chunks', 'token_tiles', 'family', 'rc')]


class LayerNormPlan(C.Structure):            # include/wdno_hip.h: wdno_ln_plan
    _fields_ = [(k, I) for k in ('tpr', 'vpl', 'rows_per_block', 'blocks', 'max_rows_walk', 'rc')]


class DiffusionPlan(C.Structure):            # include/wdno_hip.h: wdno_diffusion_plan
    _fields_ = [(k, I) for k in ('form', 'grid_x', 'grid_y', 'rc')]


DIFFUSION_FORMS = ('scalar', 'float4')                                                                       # WDNO_FORM_*


class DwtPlan(C.Structure):                 # include/wdno_hip.h: wdno_dwt_plan
    _fields_ = [(k, I) for k in ('family', 'variant', 'nh', 'tiles_h', 'tiles_t', 'blocks', 'lds_bytes', 'rc')]


DWT_ENTRIES = ('fwd', 'inv', 'inv_adjoint', 'fwd_adjoint', 'fwd_packed')                                     # WDNO_DWT_ENTRY_*
DWT_FAMILIES = ('per_axis', 'analysis', 'analysis_packed', 'synthesis2', 'synthesis_fused', 'synthesis3_stream')   # WDNO_DWT_*; -1: none


class ConvWgradPlan(C.Structure):            # include/wdno_hip.h: wdno_wgrad_plan
    _fields_ = [(k, I) for k in ('family', 'bm', 'bn', 'splits', 'pix_per_split', 'splitpair', 'reduce_tiled', 'items', 'grid')]


CONV_FAMILIES = ('fp32', 'h3', 'h3d', 'h3t', 'h3t_stem')          # WDNO_CONV_*
WGRAD_FAMILIES = ('h3', 'h3d', 'h3w', 'h3s')                       # WDNO_WGRAD_*


class RowsSumItem(C.Structure):              # include/wdno_hip.h: wdno_rows_sum_item
    _fields_ = [('part', C.c_void_p), ('out', C.c_void_p), ('rows', I), ('stride', I), ('col0', I), ('ncols', I), ('is_double', I), ('reserved', I)]


class BurgersDesc(C.Structure):             # include/wdno_hip.h: wdno_burgers_desc
    _fields_ = [(k, I) for k in ('N', 's', 'nx0', 'nt_f', 'nxf', 'steps', 'record_time', 'f_time', 'num_t', 'sub_s', 'out_cols', 'waves',
                                 'points')] + [(k, F) for k in ('c', 'd', 'dm', 'dt')]


class BurgersGenerateDesc(C.Structure):     # include/wdno_hip.h: wdno_burgers_generate_desc
    _fields_ = [(k, I) for k in ('N', 's', 't', 'steps', 'record_time', 'f_time', 'num_t', 'st', 'sx', 'f_rows', 'cols', 'waves', 'points',
                                 'clamp')] + [(k, F) for k in ('c', 'd', 'dm', 'dt', 'alpha')]


class BurgersGuidanceDesc(C.Structure):     # include/wdno_hip.h: wdno_burgers_guidance_desc
    _fields_ = [(k, I) for k in ('B', 'C', 'H', 'W', 'sample_stride', 'chan_stride', 'row_stride', 'h', 'w', 'n_t', 'n_x', 'L', 'mode', 'ntile',
                                 'tw', 'lds_bytes', 'num_timesteps', 'condition_f', 'clip_x0')] + [(k, F) for k in ('wu', 'wf')]


class SmokeGuidanceDesc(C.Structure):       # include/wdno_hip.h: wdno_smoke_guidance_desc
    _fields_ = [(k, I) for k in ('B', 'F', 'C', 'H', 'W', 'sample_stride', 'frame_stride', 'chan_stride', 'row_stride', 'tc', 'hc', 'wc', 'to', 'ho',
                                 'wo', 'L', 'mode', 'half', 'num_timesteps', 'clip_x0', 'is_condition_control', 'has_init_u', 'tn', 'hn', 'kt', 'kh',
                                 'ncopy', 'lds1_bytes', 'lds2_bytes')] + [(k, F) for k in ('w_energy', 'w_init')]


class SmokeSolveDesc(C.Structure):          # include/wdno_hip.h: wdno_smoke_solve_desc
    _fields_ = [(k, I) for k in ('B', 'nt', 'nx', 'time_interval', 'space_interval', 'num_t', 'max_iter', 'n_out', 'threads')] + [('accuracy', F)]


class SmokeGenerateDesc(C.Structure):       # include/wdno_hip.h: wdno_smoke_generate_desc
    _fields_ = [(k, I) for k in ('B', 'scenelength', 'record_scale', 'stride', 'max_iter', 'threads', 'noise_mode')] + [('accuracy', F), ('seed', C.c_uint64)]


class SmokeReconstructDesc(C.Structure):    # include/wdno_hip.h: wdno_smoke_reconstruct_desc
    _fields_ = [(k, I) for k in ('B', 'F', 'C', 'H', 'W', 'sample_stride', 'frame_stride', 'chan_stride', 'row_stride', 'tc', 'hc', 'wc', 'to', 'ho',
                                 'wo', 'L', 'mode', 'half', 'tn', 'hn', 'lds_bytes')]


class SmokeScoreChannel(C.Structure):       # include/wdno_hip.h: wdno_smoke_score_channel
    _fields_ = [('ptr', C.c_void_p)] + [(k, C.c_longlong) for k in ('sample_stride', 'frame_stride', 'row_stride', 'col_stride')] + \
               [('is_double', I), ('reserved', I)]


class SmokeCascadeDesc(C.Structure):        # include/wdno_hip.h: wdno_smoke_cascade_desc
    _fields_ = [(k, C.c_longlong) for k in ('prev_sample_stride', 'rho_sample_stride')] + \
               [(k, I) for k in ('prev_frame_stride', 'prev_chan_stride', 'prev_row_stride', 'rho_row_stride', 'B', 'F0', 'C0', 'H0', 'W0', 't0', 'h0',
                                 'w0', 't1', 'h1', 'w1', 'Hf', 'Wf', 'pad_t', 'pad_x', 'C', 'L', 'mode')]


class BurgersReconstructDesc(C.Structure):  # include/wdno_hip.h: wdno_burgers_reconstruct_desc
    _fields_ = [(k, I) for k in ('B', 'C', 'H', 'W')] + [('sample_stride', C.c_longlong)] + \
               [(k, I) for k in ('chan_stride', 'row_stride', 'h', 'w', 'n_t', 'n_x', 'L', 'mode', 'tn', 'ntile', 'lds_bytes', 'reserved')]


class BurgersCascadeDesc(C.Structure):      # include/wdno_hip.h: wdno_burgers_cascade_desc
    _fields_ = [(k, C.c_longlong) for k in ('prev_sample_stride', 'tgt_sample_stride', 'tgt_row_stride', 'tgt_col_stride')] + \
               [(k, I) for k in ('prev_chan_stride', 'prev_row_stride', 'B', 'C', 'h0', 'w0', 'h1', 'w1', 'n_t', 'n_x', 'P_t', 'P_x', 'tile', 'ntile',
                                 'cond_u0', 'cond_uT', 'L', 'mode', 'lds_bytes', 'reserved')]


class PackBurgersPlan(C.Structure):         # include/wdno_hip.h: wdno_pack_burgers_plan
    _fields_ = [(k, I) for k in ('fine_vec', 'coarse_vec', 'grid_x', 'grid_y', 'grid_z', 'lds_bytes', 'rc', 'reserved')]


class BurgersScoreDesc(C.Structure):        # include/wdno_hip.h: wdno_burgers_score_desc
    _fields_ = [(k, I) for k in ('B', 'n_t', 'n_x', 'sub')] + \
               [(k, C.c_longlong) for k in ('gt_sample_stride', 'gt_row_stride', 'gt_col_stride', 'ut_sample_stride', 'ut_row_stride', 'ut_col_stride')] + \
               [('lds_bytes', I), ('reserved', I)]


PD, PG, PA, PC = C.POINTER(DwtDesc), C.POINTER(ConvGeom), C.POINTER(AttnDesc), C.POINTER(CondDesc)
PF = C.POINTER(C.c_float)

# name -> (restype, argtypes). Every symbol declared in include/wdno_hip.h appears here (tests check both directions).
PROTOTYPES = {
    'wdno_strerror': (C.c_char_p, [I]),
    'wdno_version': (I, []),
    'wdno_last_hip_error': (C.c_char_p, []),
    'wdno_set_debug': (I, [I]),
    'wdno_dwt_ws_bytes': (Z, [PD]),
    'wdno_dwt_plan_query': (I, [PD, I, P]),
    'wdno_dwt_fwd': (I, [P, P, PD, PF, P, Z, P]),
    'wdno_dwt_fwd_packed': (I, [P, P, PD, PF, I, L, I, P, P]),
    'wdno_dwt_inv': (I, [P, P, PD, PF, P, Z, P]),
    'wdno_dwt_fwd_adjoint': (I, [P, P, PD, PF, P, Z, P]),
    'wdno_dwt_inv_adjoint': (I, [P, P, PD, PF, P, Z, P]),
    'wdno_upsample_coef': (I, [P, P, L, I, I, I, I, I, I, I, P]),
    'wdno_pack_smoke_state': (I, [P, L, P, L, P, L, P, P, P, L, I, I, I, I, I, P]),
    'wdno_pack_smoke_super_state': (I, [P, L, P, L, P, L, P, L, P, P, P, L, I, I, I, I, I, I, I, I, P]),
    'wdno_pack_smoke_fields': (I, [P, L, P, L, P, L, PF, PF, I, P, P, L, I, I, I, I, I, I, I, I, P]),
    'wdno_pack_burgers_state': (I, [P, L, P, L, P, P, P, L, I, I, I, I, I, I, I, I, I, I, I, PF, PF, PF, PF, I, P]),
    'wdno_pack_burgers_plan_query': (I, [L, L, L, I, I, I, I, I, I, I, I, I, I, I, I, C.c_uint, C.POINTER(PackBurgersPlan)]),
    'wdno_nc_to_cl': (I, [P, P, L, I, L, I, P]),
    'wdno_cl_to_nc': (I, [P, P, L, I, L, I, P]),
    'wdno_concat2_cl': (I, [P, I, P, I, P, L, P]),
    'wdno_concat2_cl_planes': (I, [P, I, P, I, P, P, P, P, P, L, P]),
    'wdno_concat2_cl_amax': (I, [P, I, P, I, P, P, L, P]),
    'wdno_split2_cl': (I, [P, P, I, P, I, L, P]),
    'wdno_upsample2x_cl_fwd': (I, [P, P, L, I, I, I, P]),
    'wdno_upsample2x_cl_bwd': (I, [P, P, L, I, I, I, P]),
    'wdno_conv_fwd': (I, [P, P, P, P, P, PG, P]),
    'wdno_amax': (I, [P, L, P, P]),
    'wdno_amax_record': (I, [P, L, P, P]),
    'wdno_split_f16': (I, [P, P, P, P, P, L, I, I, P]),
    'wdno_split_colsum_ws_bytes': (Z, [L, I]),
    'wdno_split_f16_colsum': (I, [P, P, P, P, P, P, P, Z, L, I, I, P]),
    'wdno_pack_split_weight': (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    'wdno_amax_multi': (I, [P, I, I, P]),
    'wdno_pack_split_weight_multi': (I, [P, I, I, P]),
    'wdno_conv_fwd_f16x3': (I, [P, P, P, P, P, P, P, P, P, PG, P]),
    'wdno_conv_fwd_f16x3_amax': (I, [P, P, P, P, P, P, P, P, P, P, PG, P]),
    'wdno_conv_fwd_f16x3_ws': (I, [P, P, P, P, P, P, P, P, P, P, PG, P, Z, P]),
    'wdno_conv_fwd_split_ws_bytes': (Z, [PG]),
    'wdno_conv_wgrad_f16x3_ws_bytes': (Z, [PG]),
    'wdno_conv_fwd_plan': (I, [PG, I, I, Z, P]),
    'wdno_conv_wgrad_plan': (I, [PG, I, I, I, P]),
    'wdno_conv_pixel_table': (I, [P, PG, P]),
    'wdno_conv_wgrad_f16x3': (I, [P, P, P, P, P, P, P, P, P, Z, PG, P]),
    'wdno_conv_wgrad_f16x3_param': (I, [P, P, P, P, P, P, P, P, I, I, P, Z, PG, P]),
    'wdno_conv_wgrad_partials': (I, [P, P, P, P, P, P, P, P, I, I, P, Z, PG, P, P]),
    'wdno_wgrad_reduce_multi': (I, [P, I, P]),
    'wdno_rows_sum_multi': (I, [P, I, P]),
    'wdno_cast_bf16': (I, [P, P, L, I, I, P]),
    'wdno_cast_bf16_colsum': (I, [P, P, P, P, Z, L, I, I, P]),
    'wdno_conv_fwd_bf16': (I, [P, P, P, P, P, P, PG, P]),
    'wdno_conv_fwd_f16x3_zbox': (I, [P, P, P, P, P, P, P, P, P, P, PG, P, P]),
    'wdno_conv_fwd_bf16_ex': (I, [P, P, P, P, P, I, P, PG, P, P]),
    'wdno_conv_wgrad_bf16_param': (I, [P, P, P, P, I, I, P, Z, PG, P]),
    'wdno_conv_wgrad_ws_bytes': (Z, [PG]),
    'wdno_conv_wgrad': (I, [P, P, P, P, Z, PG, P]),
    'wdno_colsum_ws_bytes': (Z, [L, I]),
    'wdno_colsum': (I, [P, P, L, I, P, Z, P]),
    'wdno_groupnorm_ws_bytes': (Z, [L, L, I, I]),
    'wdno_groupnorm_stats_floats': (Z, [L, I, I]),
    'wdno_groupnorm_act_fwd': (I, [P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_groupnorm_act_fwd_amax': (I, [P, P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_groupnorm_act_bwd': (I, [P, P, P, P, P, P, P, P, P, L, L, I, I, I, P, Z, P]),
    'wdno_groupnorm_act_bwd_amax': (I, [P, P, P, P, P, P, P, P, P, P, L, L, I, I, I, P, Z, P]),
    'wdno_groupnorm_bwd_planes_ws_bytes': (Z, [L, L, I, I]),
    'wdno_groupnorm_bwd_planes_tail': (I, [L, L, I, I, C.POINTER(Z), C.POINTER(I)]),
    'wdno_groupnorm_fwd_planes_ws_bytes': (Z, [L, L, I, I]),
    'wdno_groupnorm_act_fwd_planes': (I, [P, P, P, P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_groupnorm_act_add_fwd_planes': (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_layernorm_fwd_planes': (I, [P, P, P, P, P, L, I, F, P]),
    'wdno_groupnorm_act_bwd_planes': (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, L, L, I, I, I, P, Z, P]),
    'wdno_groupnorm_act_fwd_amax_t': (I, [P, I, P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_groupnorm_act_fwd_planes_t': (I, [P, I, P, P, P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_groupnorm_act_add_fwd_planes_t': (I, [P, I, P, P, P, P, P, P, P, P, P, P, P, P, L, L, I, I, F, I, P, Z, P]),
    'wdno_groupnorm_act_bwd_planes_t': (I, [P, I, P, I, P, P, P, P, P, P, P, P, P, P, P, P, L, L, I, I, I, P, Z, P]),
    'wdno_layernorm_fwd': (I, [P, P, P, L, I, F, P]),
    'wdno_layernorm_fwd_amax': (I, [P, P, P, P, L, I, F, P]),
    'wdno_layernorm_bwd_ws_bytes': (Z, [L, I]),
    'wdno_layernorm_bwd': (I, [P, P, P, P, P, L, I, F, P, Z, P]),
    'wdno_layernorm_bwd_add': (I, [P, P, P, P, P, P, L, I, F, P, Z, P]),
    'wdno_layernorm_bwd_add_amax': (I, [P, P, P, P, P, P, P, L, I, F, P, Z, P]),
    'wdno_attn_fwd': (I, [P, P, P, P, P, PA, F, P]),
    'wdno_attn_bwd_ws_bytes': (Z, [PA]),
    'wdno_attn_bwd': (I, [P, P, P, P, P, P, P, P, PA, F, P, Z, P]),
    'wdno_attn_fwd_amax': (I, [P, P, P, P, P, P, PA, F, P]),
    'wdno_attn_bwd_amax': (I, [P, P, P, P, P, P, P, P, P, PA, F, P, Z, P]),
    'wdno_attn_fwd_planes': (I, [P, P, P, P, P, P, P, P, P, P, PA, F, P]),
    'wdno_linattn_fwd_planes': (I, [P, P, P, P, P, P, P, L, I, I, F, P]),
    'wdno_attn_bwd_planes': (I, [P, P, P, P, P, P, P, P, P, P, P, P, PA, F, P, Z, P]),
    'wdno_attn_fwd_plan': (I, [PA, I, I, I, I, P]),
    'wdno_attn_bwd_plan': (I, [PA, I, I, I, I, P]),
    'wdno_linattn_plan': (I, [L, I, I, I, Z, P]),
    'wdno_layernorm_plan': (I, [L, I, P]),
    'wdno_tattn_fused_takes': (I, [I, I, I]),
    'wdno_tattn_fused_fwd': (I, [P, P, F, P, P, P, P, P, P, P, P, P, P, P, P, P, L, I, L, I, I, F, P]),
    'wdno_lattn_fused_takes': (I, [I, I, I]),
    'wdno_lattn_fused_ws_bytes': (Z, [L, I]),
    'wdno_lattn_fused_fwd': (I, [P, P, F, P, P, P, P, P, P, P, P, P, P, P, P, Z, L, I, I, I, F, P]),
    'wdno_lattn_fused_bwd_grads': (I, []),
    'wdno_lattn_fused_bwd_ws_bytes': (Z, [L, I]),
    'wdno_lattn_fused_bwd': (I, [P, P, P, F, P, P, P, P, P, P, P, P, P, P, P, P, P, Z, L, I, I, I, F, P]),
    'wdno_tattn_fused_plan': (I, [I, I, L, L, C.POINTER(I), C.POINTER(I)]),
    'wdno_lattn_fused_plan': (I, [L, I, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(I)]),
    'wdno_tattn_fused_bwd_ws_bytes': (Z, []),
    'wdno_tattn_fused_bwd_grads': (I, []),
    'wdno_tattn_fused_bwd': (I, [P, P, P, F, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, Z, L, I, L, I, I, F, P]),
    'wdno_linattn_ws_bytes': (Z, [L, I]),
    'wdno_linattn_fwd': (I, [P, P, P, P, L, I, I, F, P]),
    'wdno_linattn_bwd': (I, [P, P, P, P, P, P, Z, L, I, I, F, P]),
    'wdno_linattn_fwd_amax': (I, [P, P, P, P, P, L, I, I, F, P]),
    'wdno_linattn_bwd_amax': (I, [P, P, P, P, P, P, P, Z, L, I, I, F, P]),
    'wdno_linattn_bwd_planes': (I, [P, P, P, P, P, P, P, P, P, P, P, Z, L, I, I, F, P]),
    'wdno_act_fwd': (I, [P, P, L, I, P]),
    'wdno_act_bwd': (I, [P, P, P, L, I, P]),
    'wdno_linear_rows_fwd': (I, [P, I, P, I, P, P, I, I, I, I, P]),
    'wdno_linear_rows_wgrad': (I, [P, I, P, I, P, P, I, I, I, P]),
    'wdno_linear_multi_fwd': (I, [P, I, I, P, P, I, I, P]),
    'wdno_linear_multi_wgrad': (I, [P, I, I, P, P, P, P, I, I, P]),
    'wdno_linear_multi_dgrad_ws_bytes': (Z, [I, I, I]),
    'wdno_linear_multi_dgrad': (I, [P, I, I, P, P, I, I, P, Z, P]),
    'wdno_add': (I, [P, P, P, L, P]),
    'wdno_add_amax': (I, [P, P, P, P, L, P]),
    'wdno_sinusoidal_emb': (I, [P, P, P, I, I, P]),
    'wdno_q_sample_cond': (I, [P, P, P, P, P, P, P, PC, P]),
    'wdno_apply_cond': (I, [P, P, PC, P]),
    'wdno_weighted_mse_ws_bytes': (Z, [L]),
    'wdno_weighted_mse': (I, [P, P, P, P, F, P, P, L, L, I, L, P, Z, P]),
    'wdno_weighted_mse_bwd': (I, [P, P, P, P, F, P, P, L, L, I, L, P]),
    'wdno_p_sample_update': (I, [P, P, P, P, P, P, P, P, P, P, P, L, L, I, P]),
    'wdno_ddim_update': (I, [P, P, P, P, P, P, F, F, F, P, P, L, L, P]),
    'wdno_ddim_update_dev': (I, [P, P, P, P, P, P, P, P, P, L, L, P]),
    'wdno_cond_plan': (I, [PC, C.c_uint, P]),
    'wdno_weighted_mse_plan': (I, [L, L, I, L, Z, C.c_uint, I, P]),
    'wdno_update_plan': (I, [L, L, C.c_uint, P]),
    'wdno_sumsq_ws_bytes': (Z, [L]),
    'wdno_sumsq': (I, [P, L, P, P, Z, P]),
    'wdno_adam_clip_step': (I, [P, P, P, P, L, P, F, F, F, F, F, F, I, P]),
    'wdno_ema_update': (I, [P, P, L, F, P]),
    'wdno_gather_items': (I, [P, I, I, P]),
    'wdno_relpos_bias_fwd': (I, [P, P, P, I, I, P]),
    'wdno_relpos_bias_bwd': (I, [P, P, P, I, I, I, P]),
    'wdno_burgers_solve': (I, [P, P, P, C.POINTER(BurgersDesc), P]),
    'wdno_burgers_generate': (I, [P, P, P, P, P, C.POINTER(BurgersGenerateDesc), P]),
    'wdno_burgers_guidance': (I, [P, P, P, P, P, P, P, P, P, C.POINTER(BurgersGuidanceDesc), PF, P]),
    'wdno_smoke_guidance_ws_bytes': (Z, [C.POINTER(SmokeGuidanceDesc)]),
    'wdno_smoke_guidance': (I, [P, P, P, P, P, P, P, P, P, P, P, Z, C.POINTER(SmokeGuidanceDesc), PF, P]),
    'wdno_smoke_solve': (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, C.POINTER(SmokeSolveDesc), P]),
    'wdno_smoke_generate': (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, C.POINTER(SmokeGenerateDesc), P]),
    'wdno_smoke_noise': (I, [P, P, P, P, I, C.c_uint64, P, P]),
    'wdno_smoke_reconstruct': (I, [P, P, P, C.POINTER(SmokeReconstructDesc), PF, P]),
    'wdno_smoke_score': (I, [P, C.POINTER(SmokeScoreChannel), P, I, I, I, I, P]),
    'wdno_smoke_reconstruct_at': (I, [P, P, P, C.POINTER(SmokeReconstructDesc), I, PF, P]),
    'wdno_smoke_cascade_conditions': (I, [P, P, P, P, P, C.POINTER(SmokeCascadeDesc), PF, P]),
    'wdno_smoke_score_super': (I, [P, C.POINTER(SmokeScoreChannel), P, I, I, I, I, P]),
    'wdno_burgers_reconstruct': (I, [P, P, P, P, C.POINTER(BurgersReconstructDesc), PF, P]),
    'wdno_burgers_score': (I, [P, P, P, P, P, C.POINTER(BurgersScoreDesc), P]),
    'wdno_burgers_cascade_conditions': (I, [P, P, P, P, C.POINTER(BurgersCascadeDesc), PF, P]),
}

_lib = None


def load():
    """Load the shared library and attach prototypes. Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(there is no CPU / eager fallback for the wdno_amd hot path)')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)      # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    if os.environ.get('WDNO_DEBUG'):          # kernel-selection switches for A/B measurements (csrc/debug_modes.h is the list)
        try:
            check(lib.wdno_set_debug(int(os.environ['WDNO_DEBUG'])), f"WDNO_DEBUG={os.environ['WDNO_DEBUG']}")
        except RuntimeError:
            _lib = None                       # a stale number raises on every load(), not only the first
            raise
    return lib


def check(code, what):
    if code != 0:
        lib = load()
        msg = lib.wdno_strerror(code).decode()
        hip = lib.wdno_last_hip_error().decode() if code == -2 else ''
        raise RuntimeError(f'{what} failed: {msg} ({code}) {hip}')


@contextlib.contextmanager
def debug_mode(mode):
    """Run the body under library debug mode `mode` (csrc/debug_modes.h), back to 0 on exit. Raises if the library refuses the number."""
    lib = load()
    check(lib.wdno_set_debug(mode), f'wdno_set_debug({mode})')
    try:
        yield
    finally:
        lib.wdno_set_debug(0)
