"""ctypes binding of libm355seg.so (include/m355seg.h).

There is NO fallback: if the HIP library has not been built the import of any
op raises, and ops called with non-GPU tensors raise.  The product path never
touches oracle/.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# M355_LIB_PATH: load another build of the SAME library (the diagnostic build with in-kernel cycle stamps,
# build.py --stamps); never a fallback -- a missing file fails exactly like a missing product library.
LIB_PATH = os.environ.get("M355_LIB_PATH") or os.path.join(_HERE, "libm355seg.so")

M355_OK = 0
M355_EUNSUPPORTED = -2
ACT_NONE, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2
ACT_ELU, ACT_GELU, ACT_GELU_TANH, ACT_SILU = 3, 4, 5, 6   # smooth: evaluated in fp32 in every flow (csrc/activation.hpp)
COMPUTE_F32, COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32X3 = 0, 1, 2, 3
CONV_W_PACKED, CONV_SOFTMAX, CONV_SIGMOID = 1, 2, 4


class ConvDesc(C.Structure):
    """m355_conv3d_desc"""
    _fields_ = [
        ("N", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
        ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("out_pad", C.c_int32),
        ("x_batch_stride", C.c_int64), ("y_batch_stride", C.c_int64),
        ("compute", C.c_int32), ("flags", C.c_int32),
    ]


class PackItem(C.Structure):
    """m355_pack_item"""
    _fields_ = [("desc", ConvDesc), ("which", C.c_int32), ("w", C.c_void_p), ("packed", C.c_void_p)]


class NormDesc(C.Structure):
    """m355_norm_desc"""
    _fields_ = [
        ("N", C.c_int32), ("C", C.c_int32), ("S", C.c_int64),
        ("groups", C.c_int32), ("act", C.c_int32),
        ("eps", C.c_float), ("act_slope", C.c_float),
        ("x_batch_stride", C.c_int64), ("y_batch_stride", C.c_int64), ("add_batch_stride", C.c_int64),
    ]


class AugStage(C.Structure):
    """m355_aug_stage"""
    _fields_ = [("op", C.c_int32), ("order", C.c_int32), ("a", C.c_float), ("b", C.c_float), ("seed", C.c_uint64),
                ("stats", C.c_void_p), ("vec", C.c_void_p)]


AUG_BIAS, AUG_RESCALE, AUG_GAMMA, AUG_NOISE = 0, 1, 2, 3
AUG_MAX_STAGES = 8

PRE_U8, PRE_BOOL, PRE_I32, PRE_I64, PRE_F32 = 0, 1, 2, 3, 4
PRE_MASK_NONE, PRE_MASK_HALF, PRE_MASK_MAP = 0, 1, 2
PRE_MAX_REMAP = 8
PRE_MAX_ENTRIES = 8


class PreGatherDesc(C.Structure):
    """m355_pre_gather_desc"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("in_dtype", C.c_int32), ("out_dtype", C.c_int32),
                ("C", C.c_int32), ("src3", C.c_int32 * 3), ("base3", C.c_int32 * 3), ("in3", C.c_int32 * 3), ("out3", C.c_int32 * 3), ("off3", C.c_int32 * 3),
                ("off_dev", C.c_void_p), ("pad_mode", C.c_int32), ("pad_value", C.c_double), ("tables", C.c_void_p),
                ("replace_nan", C.c_int32), ("nan_value", C.c_double), ("nremap", C.c_int32),
                ("remap_old", C.c_double * PRE_MAX_REMAP), ("remap_new", C.c_double * PRE_MAX_REMAP),
                ("mask_kind", C.c_int32), ("mask_axis", C.c_int32), ("mask_upper", C.c_int32),
                ("mask_map", C.c_void_p), ("mask_dtype", C.c_int32), ("mask_C", C.c_int32)]


class PreLabelEntry(C.Structure):
    """m355_pre_label_entry"""
    _fields_ = [("map", C.c_void_p), ("dtype", C.c_int32), ("C", C.c_int32), ("one_hot", C.c_int32),
                ("weight", C.c_float), ("id", C.c_double)]

EV_BOOL, EV_U8, EV_I8, EV_I16, EV_I32, EV_I64, EV_F32, EV_BF16, EV_F16 = range(9)
EV_MASK_NONE, EV_MASK_HALF, EV_MASK_MAP = 0, 1, 2
EV_TARGET_NONE, EV_TARGET_ONEHOT, EV_TARGET_MAP = 0, 1, 2
EV_MAX_LABELS = 64
EV_MAX_CHANNELS = 64


class EvalMapDesc(C.Structure):
    """m355_eval_map_desc"""
    _fields_ = [("pred", C.c_void_p), ("target", C.c_void_p), ("S", C.c_int64), ("pred_dtype", C.c_int32),
                ("target_dtype", C.c_int32)]


class EvalScoresDesc(C.Structure):
    """m355_eval_scores_desc"""
    _fields_ = [("scores", C.c_void_p), ("target", C.c_void_p), ("mask", C.c_void_p), ("pred_out", C.c_void_p),
                ("target_out", C.c_void_p), ("size3", C.c_int32 * 3), ("target_kind", C.c_int32),
                ("target_dtype", C.c_int32), ("mask_dtype", C.c_int32)]


SLICE_MAX_DIM = 2048
EDT_MAX_DIM = 512
PLANE_SAGGITAL, PLANE_CORONAL, PLANE_AXIAL = 0, 1, 2


class RegionImage(C.Structure):
    """m355_region_image"""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("channels", C.c_int32)]


class EvalMultilabelDesc(C.Structure):
    """m355_eval_multilabel_desc"""
    _fields_ = [("scores", C.c_void_p), ("target", C.c_void_p), ("S", C.c_int64), ("target_dtype", C.c_int32)]


CAL_MAX_BINS = 32
CAL_CATEGORICAL, CAL_BINARY = 0, 1
UQ_CATEGORICAL, UQ_BINARY = 0, 1


class EvalCalibrationDesc(C.Structure):
    """m355_eval_calibration_desc"""
    _fields_ = [("scores", C.c_void_p), ("target", C.c_void_p), ("S", C.c_int64), ("target_dtype", C.c_int32)]


class SliceCountsDesc(C.Structure):
    """m355_slice_counts_desc"""
    _fields_ = [("data", C.c_void_p), ("counts_offset", C.c_int64), ("size3", C.c_int32 * 3), ("dtype", C.c_int32),
                ("channels", C.c_int32)]


class SliceSeg(C.Structure):
    """m355_slice_seg"""
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("reserved", C.c_int32)]


class SliceTileDesc(C.Structure):
    """m355_slice_tile_desc"""
    _fields_ = [("src", C.c_void_p), ("dtype", C.c_int32), ("size3", C.c_int32 * 3), ("plane", C.c_int32),
                ("slice", C.c_int32), ("row0", C.c_int32), ("col0", C.c_int32)]


class SliceMosaicDesc(C.Structure):
    """m355_slice_mosaic_desc"""
    _fields_ = [("out", C.c_void_p), ("dtype", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("tile_h", C.c_int32), ("tile_w", C.c_int32), ("ncol", C.c_int32), ("ntiles", C.c_int32),
                ("first_tile", C.c_int32), ("pad", C.c_float)]


OPTIM_SGD, OPTIM_ADAM, OPTIM_ADAMW = 0, 1, 2
OPTIM_MAX_GROUPS = 16
OPTIM_STATE_WORDS = 72
# words of the optimizer state record (include/m355seg.h)
OPTIM_ST_NORM, OPTIM_ST_CLIP, OPTIM_ST_SKIP, OPTIM_ST_T, OPTIM_ST_LR = 0, 1, 5, 6, 8


class OptimTensor(C.Structure):
    """m355_optim_tensor"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state1", C.c_void_p), ("state2", C.c_void_p),
                ("ema", C.c_void_p), ("n", C.c_int64), ("blk0", C.c_int64), ("group", C.c_int32), ("first", C.c_int32)]


class OptimGroup(C.Structure):
    """m355_optim_group"""
    _fields_ = [("lr", C.c_double), ("weight_decay", C.c_double), ("momentum", C.c_double), ("dampening", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("nesterov", C.c_int32),
                ("reserved", C.c_int32)]


class OptimDesc(C.Structure):
    """m355_optim_desc"""
    _fields_ = [("rule", C.c_int32), ("groups", C.c_int32), ("clip", C.c_int32), ("reserved", C.c_int32),
                ("max_norm", C.c_double), ("total_steps", C.c_int64), ("power", C.c_double), ("ema_decay", C.c_double),
                ("group", OptimGroup * OPTIM_MAX_GROUPS)]


_P = C.c_void_p
ABI_VERSION = 3  # M355_ABI_VERSION of include/m355seg.h this binding was written against
_i32, _i64, _f32, _sz = C.c_int32, C.c_int64, C.c_float, C.c_size_t
_CD, _ND = C.POINTER(ConvDesc), C.POINTER(NormDesc)
_I3, _D, _AS = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(AugStage)

# name -> (restype, argtypes); mirrors include/m355seg.h one to one
SIGNATURES = {
    "m355_version": (C.c_int, []),
    "m355_last_error": (C.c_char_p, []),
    "m355_reload_tuning": (None, []),
    "m355_queue_pool_bytes": (_sz, []),
    "m355_queue_pool_set": (C.c_int, [_P, _sz, _i32]),
    "m355_overflow_flag_set": (C.c_int, [_P, _i32]),
    "m355_conv3d_fuses_softmax": (_i32, [_CD]),
    "m355_conv3d_fuses_sigmoid": (_i32, [_CD]),
    "m355_conv3d_packed_bytes": (_sz, [_CD, _i32]),
    "m355_conv3d_pack": (C.c_int, [_CD, _i32, _P, _P, _P]),
    "m355_conv3d_pack_batch": (C.c_int, [_P, _i32, _P]),
    "m355_conv3d_fwd_workspace": (_sz, [_CD]),
    "m355_conv3d_fwd": (C.c_int, [_CD, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_conv3d_stats_slots": (_i64, [_CD]),
    "m355_conv3d_fwd_stats": (C.c_int, [_CD, _P, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_act16_bytes": (_sz, [_i32, _i32, _i64]),
    "m355_act16_pack": (C.c_int, [_P, _P, _i32, _i32, _i64, _i64, _i64, _i32, _P]),
    "m355_act16_unpack": (C.c_int, [_P, _P, _i32, _i32, _i64, _i64, _i64, _i32, _P]),
    "m355_conv3d_h16_workspace": (_sz, [_CD, _i32]),
    "m355_conv3d_fwd_h16": (C.c_int, [_CD, _P, _i64, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_conv3d_stats_slots_c8": (_i64, [_CD]),
    "m355_conv3d_fwd_h16_c8": (C.c_int, [_CD, _P, _i64, _P, _P, _P, _i64, _P, _P, _sz, _P]),
    "m355_conv3d_bwd_data_h16": (C.c_int, [_CD, _P, _i64, _P, _P, _P, _sz, _P]),
    "m355_conv3d_bwd_weight_h16_workspace": (_sz, [_CD]),
    "m355_conv3d_bwd_weight_h16": (C.c_int, [_CD, _P, _i64, _P, _i64, _P, _P, _P, _P, _sz, _P]),
    "m355_norm_act_fwd_h16": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _P, _i64, _i32, _P]),
    "m355_norm_act_fwd_c8": (C.c_int, [_ND, _P, _i64, _P, _P, _P, _P, _P, _i64, _P, _i64, _i32, _P]),
    "m355_act16_partials_slots": (_i64, [_i64]),
    "m355_act16_channel_partials": (C.c_int, [_P, _i64, _i32, _i32, _i64, _i32, _P, _P]),
    "m355_avgpool3d_2x_fwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_act16_pack_scaled": (C.c_int, [_P, _P, _i32, _i32, _i64, _i64, _i64, _i32, _f32, _P]),
    "m355_act16_unpack_scaled": (C.c_int, [_P, _P, _i32, _i32, _i64, _i64, _i64, _i32, _f32, _P]),
    "m355_conv3d_bwd_data_h16_c8": (C.c_int, [_CD, _P, _i64, _P, _P, _i64, _P, _sz, _P]),
    "m355_conv3d_bwd_weight_c8_workspace": (_sz, [_CD]),
    "m355_conv3d_bwd_weight_c8": (C.c_int, [_CD, _P, _i64, _P, _i64, _P, _P, _f32, _P, _sz, _P]),
    "m355_norm_act_bwd_c8": (C.c_int, [_ND, _P, _i64, _P, _i64, _P, _i64, _i32, _i32, _i32, _P, _P, _P, _P, _P, _i64, _P, _P,
                                       C.c_int, _f32, _i32, _P, _sz, _P]),
    "m355_norm_act_bwd_c8_reduce": (C.c_int, [_ND, _P, _i64, _P, _i64, _P, _i64, _i32, _i32, _i32, _P, _P, _P, _P, _P, _P,
                                              C.c_int, _P, _f32, _P, _i32, _P, _sz, _P]),
    "m355_norm_act_bwd_c8_apply": (C.c_int, [_ND, _P, _i64, _P, _i64, _P, _i64, _i32, _i32, _i32, _P, _P, _P, _P, _P, _P, _i64,
                                             _i32, _P]),
    "m355_avgpool3d_2x_bwd_h16": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _P]),
    "m355_upsample_trilinear2x_fwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_upsample_trilinear2x_bwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_act16_channel_scale": (C.c_int, [_P, _P, _P, _i32, _i32, _i64, _i64, _i64, _i32, _P]),
    "m355_space_to_depth2_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_depth_to_space2_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_conv_transpose3d_h16_bwd_supported": (_i32, [_CD]),
    "m355_conv_transpose3d_h16_bwd_workspace": (_sz, [_CD]),
    "m355_conv_transpose3d_bwd_data_h16": (C.c_int, [_CD, _P, _i64, _P, _P, _i64, _i32, _P]),
    "m355_conv_transpose3d_bwd_weight_h16": (C.c_int, [_CD, _P, _i64, _P, _i64, _P, _P, _f32, _i32, _P, _sz, _P]),
    "m355_conv3d_plan": (C.c_int, [_CD, _i32, C.POINTER(C.c_int32)]),
    "m355_conv3d_launch_plan": (C.c_int, [_i32, _CD, C.POINTER(_i64), C.POINTER(C.c_uint64), _sz, C.POINTER(_i64)]),
    "m355_conv3d_bwd_data_workspace": (_sz, [_CD]),
    "m355_conv3d_bwd_data": (C.c_int, [_CD, _P, _P, _P, _P, _sz, _P]),
    "m355_conv3d_bwd_weight_workspace": (_sz, [_CD]),
    "m355_conv3d_bwd_weight": (C.c_int, [_CD, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_conv_transpose3d_workspace": (_sz, [_CD]),
    "m355_conv_transpose3d_plan": (C.c_int, [_CD, _i32, _P, C.POINTER(C.c_int32)]),
    "m355_conv_transpose3d_fwd": (C.c_int, [_CD, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_conv_transpose3d_bwd_data": (C.c_int, [_CD, _P, _P, _P, _P, _sz, _P]),
    "m355_conv_transpose3d_bwd_weight": (C.c_int, [_CD, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_conv_transpose3d_fwd_h16": (C.c_int, [_CD, _P, _i64, _P, _P, _P, _i64, _i32, _P]),
    "m355_conv_transpose3d_x3_bwd_supported": (_i32, [_CD, _P]),
    "m355_conv_transpose3d_x3_bwd_workspace": (_sz, [_CD]),
    "m355_conv_transpose3d_x3_bwd_plan": (C.c_int, [_CD, _i32, _P, C.POINTER(C.c_int32)]),
    "m355_conv_transpose3d_bwd_data_x3": (C.c_int, [_CD, _P, _P, _P, _P, _sz, _P]),
    "m355_conv_transpose3d_bwd_weight_x3": (C.c_int, [_CD, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_norm_num_stats": (_i64, [_ND]),
    "m355_norm_workspace": (_sz, [_ND]),
    "m355_norm_plan": (C.c_int, [_ND, _i32, C.POINTER(C.c_int32)]),
    "m355_norm_stats": (C.c_int, [_ND, _P, _P, _P, _P, _P, _f32, _P, _sz, _P]),
    "m355_norm_stats_from_partials": (C.c_int, [_ND, _P, _i64, _P, _P, _P, _P, _f32, _P, _sz, _P]),
    "m355_norm_stats_from_running": (C.c_int, [_ND, _P, _P, _P, _P, _P]),
    "m355_norm_act_fwd": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _P]),
    "m355_norm_act_pool_fwd": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _i64, _i32, _i32, _i32, _P]),
    "m355_norm_act_bwd": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _sz, _P]),
    "m355_norm_act_bwd_pool": (C.c_int, [_ND, _P, _P, _i64, _P, _i64, _i32, _i32, _i32, _P, _P, _P, _P, _P, _P, _P, C.c_int,
                                         _P, _sz, _P]),
    "m355_norm_sums": (C.c_int, [_ND, _P, _P, _i64, _P, _P, _sz, _P]),
    "m355_norm_stats_from_sums": (C.c_int, [_ND, _P, _P, _P, _P, _P, _f32, _P]),
    "m355_norm_act_bwd_reduce": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _sz, _P]),
    "m355_norm_act_bwd_apply": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i64, _i32, _P]),
    "m355_norm_act_bwd_h16": (C.c_int, [_ND, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _i64, _i32, _P, _sz, _P]),
    "m355_resample_plan": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(C.c_uint64), _i32,
                                     C.POINTER(_i64)]),
    "m355_avgpool3d_2x_fwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_avgpool3d_2x_bwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_avgpool3d_2x_bwd_add": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _P]),
    "m355_maxpool3d_2x_fwd": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_maxpool3d_2x_bwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _P]),
    "m355_maxpool3d_2x_fwd_h16": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_maxpool3d_2x_bwd_h16": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _P]),
    "m355_upsample_trilinear2x_fwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_upsample_trilinear2x_bwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_upsample_nearest2x_fwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_upsample_nearest2x_bwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_upsample_trilinear2x_hp_fwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_upsample_trilinear2x_hp_bwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_upsample_nearest2x_fwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_upsample_nearest2x_bwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_upsample_trilinear2x_hp_fwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_upsample_trilinear2x_hp_bwd_h16": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _P]),
    "m355_upsample2x_plan": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(C.c_uint64),
                                       _i32, C.POINTER(_i64)]),
    "m355_softmax_fwd": (C.c_int, [_P, _P, _i32, _i32, _i32, _i64, _f32, _P]),
    "m355_softmax_bwd": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i64, _P]),
    "m355_sigmoid_fwd": (C.c_int, [_P, _P, _i64, _P]),
    "m355_sigmoid_bwd": (C.c_int, [_P, _P, _P, _i64, _P]),
    "m355_hybrid_loss_workspace": (_sz, [_i32, _i32, _i64]),
    "m355_hybrid_loss_fwd": (C.c_int, [_P, _P, _i32, _i32, _i64, _f32, _P, _i32, _P, _P, _P, _sz, _P]),
    "m355_hybrid_loss_bwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i64, _f32, _P, _i32, _P, _P]),
    "m355_binary_loss_workspace": (_sz, [_i32, _i32, _i64]),
    "m355_binary_loss_fwd": (C.c_int, [_P, _P, _i32, _i32, _i64, _f32, _P, _P, _i32, _i32, _P, _P, _P, _sz, _P]),
    "m355_binary_loss_bwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i64, _f32, _P, _P, _i32, _i32, _P, _P]),
    "m355_focal_tversky_workspace": (_sz, [_i32, _i32, _i64]),
    "m355_focal_tversky_fwd": (C.c_int, [_P, _P, _i32, _i32, _i64, _f32, _f32, _f32, _f32, _f32, _P, _P, _i32, _P, _P, _P, _sz, _P]),
    "m355_focal_tversky_bwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i64, _f32, _f32, _f32, _f32, _f32, _P, _P, _i32, _P, _P]),
    "m355_topk_loss_workspace": (_sz, [_i32, _i32, _i64]),
    "m355_topk_loss_fwd": (C.c_int, [_P, _P, _i32, _i32, _i64, _i64, _P, _f32, _P, _i32, _i32, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_topk_loss_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _i32, _i32, _i64, _f32, _P, _i32, _i32, _P, _P]),
    "m355_segmented_sort_workspace": (_sz, [_i64, _i64]),
    "m355_segmented_sort_tile": (_i32, []),
    "m355_segmented_sort_u32": (C.c_int, [_P, _P, _i64, _i64, _i32, _P, _sz, _P]),
    "m355_lovasz_loss_workspace": (_sz, [_i32, _i32, _i64, _i32]),
    "m355_lovasz_loss_tile": (_i32, []),
    "m355_lovasz_loss_fwd": (C.c_int, [_P, _P, _i32, _i32, _i64, _i32, _i32, _P, _P, _P, _P, _P, _P, _sz, _P]),
    "m355_lovasz_loss_bwd": (C.c_int, [_P, _P, _P, _P, _P, _P, _i32, _i32, _i64, _i32, _P, _P]),
    "m355_target_pyramid_elems": (_i64, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "m355_target_pyramid": (C.c_int, [_P, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _P, _P]),
    "m355_copy_channels": (C.c_int, [_P, _P, _i32, _i32, _i64, _i64, _i64, _P]),
    "m355_channel_scale": (C.c_int, [_P, _P, _P, _i32, _i32, _i64, _P]),
    "m355_add": (C.c_int, [_P, _P, _P, _i64, _P]),
    "m355_space_to_depth2": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_depth_to_space2": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _P]),
    "m355_blur_weight_fwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i32, _i32, _P]),
    "m355_blur_weight_bwd": (C.c_int, [_P, _P, _P, _P, _P, _i32, _i32, _i32, _i32, _P]),
    "m355_weight_standardize_fwd": (C.c_int, [_P, _P, _P, _i32, _i32, _P]),
    "m355_weight_standardize_bwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _P]),
    "m355_sampler_table_bytes": (_sz, [_i32, _i32, _i32]),
    "m355_sampler_build": (C.c_int, [_P] + [_i32] * 6 + [_P, _P]),
    "m355_sampler_draw": (C.c_int, [_P, _P] + [_i32] * 6 + [_P, _i32, _P, _P]),
    "m355_patch_gather": (C.c_int, [_P, _P, _P] + [_i32] * 8 + [_P]),
    "m355_patch_aggregate_grid": (C.c_int, [_P, _P, _i32, _i32, _i32, _P] + [_i32] * 10 + [_P]),
    "m355_patch_aggregate_grid_weighted": (C.c_int, [_P, _P, _i32, _i32, _i32, _P, _P] + [_i32] * 10 + [_P]),
    "m355_patch_accumulate": (C.c_int, [_P, _P, _P, _P] + [_i32] * 8 + [_P]),
    "m355_patch_gather_padded": (C.c_int, [_P, _P, _P] + [_i32] * 12 + [_f32, _P]),
    "m355_patch_finalize_crop": (C.c_int, [_P, _P, _P] + [_i32] * 7 + [_P]),
    "m355_patch_finalize": (C.c_int, [_P, _P, _P, _i32, _i64, _P]),
    "m355_flip_permute": (C.c_int, [_P, _P, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i32, _P]),
    "m355_ensemble_accumulate": (C.c_int, [_P, _P, _P, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i32, _i32,
                                           _i32, _P]),
    "m355_ensemble_finalize": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i64, _i32, _i32, _P]),
    "m355_argmax_confusion": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _i64, _P]),
    "m355_ccl_workspace": (_sz, [_i32, _i32, _i32]),
    "m355_ccl_label": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i32, _i32, _P, _sz, _P]),
    "m355_label_histogram": (C.c_int, [_P, _P, _i64, _i64, _i64, _i64, _P, _P, _P]),
    "m355_masked_dilate6": (C.c_int, [_P, _P, _i32, _i32, _i32, _P, _P, _P, _P, _i32, _P, _P]),
    "m355_label_convert_in": (C.c_int, [_P, _i32, _i32, _P, _i64, _P, _P]),
    "m355_label_convert_out": (C.c_int, [_P, _P, _P, _P, _i32, _i64, _P]),
    "m355_aug_resample": (C.c_int, [_P, _P, _i32, _I3, _I3, _i32, _i32, _D, _D, _P, _I3, _P, C.c_double, _P]),
    "m355_aug_prefilter": (C.c_int, [_P, _i32, _I3, _P]),
    "m355_aug_workspace": (_sz, []),
    "m355_aug_order_stats": (C.c_int, [_P, _i32, _I3, _AS, _i32, _i32, C.POINTER(C.c_int64), _D, _P, _P, _sz, _P]),
    "m355_aug_intensity": (C.c_int, [_P, _P, _i32, _I3, _AS, _i32, _P]),
    "m355_aug_blur": (C.c_int, [_P, _P, _i32, _I3, _i32, C.c_double, _AS, _i32, _P]),
    "m355_aug_otsu_pad": (C.c_int, [_P, _i32, _I3, _P, _P]),
    "m355_aug_channel_minmax": (C.c_int, [_P, _i32, _I3, _i32, _P, _P, _sz, _P]),
    "m355_pre_bbox": (C.c_int, [_P, _i32, _i32, _I3, _i32, _i32, C.c_double, _P, _P]),
    "m355_pre_crop_or_pad_offsets": (C.c_int, [_P, _I3, _I3, _P, _P]),
    "m355_pre_min_tables_bytes": (_sz, [_i32, _I3]),
    "m355_pre_min_tables": (C.c_int, [_P, _i32, _i32, _I3, _i32, C.c_double, _P, _sz, _P]),
    "m355_pre_gather": (C.c_int, [C.POINTER(PreGatherDesc), _P]),
    "m355_pre_one_hot": (C.c_int, [_P, _i32, _I3, _i32, _P, _P, _P]),
    "m355_pre_image_from_labels": (C.c_int, [C.POINTER(PreLabelEntry), _i32, _I3, _i32, _P, _P]),
    "m355_dwi_mean": (C.c_int, [_P, _i32, _I3, _P, _i32, _P, _P]),
    "m355_eval_confusion": (C.c_int, [C.POINTER(EvalMapDesc), _i32, _P, _I3, _i32, _i32, _P, _P]),
    "m355_eval_scores": (C.c_int, [C.POINTER(EvalScoresDesc), _i32, _P, _i32, _i32, _I3, _i32, _i32, _i32, _I3, _i32,
                                   _i32, _P, _P]),
    "m355_eval_multilabel": (C.c_int, [C.POINTER(EvalMultilabelDesc), _i32, _P, _i32, _i32, C.POINTER(C.c_float), _P, _P]),
    "m355_eval_calibration_workspace": (_sz, [_i32]),
    "m355_eval_calibration": (C.c_int, [C.POINTER(EvalCalibrationDesc), _i32, _P, _i32, _i32, _i32, _i32, _i32, _P, _P, _P, _P,
                                        _P, _P, _sz, _P]),
    "m355_predictive_entropy": (C.c_int, [_P, _i32, _P, _P, _i32, _i32, _i64, _i32, _P]),
    "m355_ensemble_entropy_accumulate": (C.c_int, [_P, _P, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i32,
                                                   _i32, _i32, _P]),
    "m355_ensemble_uncertainty_finalize": (C.c_int, [_P, _P, _P, _P, _P, _P, _i32, _i32, _i64, _i32, _i32, _P]),
    "m355_slice_counts": (C.c_int, [C.POINTER(SliceCountsDesc), _i32, _P, _P, _P]),
    "m355_slice_rank": (C.c_int, [_P, C.POINTER(SliceSeg), _i32, _P, _P, _P, _P, _P]),
    "m355_slice_mosaic": (C.c_int, [C.POINTER(SliceMosaicDesc), _i32, C.POINTER(SliceTileDesc), _i32, _P, _P]),
    "m355_edt_workspace": (_sz, [_I3]),
    "m355_edt_sq": (C.c_int, [_P, _I3, C.POINTER(C.c_float), _P, _P, _P]),
    "m355_edt_sqrt": (C.c_int, [_P, _P, _i64, _P]),
    "m355_surface_mask": (C.c_int, [_P, _i32, _I3, _P, _P, _P]),
    "m355_surface_gather": (C.c_int, [_P, _P, _i64, _P, _P, _i32, _P]),
    "m355_signed_distance_workspace": (_sz, [_i32, _I3]),
    "m355_signed_distance": (C.c_int, [_P, _i32, _I3, C.POINTER(C.c_float), _P, _P, _P, _sz, _P]),
    "m355_boundary_loss_workspace": (_sz, [_i32, _i32, _i64]),
    "m355_boundary_loss_fwd": (C.c_int, [_P, _P, _P, _i32, _i32, _i64, _P, _P, _sz, _P]),
    "m355_boundary_loss_bwd": (C.c_int, [_P, _P, _P, _i32, _i32, _i64, _P, _P]),
    "m355_blob_capacity": (_i64, [_i32, _P, _i32, _i32, _i32, _i32]),
    "m355_blob_label_workspace": (_sz, [_i32, _P, _i32, _i32, _i32]),
    "m355_blob_label": (C.c_int, [_P, _i32, _P, _i32, _i32, _i32, _i32, _P, _P, _P, _P, _sz, _P]),
    "m355_blob_dice_workspace": (_sz, [_i32, _P, _i32, _i32, _i32, _i32]),
    "m355_blob_dice_tables": (_sz, [_i32, _P, _i32, _i32, _i32, _i32]),
    "m355_blob_dice_fwd": (C.c_int, [_P, _P, _P, _P, _P, _i32, _i32, _P, _i32, _i32, _i32, _i32, _i32, _P, _P, _P, _sz, _P,
                                     _sz, _P]),
    "m355_blob_dice_bwd": (C.c_int, [_P, _P, _P, _P, _i32, _i32, _P, _i32, _i32, _i32, _i32, _i32, _P, _P]),
    "m355_region_stats_workspace": (_sz, [_i32, _i32, _i32]),
    "m355_region_stats_plan": (C.c_int, [_I3]),
    "m355_region_stats": (C.c_int, [_P, _i32, _I3, C.POINTER(RegionImage), _i32, _I3, _i32, _i32, _P, _P, _P, _P, _sz, _P]),
    "m355_optim_capacity": (_i32, []),
    "m355_optim_plan": (C.c_int, [C.POINTER(_i64), _i32, _I3, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_sz)]),
    "m355_optim_norm": (C.c_int, [_P, _i32, _P, _sz, _P]),
    "m355_optim_prepare": (C.c_int, [C.POINTER(OptimDesc), _i64, _P, _sz, _P, _P, _P, _P]),
    "m355_optim_update": (C.c_int, [C.POINTER(OptimDesc), _P, _i32, _P, _P]),
}


# The factor-2 resampling family in the numbering of m355_resample_plan's `op`: (entry point, its pointer arguments as indices
# into (tensor 0, tensor 1, tensor 2, route bytes) -- the tensors in the order of its batch strides --, number of batch
# strides, its argument checks first to last: n null, d dimension <= 0, o odd size, c compute mode, a alignment).
RESAMPLE_OPS = [
    ("avgpool3d_2x_fwd", (0, 1), 2, "dno"), ("avgpool3d_2x_bwd", (0, 1), 2, "dno"), ("avgpool3d_2x_bwd_add", (0, 1, 2), 3, "dno"),
    ("upsample_trilinear2x_fwd", (0, 1), 2, "dn"), ("upsample_trilinear2x_bwd", (0, 1), 2, "dn"),
    ("space_to_depth2", (0, 1), 2, "ndoa"), ("depth_to_space2", (0, 1), 2, "ndoa"),
    ("maxpool3d_2x_fwd", (0, 1, 3), 2, "ndo"), ("maxpool3d_2x_bwd", (0, 3, 1, 2), 3, "ndo"),
    ("avgpool3d_2x_fwd_h16", (0, 1), 2, "ndoca"), ("avgpool3d_2x_bwd_h16", (0, 1, 2), 3, "cndoa"),
    ("upsample_trilinear2x_fwd_h16", (0, 1), 2, "ndca"), ("upsample_trilinear2x_bwd_h16", (0, 1), 2, "ndca"),
    ("space_to_depth2_h16", (0, 1), 2, "ondca"), ("depth_to_space2_h16", (0, 1), 2, "ondca"),
    ("maxpool3d_2x_fwd_h16", (0, 1, 3), 2, "ndoca"), ("maxpool3d_2x_bwd_h16", (0, 3, 1, 2), 3, "ndoca"),
]

# The 2x upsamplers of csrc/upsample.hip in the numbering of m355_upsample2x_plan: UPSAMPLE2X_OPS[(mode, direction, c8)] with
# mode 0 nearest / 1 half-pixel trilinear, direction 0 forward / 1 backward; entries as in RESAMPLE_OPS.
UPSAMPLE2X_MODES = ("nearest", "trilinear_hp")
UPSAMPLE2X_OPS = {
    (mode, direction, c8): ("upsample_%s2x%s_%s%s" % ("nearest" if mode == 0 else "trilinear", "_hp" if mode else "",
                                                     "bwd" if direction else "fwd", "_h16" if c8 else ""),
                            (0, 1), 2, "ndca" if c8 else "dn")
    for mode in (0, 1) for direction in (0, 1) for c8 in (0, 1)
}



def resample_args(op, shape, strides, pointers, compute):
    """the argument tuple of entry point RESAMPLE_OPS[op] (op a (mode, direction, c8) tuple: UPSAMPLE2X_OPS[op]) for what
    m355_resample_plan / m355_upsample2x_plan takes (stream: the default one)"""
    _, order, nstrides, checks = UPSAMPLE2X_OPS[op] if isinstance(op, tuple) else RESAMPLE_OPS[op]
    return (tuple(C.c_void_p(pointers[i]) for i in order) + tuple(shape) + tuple(strides[:nstrides])
            + ((compute,) if "c" in checks else ()) + (None,))


# The launching conv entry points in the numbering of m355_conv3d_launch_plan's `entry`: (entry point, its arguments after the
# descriptor: 0..6 = that slot of the query's `pointers`, "s0" / "s1" = that one of its `batch_strides`, "b" = workspace_bytes,
# "u" = grad_unscale).
CONV_ENTRIES = [
    ("conv3d_fwd", (0, 1, 2, 3, 4, 6, "b")), ("conv3d_fwd_stats", (0, 1, 2, 3, 4, 5, 6, "b")),
    ("conv3d_bwd_data", (0, 1, 4, 6, "b")), ("conv3d_bwd_weight", (0, 1, 4, 5, 6, "b")),
    ("conv3d_fwd_h16", (0, "s0", 1, 2, 3, 4, 5, 6, "b")), ("conv3d_fwd_h16_c8", (0, "s0", 1, 2, 4, "s1", 5, 6, "b")),
    ("conv3d_bwd_data_h16", (0, "s0", 1, 4, 6, "b")), ("conv3d_bwd_data_h16_c8", (0, "s0", 1, 4, "s1", 6, "b")),
    ("conv3d_bwd_weight_h16", (0, "s0", 1, "s1", 2, 4, 5, 6, "b")), ("conv3d_bwd_weight_c8", (0, "s0", 1, "s1", 4, 5, "u", 6, "b")),
]


def conv_entry_args(entry, desc, strides, pointers, workspace_bytes):
    """the argument tuple of entry point CONV_ENTRIES[entry] for what m355_conv3d_launch_plan takes (stream: the default one)"""
    other = {"s0": strides[0], "s1": strides[1], "b": workspace_bytes, "u": 1.0}
    return (C.byref(desc),) + tuple(C.c_void_p(pointers[k]) if isinstance(k, int) else other[k] for k in CONV_ENTRIES[entry][1]) \
        + (None,)


class M355Error(RuntimeError):
    pass


def bind(lib, prefix="m355_"):
    """Declare argtypes/restype of every ABI symbol on a loaded CDLL.

    `prefix` lets the test-suite bind the CPU oracle (m355o_*) with the same
    signatures; the product only ever binds "m355_".
    """
    for name, (res, args) in SIGNATURES.items():
        sym = prefix + name[len("m355_"):]
        fn = getattr(lib, sym, None)
        if fn is None:
            if prefix == "m355_":
                raise M355Error(f"{LIB_PATH} does not export {sym}")
            continue
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def lib():
    """The loaded HIP library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise M355Error(
                f"HIP extension {LIB_PATH} is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, no GPU). "
                "There is no CPU or PyTorch fallback for the hot path.")
        _lib = bind(C.CDLL(LIB_PATH))
        if _lib.m355_version() != ABI_VERSION:
            raise M355Error(f"ABI version mismatch: library reports {_lib.m355_version()}, expected {ABI_VERSION}")
    return _lib


_queue_pools = {}   # device index -> the zero-filled tensor handed to m355_queue_pool_set (kept alive here)


def ensure_queue_pool(device):
    """Hand the library its work-queue pool for `device` from torch's allocator (once per device): with this host the
    library never allocates device memory itself (include/m355seg.h, "Conventions")."""
    idx = device.index if device.index is not None else 0
    if idx in _queue_pools:
        return
    import torch
    L = lib()
    n = int(L.m355_queue_pool_bytes())
    with torch.cuda.device(idx):
        if torch.cuda.is_current_stream_capturing():
            return   # (a capture's warm-up ran eagerly before: the pool exists unless the caller skipped the warm-up)
        buf = torch.zeros(n, dtype=torch.uint8, device=device)
        torch.cuda.current_stream().synchronize()
    rc = L.m355_queue_pool_set(C.c_void_p(buf.data_ptr()), n, idx)
    # M355_EUNSUPPORTED: another binding in this process already set / allocated one -- fine, it is in use
    _queue_pools[idx] = buf if rc == M355_OK else None


def reload_tuning():
    """Re-read the M355_* environment overrides (the library caches them at load time)."""
    lib().m355_reload_tuning()


def check(rc, what):
    if rc != M355_OK:
        msg = lib().m355_last_error().decode("utf-8", "replace")
        raise M355Error(f"{what} failed (status {rc}): {msg}")
