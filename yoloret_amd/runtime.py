"""ctypes binding of libyoloret_hip.so (include/yoloret_hip.h).

PyTorch-ROCm tensors are only the containers (device memory + streams); every
arithmetic step happens in the HIP kernels behind the C-ABI.  There is no CPU
fallback: if the library is missing, loading fails loudly.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('YOLORET_LIB') or os.path.join(_HERE, 'libyoloret_hip.so')     # (YOLORET_LIB: another build of the same ABI, e.g. for same-box A/B runs)

YR_MAX_SRC = 4
ACT = {'none': 0, None: 0, 'relu6': 1, 'swish': 2, 'sigmoid': 3, 'leaky': 4}
XFORM = {'identity': 0, 'up2': 1, 'maxpool2': 2, 'maxpool4': 3, 'up2_add': 4, 'dw3': 5}
OP_STEM, OP_POINTWISE, OP_DEPTHWISE, OP_SE_MEAN, OP_SE_FC, OP_WSUM, OP_GATHER, OP_MBCONV = 1, 2, 3, 4, 5, 6, 7, 8
OP_STEMBLOCK, OP_MBLANE, OP_MBH, OP_MBX, OP_MBR, OP_MBE, OP_HEAD = 9, 10, 11, 12, 13, 14, 15
# launch-form bits packed into yr_op.k / se_reduced / reserved0, per op kind: the constant block of include/yoloret_hip.h, name by
# name without the YR_ prefix (tests/test_host_logic.py compares the two)
PWF_F32_MFMA, PWF_KSPLIT, PWF_STATIONARY, PWF_TWO_OUT = 0x10000, 0x20000, 0x40000, 0x80000      # POINTWISE se_reduced
PWDW_STRIDE_MASK, PWDW_ACT_SHIFT, PWDW_ACT_MASK = 0xff, 8, 0xff00                               # ... of an op with a 'dw3' source
PW2_ACT_MASK, PW2_POOLED = 0xff, 0x100                                                          # POINTWISE reserved0 (two outputs)
MBR_K_MASK, MBR_STREAM, MBR_SPLIT, MBR_FORM_MASK = 0x3f, 0x40, 0x80, 0xff                       # MBR / MBE k
MBR_NW_SHIFT, MBR_NW_MASK, MBR_SEGS_SHIFT, MBR_SEGS_MASK = 8, 0xff00, 16, 0xff0000
HEAD_K_MASK, HEAD_STREAM_BIT, HEAD_WALK, HEAD_PLANES = 0x1f, 0x20, 0x40, 0x80                   # HEAD k
HEAD_STREAM = HEAD_WALK | HEAD_STREAM_BIT
HEAD_ACT_SHIFT, HEAD_ACT_MASK, HEAD_TILES_SHIFT, HEAD_TILES_MASK = 8, 0xff00, 16, 0xff0000
MBH_K_MASK, MBH_TH_SHIFT, MBH_TH_MASK, MBH_TW_SHIFT, MBH_TW_MASK = 0xff, 8, 0xff00, 16, 0xff0000    # MBH / MBX k
MBH_TILE_LDS, MBH_TILE_CHAINED = 254, 255
STEMBLOCK_K_MASK, STEMBLOCK_ENTRY_SHIFT, STEMBLOCK_ENTRY_MASK, STEMBLOCK_ENTRY_MFMA = 0xff, 8, 0xff00, 1     # STEMBLOCK k
# yr_dtype: element type of activation tensors / pointwise weights (include/yoloret_hip.h)
DTYPE = {'f32': 0, 'float32': 0, None: 0, 'bf16': 1, 'bfloat16': 1, 'f16': 2, 'float16': 2, 'u8': 3, 'uint8': 3}   # (u8: images only)
DTYPE_NAME = {0: 'f32', 1: 'bf16', 2: 'f16', 3: 'u8'}
ESIZE = {0: 4, 1: 2, 2: 2, 3: 1}
VEC = {0: 4, 1: 8, 2: 8}          # channels per 16 bytes: granule of `ld` and of the pointwise k-space
TORCH_DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16, 3: torch.uint8}


def dtype_id(d):
    """'f32' | 'bf16' | 'f16' | 'float32' | 'bfloat16' | 'float16' | torch dtype | yr_dtype int -> yr_dtype int."""
    if isinstance(d, int):
        if d in DTYPE_NAME:
            return d
    elif isinstance(d, torch.dtype):
        for k, v in TORCH_DTYPE.items():
            if v == d:
                return k
    elif d in DTYPE:
        return DTYPE[d]
    raise ValueError('unsupported dtype %r (float32, bfloat16, float16)' % (d,))


def to_bits16(a, dtype):
    """float32 array -> uint16 bit patterns of the 16-bit type, round to nearest even (what the kernels' stores do)."""
    a = np.ascontiguousarray(a, np.float32)
    if dtype_id(dtype) == 2:
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def from_bits16(b, dtype):
    b = np.ascontiguousarray(b, np.uint16)
    if dtype_id(dtype) == 2:
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)
OP_NAMES = {1: 'stem', 2: 'pointwise', 3: 'depthwise', 4: 'se_mean', 5: 'se_fc', 6: 'wsum', 7: 'gather', 8: 'mbconv',
            9: 'stemblock', 10: 'mblane', 11: 'mbh', 12: 'mbx', 13: 'mbr', 14: 'mbe', 15: 'head'}


class YrSrc(ctypes.Structure):
    _fields_ = [('ptr', ctypes.c_void_p), ('buf', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
                ('c', ctypes.c_int32), ('ld', ctypes.c_int32), ('xform', ctypes.c_int32), ('dtype', ctypes.c_int32)]


class YrOp(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('act', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
                ('cin', ctypes.c_int32), ('cout', ctypes.c_int32), ('k', ctypes.c_int32), ('stride', ctypes.c_int32),
                ('nsrc', ctypes.c_int32), ('se_reduced', ctypes.c_int32),
                ('dtype', ctypes.c_int32), ('out_dtype', ctypes.c_int32),
                ('src', YrSrc * YR_MAX_SRC),
                ('out', ctypes.c_void_p), ('out_buf', ctypes.c_int32), ('out_ld', ctypes.c_int32),
                ('res', ctypes.c_void_p), ('res_buf', ctypes.c_int32), ('res_ld', ctypes.c_int32),
                ('gate', ctypes.c_void_p), ('gate_buf', ctypes.c_int32), ('gate_ld', ctypes.c_int32),
                ('wgt', ctypes.c_void_p), ('wgt_off', ctypes.c_int64),
                ('scale', ctypes.c_void_p), ('scale_off', ctypes.c_int64),
                ('shift', ctypes.c_void_p), ('shift_off', ctypes.c_int64),
                ('wgt2', ctypes.c_void_p), ('wgt2_off', ctypes.c_int64),
                ('b1', ctypes.c_void_p), ('b1_off', ctypes.c_int64),
                ('b2', ctypes.c_void_p), ('b2_off', ctypes.c_int64),
                # ABI 7: the SE tail (squeeze-excite finished by the op that produces the map)
                ('gate_out', ctypes.c_void_p), ('gate_out_buf', ctypes.c_int32), ('gate_out_ld', ctypes.c_int32),
                ('se_hidden', ctypes.c_int32), ('reserved0', ctypes.c_int32),
                ('se_w', ctypes.c_void_p), ('se_w_off', ctypes.c_int64),
                ('sync', ctypes.c_void_p)]


class YrBuf(ctypes.Structure):
    _fields_ = [('bytes_per_image', ctypes.c_int64), ('arena_off_per_image', ctypes.c_int64),
                ('external_slot', ctypes.c_int32), ('dtype', ctypes.c_int32)]


class YrIngestGeom(ctypes.Structure):
    """yr_ingest_geom: one image of a ragged batch - where it sits in the packed source and in the network input."""
    _fields_ = [('src_off', ctypes.c_int64), ('ih', ctypes.c_int32), ('iw', ctypes.c_int32), ('nh', ctypes.c_int32), ('nw', ctypes.c_int32),
                ('dy', ctypes.c_int32), ('dx', ctypes.c_int32), ('nh_f', ctypes.c_float), ('nw_f', ctypes.c_float), ('dy_f', ctypes.c_float),
                ('dx_f', ctypes.c_float), ('reserved', ctypes.c_int32 * 4)]


# the same layout for NumPy: a table is one structured array, its bytes are what the device reads
INGEST_GEOM_DTYPE = np.dtype([('src_off', '<i8'), ('ih', '<i4'), ('iw', '<i4'), ('nh', '<i4'), ('nw', '<i4'), ('dy', '<i4'), ('dx', '<i4'),
                              ('nh_f', '<f4'), ('nw_f', '<f4'), ('dy_f', '<f4'), ('dx_f', '<f4'), ('reserved', '<i4', (4,))])


class YrAugmentGeom(ctypes.Structure):
    """yr_augment_geom: one image of a ragged batch under get_random_data(train=True) - resize size, crop, window, pad, flip, the
    untruncated floats of the boxes and the four colour scalars."""
    _fields_ = [('src_off', ctypes.c_int64), ('ih', ctypes.c_int32), ('iw', ctypes.c_int32), ('rh', ctypes.c_int32), ('rw', ctypes.c_int32),
                ('cy', ctypes.c_int32), ('cx', ctypes.c_int32), ('wh', ctypes.c_int32), ('ww', ctypes.c_int32), ('py', ctypes.c_int32),
                ('px', ctypes.c_int32), ('flip', ctypes.c_int32), ('clamped', ctypes.c_int32), ('reserved', ctypes.c_int32 * 2),
                ('nh_f', ctypes.c_float), ('nw_f', ctypes.c_float), ('dy_f', ctypes.c_float), ('dx_f', ctypes.c_float),
                ('hue6', ctypes.c_float), ('sat', ctypes.c_float), ('gamma', ctypes.c_float), ('cont', ctypes.c_float)]


AUGMENT_GEOM_DTYPE = np.dtype([('src_off', '<i8'), ('ih', '<i4'), ('iw', '<i4'), ('rh', '<i4'), ('rw', '<i4'), ('cy', '<i4'), ('cx', '<i4'),
                               ('wh', '<i4'), ('ww', '<i4'), ('py', '<i4'), ('px', '<i4'), ('flip', '<i4'), ('clamped', '<i4'),
                               ('reserved', '<i4', (2,)), ('nh_f', '<f4'), ('nw_f', '<f4'), ('dy_f', '<f4'), ('dx_f', '<f4'),
                               ('hue6', '<f4'), ('sat', '<f4'), ('gamma', '<f4'), ('cont', '<f4')])

ABI_VERSION = 9   # == YR_ABI_VERSION of include/yoloret_hip.h
EXPORTS = ['yr_jpeg_workspace_bytes', 'yr_jpeg_roundtrip_batch', 'yr_augment_geometry', 'yr_augment_workspace_bytes', 'yr_augment_batch', 'yr_ingest_geometry', 'yr_ingest_batch', 'yr_last_error', 'yr_last_kernel', 'yr_abi_version', 'yr_abi_sizeof', 'yr_create', 'yr_create_from_blob', 'yr_plan_io_dims', 'yr_destroy', 'yr_load_weights', 'yr_workspace_bytes',
           'yr_forward', 'yr_forward_profile', 'yr_forward_ranges', 'yr_autotune', 'yr_get_tuning', 'yr_set_tuning', 'yr_plan_num_launches', 'yr_op_run', 'yr_head_regions', 'yr_head_walk_rows', 'yr_head_stream_rows', 'yr_pwt_chunks', 'yr_decode', 'yr_decode_zoom', 'yr_yolo_head', 'yr_correct_boxes',
           'yr_nms', 'yr_pack_detections', 'yr_letterbox', 'yr_letterbox_batch', 'yr_yolo_loss_workspace_bytes', 'yr_yolo_loss', 'yr_yolo_loss_grad', 'yr_voc_match', 'yr_encode_labels',
           'yr_linear_forward', 'yr_linear_wgrad_chunk', 'yr_linear_wgrad_workspace_bytes', 'yr_linear_wgrad', 'yr_adam_step',
           'yr_linear_dgrad', 'yr_depthwise_forward', 'yr_depthwise_dgrad', 'yr_depthwise_wgrad_chunk', 'yr_depthwise_wgrad_workspace_bytes', 'yr_depthwise_wgrad',
           'yr_bn_act_forward', 'yr_bn_act_backward',
           'yr_bn_train_chunk', 'yr_bn_train_workspace_bytes', 'yr_bn_train_forward', 'yr_bn_train_backward',
           'yr_maxpool_forward', 'yr_maxpool_backward', 'yr_upsample2_forward', 'yr_upsample2_backward',
           'yr_wsum_chunk', 'yr_wsum_workspace_bytes', 'yr_wsum_forward', 'yr_wsum_backward',
           'yr_se_chunk', 'yr_se_workspace_bytes', 'yr_se_forward', 'yr_se_backward',
           'yr_linear_wide_forward', 'yr_linear_wide_dgrad', 'yr_linear_wide_wgrad_chunk', 'yr_linear_wide_wgrad_workspace_bytes', 'yr_linear_wide_wgrad',
           'yr_conv3x3_forward', 'yr_conv3x3_dgrad', 'yr_conv3x3_wgrad_chunk', 'yr_conv3x3_wgrad_workspace_bytes', 'yr_conv3x3_wgrad']

_lib = None


class YoloretHipError(RuntimeError):
    pass


def lib():
    """Loads libyoloret_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise YoloretHipError(
                'libyoloret_hip.so is missing (%s). Build it with `python -m yoloret_amd.build` '
                '(hipcc --offload-arch=gfx950); there is no CPU fallback.' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.yr_last_error.restype = ctypes.c_char_p
        L.yr_last_kernel.restype = ctypes.c_char_p
        L.yr_abi_version.restype = ctypes.c_int
        L.yr_workspace_bytes.restype = ctypes.c_size_t
        L.yr_workspace_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.yr_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_create_from_blob.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.yr_plan_io_dims.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_destroy.argtypes = [ctypes.c_void_p]
        L.yr_destroy.restype = None
        L.yr_load_weights.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        L.yr_forward.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.yr_plan_num_launches.argtypes = [ctypes.c_void_p]
        L.yr_forward_profile.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_forward_ranges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_autotune.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
        L.yr_get_tuning.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.yr_set_tuning.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.yr_op_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_head_regions.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_head_walk_rows.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.yr_head_stream_rows.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.yr_decode.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 5
        L.yr_decode_zoom.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_float] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 5
        L.yr_yolo_head.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
            [ctypes.c_void_p] * 6
        L.yr_correct_boxes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_nms.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_float] + \
            [ctypes.c_void_p] * 3
        L.yr_pack_detections.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
        L.yr_letterbox.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_void_p]
        L.yr_letterbox_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.yr_yolo_loss_workspace_bytes.restype = ctypes.c_size_t
        L.yr_yolo_loss_workspace_bytes.argtypes = [ctypes.c_int] * 4
        L.yr_yolo_loss.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                                            ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t,
                                                                                            ctypes.c_void_p, ctypes.c_void_p]
        L.yr_yolo_loss_grad.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                                                 ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t,
                                                                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                                                                 ctypes.c_void_p]
        L.yr_voc_match.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                                                            ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_encode_labels.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
        L.yr_ingest_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_ingest_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_augment_geometry.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + \
            [ctypes.c_double] * 8 + [ctypes.c_void_p, ctypes.c_void_p]
        L.yr_augment_workspace_bytes.restype = ctypes.c_size_t
        L.yr_augment_workspace_bytes.argtypes = [ctypes.c_int] * 3
        L.yr_augment_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.yr_jpeg_workspace_bytes.restype = ctypes.c_size_t
        L.yr_jpeg_workspace_bytes.argtypes = [ctypes.c_int] * 3
        L.yr_jpeg_roundtrip_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_void_p]
        L.yr_linear_forward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p]
        L.yr_linear_wgrad_chunk.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
        L.yr_linear_wgrad_workspace_bytes.restype = ctypes.c_size_t
        L.yr_linear_wgrad_workspace_bytes.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
        L.yr_linear_wgrad.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_adam_step.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong] + [ctypes.c_float] * 4 + [ctypes.c_void_p]
        L.yr_linear_dgrad.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_void_p]
        L.yr_linear_wide_forward.argtypes = L.yr_linear_forward.argtypes
        L.yr_linear_wide_dgrad.argtypes = L.yr_linear_dgrad.argtypes
        L.yr_linear_wide_wgrad_chunk.argtypes = L.yr_linear_wgrad_chunk.argtypes
        L.yr_linear_wide_wgrad_workspace_bytes.restype = ctypes.c_size_t
        L.yr_linear_wide_wgrad_workspace_bytes.argtypes = L.yr_linear_wgrad_workspace_bytes.argtypes
        L.yr_linear_wide_wgrad.argtypes = L.yr_linear_wgrad.argtypes
        for entry in (L.yr_depthwise_forward, L.yr_depthwise_dgrad):
            entry.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 10 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_depthwise_wgrad_chunk.argtypes = [ctypes.c_int] * 5
        L.yr_depthwise_wgrad_workspace_bytes.restype = ctypes.c_size_t
        L.yr_depthwise_wgrad_workspace_bytes.argtypes = [ctypes.c_int] * 5
        L.yr_depthwise_wgrad.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 10 + \
            [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        for entry in (L.yr_conv3x3_forward, L.yr_conv3x3_dgrad):
            entry.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 10 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_conv3x3_wgrad_chunk.argtypes = [ctypes.c_int] * 5
        L.yr_conv3x3_wgrad_workspace_bytes.restype = ctypes.c_size_t
        L.yr_conv3x3_wgrad_workspace_bytes.argtypes = [ctypes.c_int] * 5
        L.yr_conv3x3_wgrad.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 10 + \
            [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.yr_bn_act_forward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_bn_act_backward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_bn_train_chunk.argtypes = [ctypes.c_longlong, ctypes.c_int]
        L.yr_bn_train_workspace_bytes.restype = ctypes.c_size_t
        L.yr_bn_train_workspace_bytes.argtypes = [ctypes.c_longlong, ctypes.c_int]
        L.yr_bn_train_forward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
        L.yr_bn_train_backward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + \
            [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
        L.yr_maxpool_forward.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_maxpool_backward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 5 + \
            [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_upsample2_forward.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_upsample2_backward.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.yr_wsum_chunk.argtypes = [ctypes.c_longlong, ctypes.c_int]
        L.yr_wsum_workspace_bytes.restype = ctypes.c_size_t
        L.yr_wsum_workspace_bytes.argtypes = [ctypes.c_longlong, ctypes.c_int]
        L.yr_wsum_forward.argtypes = [ctypes.c_void_p, ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                                          ctypes.c_void_p]
        L.yr_wsum_backward.argtypes = [ctypes.c_void_p, ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + \
            [ctypes.c_void_p, ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.yr_se_chunk.restype = ctypes.c_longlong
        L.yr_se_chunk.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
        L.yr_se_workspace_bytes.restype = ctypes.c_size_t
        L.yr_se_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
        L.yr_se_forward.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int] + \
            [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
        L.yr_se_backward.argtypes = [ctypes.c_void_p, ctypes.c_int] * 2 + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int] + \
            [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
        if L.yr_abi_version() != ABI_VERSION:
            raise YoloretHipError('libyoloret_hip.so ABI version mismatch')
        L.yr_abi_sizeof.argtypes = [ctypes.c_int]
        if INGEST_GEOM_DTYPE.itemsize != ctypes.sizeof(YrIngestGeom):
            raise YoloretHipError('INGEST_GEOM_DTYPE: %d bytes, YrIngestGeom %d' % (INGEST_GEOM_DTYPE.itemsize, ctypes.sizeof(YrIngestGeom)))
        if AUGMENT_GEOM_DTYPE.itemsize != ctypes.sizeof(YrAugmentGeom):
            raise YoloretHipError('AUGMENT_GEOM_DTYPE: %d bytes, YrAugmentGeom %d' % (AUGMENT_GEOM_DTYPE.itemsize, ctypes.sizeof(YrAugmentGeom)))
        for which, st in enumerate((YrSrc, YrOp, YrBuf, YrIngestGeom, YrAugmentGeom)):
            if L.yr_abi_sizeof(which) != ctypes.sizeof(st):
                raise YoloretHipError('struct %s: %d bytes here, %d in libyoloret_hip.so'
                                      % (st.__name__, ctypes.sizeof(st), L.yr_abi_sizeof(which)))
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise YoloretHipError('libyoloret_hip: %s (status %d)' % (lib().yr_last_error().decode(), rc))


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _require_cuda_f32(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError('%s must be a contiguous float32 CUDA tensor' % name)


def make_src(t, c=None, xform='identity', ld=None):
    """yr_src for a [B,H,W,ld] tensor (float32 / bfloat16 / float16) of which `c` channels are taken."""
    s = YrSrc()
    s.dtype = dtype_id(t.dtype)
    s.ptr = t.data_ptr()
    s.buf = -1
    s.h, s.w = t.shape[1], t.shape[2]
    s.ld = t.shape[3] if ld is None else ld
    s.c = s.ld if c is None else c
    s.xform = XFORM[xform] if isinstance(xform, str) else int(xform)
    return s


def run_op(op, batch, device=None):
    """One fused op on `device` (default: the current device) - the tensors behind its pointers must live there."""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(lib().yr_op_run(ctypes.byref(op), int(batch), stream_ptr(device)))


def new_op(kind, act='none'):
    op = YrOp()
    op.kind = kind
    op.act = ACT[act] if not isinstance(act, int) else act
    op.out_buf = op.res_buf = op.gate_buf = op.gate_out_buf = -1
    for f in ('wgt_off', 'scale_off', 'shift_off', 'wgt2_off', 'b1_off', 'b2_off', 'se_w_off'):
        setattr(op, f, -1)
    return op


# ----------------------------------------------------------------------------- post-processing wrappers
def num_boxes(in_h, in_w, num_anchors=3, num_scales=3):
    return sum((in_h // (32 >> s)) * (in_w // (32 >> s)) * num_anchors for s in range(num_scales))


# model.py:411-412: the zoom-in TTA pass is mapped back with these hard-coded constants
ZOOM_MUL = float(np.float32(224 / 416))
ZOOM_ADD = float(np.float32((416 - 224) / (2 * 416)))
ZOOM_RATIO = (224 * 224) / (416 * 416)     # utils.py:7: the central_crop fraction of the zoom pass (yolo.py:108-109)


def decode(ys, anchors, num_classes, image_hw, input_hw, num_scales=3, zoom_ys=None):
    """ys: list of [B,G,G,A*(C+5)] (or [B,G,G,A,C+5]) logits -> boxes [B,N,4], scores [B,C,N].
    zoom_ys: the logits of the zoom-in TTA pass (model.py:408-417) -> boxes [B,2N,4], scores [B,C,2N]."""
    if len(ys) < num_scales:
        raise ValueError('decode: %d logit tensors for %d scales' % (len(ys), num_scales))
    anchors = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(-1, 2))
    if anchors.shape[0] % 3 or anchors.shape[0] == 0:
        raise ValueError('decode: the anchor list must hold 3 scales x A anchors')
    a_ = anchors.shape[0] // 3
    in_h_, in_w_ = int(input_hw[0]), int(input_hw[1])
    for i, y in enumerate(ys[:num_scales]):
        _require_cuda_f32(y, 'y%d' % (i + 1))
        # the kernel derives the grids from input_hw and the strides, not from the tensors: the shapes must agree,
        # otherwise it would read past the end of y
        gh, gw = in_h_ // (32 >> i), in_w_ // (32 >> i)
        if y.dim() < 3 or tuple(y.shape[1:3]) != (gh, gw) or y[0].numel() != gh * gw * a_ * (num_classes + 5) \
                or y.shape[0] != ys[0].shape[0] or y.device != ys[0].device:
            raise ValueError('y%d has shape %s, expected [B=%d,%d,%d,%d*(%d+5)] for input %dx%d'
                             % (i + 1, tuple(y.shape), ys[0].shape[0], gh, gw, a_, num_classes, in_h_, in_w_))
    if not (isinstance(image_hw, torch.Tensor) and image_hw.dtype == torch.int32 and image_hw.is_contiguous()
            and image_hw.device == ys[0].device and tuple(image_hw.shape) == (ys[0].shape[0], 2)):
        raise ValueError('image_hw must be a contiguous int32 [B,2] tensor on the logits\' device (image_hw_tensor)')
    with torch.cuda.device(ys[0].device):
        return _decode(ys, anchors, num_classes, image_hw, input_hw, num_scales, zoom_ys)


def _decode(ys, anchors, num_classes, image_hw, input_hw, num_scales, zoom_ys):
    """anchors: the contiguous float32 [3 * A, 2] array ``decode`` made."""
    zoom = zoom_ys is not None
    if zoom:
        for i, (y, z) in enumerate(zip(ys[:num_scales], zoom_ys[:num_scales])):
            _require_cuda_f32(z, 'zoom y%d' % (i + 1))
            if z.shape != y.shape:
                raise ValueError('zoom y%d has shape %s, expected %s' % (i + 1, tuple(z.shape), tuple(y.shape)))
    b = ys[0].shape[0]
    a = anchors.shape[0] // 3
    in_h, in_w = int(input_hw[0]), int(input_hw[1])
    n = (2 if zoom else 1) * num_boxes(in_h, in_w, a, num_scales)
    dev = ys[0].device
    boxes = torch.empty((b, n, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((b, num_classes, n), dtype=torch.float32, device=dev)
    yp = [_ptr(ys[i]) if i < num_scales else None for i in range(3)]
    tail = (b, in_h, in_w, a, num_classes, num_scales, anchors.ctypes.data_as(ctypes.c_void_p), _ptr(image_hw), _ptr(boxes), _ptr(scores),
            stream_ptr(dev))
    if zoom:
        zp = [_ptr(zoom_ys[i]) if i < num_scales else None for i in range(3)]
        check(lib().yr_decode_zoom(*yp, *zp, ZOOM_MUL, ZOOM_ADD, *tail))
    else:
        check(lib().yr_decode(*yp, *tail))
    return boxes, scores


def nms(boxes, scores, max_boxes=20, score_threshold=.6, iou_threshold=.5):
    """boxes [B,N,4], scores [B,C,N] -> idx [B,C,max] int32 (-1 padded), count [B,C] int32."""
    _require_cuda_f32(boxes, 'boxes')
    _require_cuda_f32(scores, 'scores')
    if scores.dim() != 3 or tuple(boxes.shape) != (scores.shape[0], scores.shape[2], 4) or boxes.device != scores.device:
        raise ValueError('nms: boxes %s / scores %s, expected [B,N,4] / [B,C,N] on one device' % (tuple(boxes.shape), tuple(scores.shape)))
    b, c, n = scores.shape
    idx = torch.empty((b, c, max_boxes), dtype=torch.int32, device=boxes.device)
    cnt = torch.empty((b, c), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        check(lib().yr_nms(_ptr(boxes), _ptr(scores), b, n, c, int(max_boxes), float(score_threshold),
                           float(iou_threshold), _ptr(idx), _ptr(cnt), stream_ptr(boxes.device)))
    return idx, cnt


def pack_detections(boxes, scores, idx, cnt):
    """-> det [B, C*max, 6] int32 words, det_count [B] int32 (see yoloret_hip.h)."""
    b, c, n = scores.shape
    max_boxes = idx.shape[2]
    det = torch.empty((b, c * max_boxes, 6), dtype=torch.int32, device=boxes.device)
    det_count = torch.empty((b,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        check(lib().yr_pack_detections(_ptr(boxes), _ptr(scores), _ptr(idx), _ptr(cnt), b, n, c, max_boxes,
                                       _ptr(det), _ptr(det_count), stream_ptr(boxes.device)))
    return det, det_count


def yolo_head(feats, anchors, input_hw, with_scores=False):
    """feats [B,G,G,A,C+5] -> box_xy, box_wh [B,G,G,A,2], conf [B,G,G,A,1], probs [B,G,G,A,C]
    (+ scores = conf*probs [B,G,G,A,C] when with_scores)."""
    _require_cuda_f32(feats, 'feats')
    b, gh, gw, a, ch = feats.shape
    c = ch - 5
    anchors = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(-1, 2))
    if anchors.shape[0] != a:
        raise ValueError('yolo_head: %d anchors for %d anchor slots' % (anchors.shape[0], a))
    dev = feats.device
    xy = torch.empty((b, gh, gw, a, 2), dtype=torch.float32, device=dev)
    wh = torch.empty((b, gh, gw, a, 2), dtype=torch.float32, device=dev)
    conf = torch.empty((b, gh, gw, a, 1), dtype=torch.float32, device=dev)
    probs = torch.empty((b, gh, gw, a, c), dtype=torch.float32, device=dev)
    scores = torch.empty_like(probs) if with_scores else None
    with torch.cuda.device(dev):
        check(lib().yr_yolo_head(_ptr(feats), b, gh, gw, a, c, anchors.ctypes.data_as(ctypes.c_void_p),
                                 int(input_hw[0]), int(input_hw[1]), _ptr(xy), _ptr(wh), _ptr(conf), _ptr(probs),
                                 _ptr(scores), stream_ptr(dev)))
    return (xy, wh, conf, probs, scores) if with_scores else (xy, wh, conf, probs)


def _out_like(out, shape, dev, name):
    """A fresh float32 tensor of ``shape`` on ``dev``, or the caller's, which must be exactly that and contiguous."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == dev and tuple(out.shape) == tuple(shape)
            and out.is_contiguous()):
        raise ValueError('%s: out must be a contiguous float32 tensor of shape %s on %s' % (name, tuple(shape), dev))
    return out


def _workspace_arg(workspace, need, dev, name):
    """A fresh uint8 tensor of ``need`` bytes on ``dev``, or the caller's, which must be contiguous and hold at least that many."""
    if workspace is None:
        return torch.empty((need,), dtype=torch.uint8, device=dev)
    if not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
            and workspace.numel() >= need):
        raise ValueError('%s: workspace must be a contiguous uint8 tensor of at least %d bytes on %s' % (name, need, dev))
    return workspace


def yolo_loss_workspace_bytes(batch, gh, gw, num_anchors):
    return int(lib().yr_yolo_loss_workspace_bytes(int(batch), int(gh), int(gw), int(num_anchors)))


def _yolo_loss_args(name, feats, y_true, anchors, workspace):
    """The validation yolo_loss and yolo_loss_grad share -> (b, gh, gw, a, ch, anchors, device, workspace, its size)."""
    _require_cuda_f32(feats, 'feats')
    _require_cuda_f32(y_true, 'y_true')
    if feats.dim() != 5 or feats.shape[-1] < 5 or feats.numel() == 0:
        raise ValueError('%s: feats has shape %s, expected [B,gh,gw,A,5+C]' % (name, tuple(feats.shape)))
    if y_true.shape != feats.shape or y_true.device != feats.device:
        raise ValueError('%s: y_true %s on %s, expected the logits\' %s on %s'
                         % (name, tuple(y_true.shape), y_true.device, tuple(feats.shape), feats.device))
    b, gh, gw, a, ch = feats.shape
    anchors = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(-1, 2))
    if anchors.shape[0] != a:
        raise ValueError('%s: %d anchors for %d anchor slots' % (name, anchors.shape[0], a))
    if not 1 <= a <= 8:
        raise ValueError('%s: 1..8 anchor slots per cell, not %d' % (name, a))
    dev = feats.device
    return b, gh, gw, a, ch, anchors, dev, _workspace_arg(workspace, yolo_loss_workspace_bytes(b, gh, gw, a), dev, name)


def yolo_loss(feats, y_true, anchors, input_hw, ignore_thresh=.5, workspace=None):
    """YoloLoss.call, GIOU branch (model.py:607-671) for one scale.  feats, y_true [B,gh,gw,A,5+C] float32 on one device,
    anchors: the A (w,h) anchors of this scale -> float32 [5] on that device: loss, giou_loss, confidence_loss, class_loss,
    ignore_sum.  Launches only; nothing is copied to the host.  workspace: a uint8 tensor of at least
    yolo_loss_workspace_bytes(B, gh, gw, A) bytes on that device to work in (its contents do not matter); default: a fresh one."""
    b, gh, gw, a, ch, anchors, dev, ws = _yolo_loss_args('yolo_loss', feats, y_true, anchors, workspace)
    out = torch.empty((5,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_yolo_loss(_ptr(feats), _ptr(y_true), b, gh, gw, a, ch - 5, anchors.ctypes.data_as(ctypes.c_void_p),
                                 int(input_hw[0]), int(input_hw[1]), float(ignore_thresh), _ptr(ws), ws.numel(), _ptr(out),
                                 stream_ptr(dev)))
    return out


def yolo_loss_grad(feats, y_true, anchors, input_hw, ignore_thresh=.5, upstream=None, workspace=None, out=None):
    """The loss of ``yolo_loss`` and its gradient with respect to ``feats`` in one call (yr_yolo_loss_grad; the rules are in
    csrc/loss.hip) -> (terms float32 [5]: the bits ``yolo_loss`` returns, dfeats float32 of feats' shape = upstream * d loss / d feats).
    upstream: a float32 tensor of one element on the logits' device, the cotangent of the scalar loss (default: 1); it is read on
    the device.  out: a contiguous float32 tensor of feats' shape on that device to receive dfeats (every element is written);
    default: a fresh one.  Launches only."""
    b, gh, gw, a, ch, anchors, dev, ws = _yolo_loss_args('yolo_loss_grad', feats, y_true, anchors, workspace)
    if upstream is not None and not (isinstance(upstream, torch.Tensor) and upstream.dtype == torch.float32 and upstream.numel() == 1
                                     and upstream.device == dev):
        raise ValueError('yolo_loss_grad: upstream must be a float32 tensor of one element on %s' % dev)
    out = _out_like(out, feats.shape, dev, 'yolo_loss_grad')
    terms = torch.empty((5,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_yolo_loss_grad(_ptr(feats), _ptr(y_true), b, gh, gw, a, ch - 5, anchors.ctypes.data_as(ctypes.c_void_p),
                                      int(input_hw[0]), int(input_hw[1]), float(ignore_thresh), _ptr(ws), ws.numel(), _ptr(upstream),
                                      _ptr(terms), _ptr(out), stream_ptr(dev)))
    return terms, out


# ----------------------------------------------------------------------------- training the output convolutions (csrc/headtrain.hip)
def _rows(t, name):
    """A float32 CUDA tensor whose last axis holds the channels and whose leading axes are dense -> (pixels, channels)."""
    _require_cuda_f32(t, name)
    if t.dim() < 2 or t.numel() == 0:
        raise ValueError('%s has shape %s, expected [..., channels]' % (name, tuple(t.shape)))
    return t.numel() // t.shape[-1], t.shape[-1]


def _linear_wt(wt, name, limit, cin=None):
    _require_cuda_f32(wt, name)
    if wt.dim() != 2 or wt.shape[1] % 4 or not 1 <= wt.shape[0] <= limit or (cin is not None and wt.shape[1] != (cin + 3) // 4 * 4):
        raise ValueError('%s has shape %s, expected [cout, round_up(cin, 4)] with cout <= %d' % (name, tuple(wt.shape), limit))


# The 1x1 operators exist twice, up to 256 channels (csrc/headtrain.hip, csrc/convgrad.hip) and up to LINEAR_WIDE_MAX (csrc/linearwide.hip),
# behind one set of checks: ``name`` is the public function's (the prefix of its messages), ``limit`` the width it takes, ``entry`` its
# C entry (and, with '_workspace_bytes', the size of the weight gradient's workspace), looked up once the arguments have passed.
def _linear_forward(name, limit, entry, x, wt, out):
    pixels, cin = _rows(x, 'x')
    if not 1 <= cin <= limit:
        raise ValueError('%s: 1..%d channels, not %d' % (name, limit, cin))
    _linear_wt(wt, 'wt', limit, cin)
    if wt.device != x.device:
        raise ValueError('%s: wt on %s, x on %s' % (name, wt.device, x.device))
    out = _out_like(out, tuple(x.shape[:-1]) + (wt.shape[0],), x.device, name)
    with torch.cuda.device(x.device):
        check(getattr(lib(), entry)(_ptr(x), cin, _ptr(wt), pixels, cin, wt.shape[0], _ptr(out), wt.shape[0], stream_ptr(x.device)))
    return out


def _linear_dgrad(name, limit, entry, dy, wt, cin, out):
    pixels, cout = _rows(dy, 'dy')
    cin = int(cin)
    if not (1 <= cin <= limit and 1 <= cout <= limit):
        raise ValueError('%s: 1..%d channels, not %d and %d' % (name, limit, cin, cout))
    _linear_wt(wt, 'wt', limit, cin)
    if wt.device != dy.device or wt.shape[0] != cout:
        raise ValueError('%s: wt %s on %s for dy %s on %s' % (name, tuple(wt.shape), wt.device, tuple(dy.shape), dy.device))
    out = _out_like(out, tuple(dy.shape[:-1]) + (cin,), dy.device, name)
    with torch.cuda.device(dy.device):
        check(getattr(lib(), entry)(_ptr(dy), cout, _ptr(wt), pixels, cin, cout, _ptr(out), cin, stream_ptr(dy.device)))
    return out


def _linear_wgrad(name, limit, entry, x, dy, out, workspace):
    pixels, cin = _rows(x, 'x')
    pdy, cout = _rows(dy, 'dy')
    if pdy != pixels or dy.device != x.device:
        raise ValueError('%s: dy %s on %s for x %s on %s' % (name, tuple(dy.shape), dy.device, tuple(x.shape), x.device))
    if not (1 <= cin <= limit and 1 <= cout <= limit):
        raise ValueError('%s: 1..%d channels, not %d and %d' % (name, limit, cin, cout))
    dev = x.device
    out = _out_like(out, (cout, (cin + 3) // 4 * 4), dev, name)
    ws = _workspace_arg(workspace, int(getattr(lib(), entry + '_workspace_bytes')(pixels, cin, cout)), dev, name)
    with torch.cuda.device(dev):
        check(getattr(lib(), entry)(_ptr(x), cin, _ptr(dy), cout, pixels, cin, cout, _ptr(ws), ws.numel(), _ptr(out), stream_ptr(dev)))
    return out


def linear_forward(x, wt, out=None):
    """A bias-free 1x1 convolution on dense rows (yr_linear_forward): x [..., cin] float32, wt [cout, round_up(cin, 4)] (the layout of
    YR_OP_POINTWISE, pad columns 0) -> y [..., cout] = x @ wt[:, :cin].T on the float32 matrix pipe.  out: a contiguous float32
    tensor of that shape on x's device (every element is written); default: a fresh one.  One launch."""
    return _linear_forward('linear_forward', 256, 'yr_linear_forward', x, wt, out)


def linear_wgrad_chunk(pixels, cin, cout):
    """Pixels per workgroup of the gradient's first stage: a function of these three numbers only (0: sizes the call refuses)."""
    return int(lib().yr_linear_wgrad_chunk(int(pixels), int(cin), int(cout)))


def linear_wgrad_workspace_bytes(pixels, cin, cout):
    return int(lib().yr_linear_wgrad_workspace_bytes(int(pixels), int(cin), int(cout)))


def linear_wgrad(x, dy, out=None, workspace=None):
    """The weight gradient of ``linear_forward`` (yr_linear_wgrad): x [..., cin], dy [..., cout] float32 with the same leading axes
    -> dwt [cout, round_up(cin, 4)] = dy.T @ x, pad columns +0, float32 on the float32 matrix pipe; no atomics, the same call gives
    the same bytes.  out: a contiguous float32 tensor of that shape on x's device (every element is written); workspace: a uint8
    tensor of at least linear_wgrad_workspace_bytes(pixels, cin, cout) bytes there (its contents do not matter).  Defaults: fresh
    ones.  Two launches."""
    return _linear_wgrad('linear_wgrad', 256, 'yr_linear_wgrad', x, dy, out, workspace)


def adam_alpha(learning_rate, step, beta1=.9, beta2=.999):
    """Keras Adam's step size at the 1-based ``step``: float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t)), formed in float64."""
    return float(np.float32(float(learning_rate) * np.sqrt(1.0 - float(beta2) ** step) / (1.0 - float(beta1) ** step)))


def adam_step(w, m, v, g, alpha, beta1=.9, beta2=.999, eps=1e-8):
    """Keras Adam's dense update in place (yr_adam_step): m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g g;
    w = w - alpha m / (sqrt(v) + eps), float32 in that order.  w, m, v, g: contiguous float32 tensors of one size on one device (g is
    only read); alpha: ``adam_alpha(lr, t)``.  One launch."""
    _require_cuda_f32(w, 'w')
    for t, name in ((m, 'm'), (v, 'v'), (g, 'g')):
        _require_cuda_f32(t, name)
        if t.numel() != w.numel() or t.device != w.device:
            raise ValueError('adam_step: %s has %d elements on %s, w %d on %s' % (name, t.numel(), t.device, w.numel(), w.device))
    if w.numel() == 0:
        raise ValueError('adam_step: no elements')
    with torch.cuda.device(w.device):
        check(lib().yr_adam_step(_ptr(w), _ptr(m), _ptr(v), _ptr(g), w.numel(), float(alpha), float(beta1), float(beta2), float(eps),
                                 stream_ptr(w.device)))
    return w


# ----------------------------------------------------------------------------- backward operators (csrc/convgrad.hip)
def linear_dgrad(dy, wt, cin, out=None):
    """The input gradient of ``linear_forward`` (yr_linear_dgrad): dy [..., cout] float32, wt [cout, round_up(cin, 4)] ->
    dx [..., cin] = dy @ wt[:, :cin] on the float32 matrix pipe.  ``cin`` names the channels taken of wt's rows.  out: a contiguous
    float32 tensor of that shape on dy's device (every element is written); default: a fresh one.  One launch."""
    return _linear_dgrad('linear_dgrad', 256, 'yr_linear_dgrad', dy, wt, cin, out)


# ----------------------------------------------------------------------------- 1x1 operators of any width up to 1024 (csrc/linearwide.hip)
LINEAR_WIDE_MAX = 1024


def linear_wide_forward(x, wt, out=None):
    """``linear_forward`` for 1..1024 channels on either side (yr_linear_wide_forward): x [..., cin] float32, wt [cout, round_up(cin, 4)]
    -> y [..., cout] = x @ wt[:, :cin].T on the float32 matrix pipe, the activations read once per 256 output channels.  out: a
    contiguous float32 tensor of that shape on x's device (every element is written); default: a fresh one.  One launch."""
    return _linear_forward('linear_wide_forward', LINEAR_WIDE_MAX, 'yr_linear_wide_forward', x, wt, out)


def linear_wide_dgrad(dy, wt, cin, out=None):
    """``linear_dgrad`` for 1..1024 channels on either side (yr_linear_wide_dgrad): dy [..., cout] float32, wt [cout, round_up(cin, 4)]
    -> dx [..., cin] = dy @ wt[:, :cin].  out: a contiguous float32 tensor of that shape on dy's device (every element is written);
    default: a fresh one.  One launch."""
    return _linear_dgrad('linear_wide_dgrad', LINEAR_WIDE_MAX, 'yr_linear_wide_dgrad', dy, wt, cin, out)


def linear_wide_wgrad_chunk(pixels, cin, cout):
    """Pixels per workgroup of the wide gradient's first stage: the least multiple of 16 that is at least 64, cout * round_up(cin, 4) /
    (cin + cout) and pixels / 1024; where cin and cout are both at most 256 ``linear_wgrad_chunk``'s value (the call is then
    ``linear_wgrad`` itself) - a function of these three numbers only (0: sizes the call refuses)."""
    return int(lib().yr_linear_wide_wgrad_chunk(int(pixels), int(cin), int(cout)))


def linear_wide_wgrad_workspace_bytes(pixels, cin, cout):
    return int(lib().yr_linear_wide_wgrad_workspace_bytes(int(pixels), int(cin), int(cout)))


def linear_wide_wgrad(x, dy, out=None, workspace=None):
    """``linear_wgrad`` for 1..1024 channels on either side (yr_linear_wide_wgrad): x [..., cin], dy [..., cout] float32 with the same
    leading axes -> dwt [cout, round_up(cin, 4)] = dy.T @ x, pad columns +0; no atomics, the same call gives the same bytes (those of
    ``linear_wgrad`` where cin and cout are both at most 256).  out: a
    contiguous float32 tensor of that shape on x's device (every element is written); workspace: a uint8 tensor of at least
    linear_wide_wgrad_workspace_bytes(pixels, cin, cout) bytes there (its contents do not matter).  Defaults: fresh ones.  Two
    launches."""
    return _linear_wgrad('linear_wide_wgrad', LINEAR_WIDE_MAX, 'yr_linear_wide_wgrad', x, dy, out, workspace)


def depthwise_geometry(h, w, k, stride=1, padding='same'):
    """-> (pad_top, pad_left, out_h, out_w) of a k x k depthwise convolution.  padding: 'same' (the Keras rule: out = ceil(n / stride),
    total pad max((out - 1) stride + k - n, 0), the smaller half in front) or (top, left, bottom, right), e.g. MobileNetV2's
    ZeroPadding2D(correct_pad) in front of its stride-2 'valid' convolutions."""
    h, w, k, stride = int(h), int(w), int(k), int(stride)
    if k not in (3, 5) or stride not in (1, 2) or h < 1 or w < 1:
        raise ValueError('depthwise: k in {3, 5}, stride in {1, 2} and a non-empty map, not k %d, stride %d, %d x %d' % (k, stride, h, w))
    if isinstance(padding, str):
        if padding != 'same':
            raise ValueError("depthwise: padding must be 'same' or (top, left, bottom, right), not %r" % (padding,))
        oh, ow = -(-h // stride), -(-w // stride)
        return max((oh - 1) * stride + k - h, 0) // 2, max((ow - 1) * stride + k - w, 0) // 2, oh, ow
    pt, pl, pb, pr = (int(v) for v in padding)
    if not all(0 <= v < k for v in (pt, pl, pb, pr)) or h + pt + pb < k or w + pl + pr < k:
        raise ValueError('depthwise: pads %r outside 0..k-1, or the padded map is smaller than the kernel' % (padding,))
    return pt, pl, (h + pt + pb - k) // stride + 1, (w + pl + pr - k) // stride + 1


def _dw_map(t, name):
    _require_cuda_f32(t, name)
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError('%s has shape %s, expected [B, H, W, C]' % (name, tuple(t.shape)))
    return tuple(t.shape)


def _dw_taps(w, c, name):
    _require_cuda_f32(w, name)
    if w.dim() != 2 or w.shape[0] not in (9, 25) or w.shape[1] != c:
        raise ValueError('%s has shape %s, expected [k * k, %d] with k in {3, 5}' % (name, tuple(w.shape), c))
    return 3 if w.shape[0] == 9 else 5


def depthwise_forward(x, w, stride=1, padding='same', out=None):
    """A k x k depthwise convolution on a plain map (yr_depthwise_forward): x [B, H, W, C] float32, w [k * k, C] (the Keras kernel
    [k, k, C, 1] reshaped) -> y [B, OH, OW, C]; stride and padding as ``depthwise_geometry`` reads them.  One launch."""
    b, h, wd, c = _dw_map(x, 'x')
    k = _dw_taps(w, c, 'w')
    if w.device != x.device:
        raise ValueError('depthwise_forward: w on %s, x on %s' % (w.device, x.device))
    pt, pl, oh, ow = depthwise_geometry(h, wd, k, stride, padding)
    out = _out_like(out, (b, oh, ow, c), x.device, 'depthwise_forward')
    with torch.cuda.device(x.device):
        check(lib().yr_depthwise_forward(_ptr(x), c, _ptr(w), b, h, wd, c, k, int(stride), pt, pl, oh, ow, _ptr(out), c, stream_ptr(x.device)))
    return out


def depthwise_dgrad(dy, w, input_hw, stride=1, padding='same', out=None):
    """The input gradient of ``depthwise_forward`` (yr_depthwise_dgrad): dy [B, OH, OW, C], w [k * k, C], input_hw = (H, W) of the
    forward's input -> dx [B, H, W, C], every element written once (a gather, taps in a fixed order).  One launch."""
    b, oh, ow, c = _dw_map(dy, 'dy')
    k = _dw_taps(w, c, 'w')
    if w.device != dy.device:
        raise ValueError('depthwise_dgrad: w on %s, dy on %s' % (w.device, dy.device))
    h, wd = int(input_hw[0]), int(input_hw[1])
    pt, pl, eh, ew = depthwise_geometry(h, wd, k, stride, padding)
    if (eh, ew) != (oh, ow):
        raise ValueError('depthwise_dgrad: dy is %d x %d, the forward of a %d x %d map gives %d x %d' % (oh, ow, h, wd, eh, ew))
    out = _out_like(out, (b, h, wd, c), dy.device, 'depthwise_dgrad')
    with torch.cuda.device(dy.device):
        check(lib().yr_depthwise_dgrad(_ptr(dy), c, _ptr(w), b, h, wd, c, k, int(stride), pt, pl, oh, ow, _ptr(out), c, stream_ptr(dy.device)))
    return out


def depthwise_wgrad_chunk(b, oh, ow, c, k):
    """Output rows (of the b * oh) per workgroup of the gradient's first stage: a function of these numbers only (0: refused sizes)."""
    return int(lib().yr_depthwise_wgrad_chunk(int(b), int(oh), int(ow), int(c), int(k)))


def depthwise_wgrad_workspace_bytes(b, oh, ow, c, k):
    return int(lib().yr_depthwise_wgrad_workspace_bytes(int(b), int(oh), int(ow), int(c), int(k)))


def depthwise_wgrad(x, dy, k, stride=1, padding='same', out=None, workspace=None):
    """The weight gradient of ``depthwise_forward`` (yr_depthwise_wgrad): x [B, H, W, C], dy [B, OH, OW, C] -> dw [k * k, C]; two
    stages, no atomics, the same call gives the same bytes.  workspace: a uint8 tensor of at least
    depthwise_wgrad_workspace_bytes(B, OH, OW, C, k) bytes (its contents do not matter); default: a fresh one.  Two launches."""
    b, h, wd, c = _dw_map(x, 'x')
    pt, pl, oh, ow = depthwise_geometry(h, wd, k, stride, padding)
    _require_cuda_f32(dy, 'dy')
    if tuple(dy.shape) != (b, oh, ow, c) or dy.device != x.device:
        raise ValueError('depthwise_wgrad: dy %s on %s, expected %s on %s' % (tuple(dy.shape), dy.device, (b, oh, ow, c), x.device))
    dev = x.device
    out = _out_like(out, (k * k, c), dev, 'depthwise_wgrad')
    ws = _workspace_arg(workspace, depthwise_wgrad_workspace_bytes(b, oh, ow, c, k), dev, 'depthwise_wgrad')
    with torch.cuda.device(dev):
        check(lib().yr_depthwise_wgrad(_ptr(x), c, _ptr(dy), c, b, h, wd, c, int(k), int(stride), pt, pl, oh, ow, _ptr(ws), ws.numel(), _ptr(out),
                                       stream_ptr(dev)))
    return out


# ----------------------------------------------------------------------------- the network entry as a training operator (csrc/stemgrad.hip)
def _conv3x3_w(w, name, cin=None):
    """w [9 * cin, cout] (the Keras kernel [3, 3, cin, cout] reshaped), cin in 1..4, cout in 1..64 -> (cin, cout)"""
    _require_cuda_f32(w, name)
    if w.dim() != 2 or w.shape[0] % 9 or not 1 <= w.shape[0] // 9 <= 4 or not 1 <= w.shape[1] <= 64 or (cin is not None and w.shape[0] != 9 * cin):
        raise ValueError('%s has shape %s, expected [9 * cin, cout] with cin in 1..4%s and cout in 1..64'
                         % (name, tuple(w.shape), '' if cin is None else ' (here %d)' % cin))
    return w.shape[0] // 9, w.shape[1]


def conv3x3_forward(x, w, stride=1, padding='same', out=None):
    """A dense 3 x 3 convolution on a plain map (yr_conv3x3_forward): x [B, H, W, cin] float32, w [9 * cin, cout] (the Keras kernel
    [3, 3, cin, cout] reshaped), cin in 1..4, cout in 1..64 -> y [B, OH, OW, cout]; stride and padding as ``depthwise_geometry`` reads
    them.  Every output is one chain of fmaf, taps row-major and channels innermost, padded taps skipped.  One launch."""
    b, h, wd, cin = _dw_map(x, 'x')
    _, cout = _conv3x3_w(w, 'w', cin)
    if w.device != x.device:
        raise ValueError('conv3x3_forward: w on %s, x on %s' % (w.device, x.device))
    pt, pl, oh, ow = depthwise_geometry(h, wd, 3, stride, padding)
    out = _out_like(out, (b, oh, ow, cout), x.device, 'conv3x3_forward')
    with torch.cuda.device(x.device):
        check(lib().yr_conv3x3_forward(_ptr(x), cin, _ptr(w), b, h, wd, cin, cout, int(stride), pt, pl, oh, ow, _ptr(out), cout, stream_ptr(x.device)))
    return out


def conv3x3_dgrad(dy, w, input_hw, stride=1, padding='same', out=None):
    """The input gradient of ``conv3x3_forward`` (yr_conv3x3_dgrad): dy [B, OH, OW, cout], w [9 * cin, cout], input_hw = (H, W) of the
    forward's input -> dx [B, H, W, cin], every element written once (+0 where no window reaches).  One launch."""
    b, oh, ow, cout = _dw_map(dy, 'dy')
    cin, wc = _conv3x3_w(w, 'w')
    if wc != cout or w.device != dy.device:
        raise ValueError('conv3x3_dgrad: w %s on %s for dy %s on %s' % (tuple(w.shape), w.device, tuple(dy.shape), dy.device))
    h, wd = int(input_hw[0]), int(input_hw[1])
    pt, pl, eh, ew = depthwise_geometry(h, wd, 3, stride, padding)
    if (eh, ew) != (oh, ow):
        raise ValueError('conv3x3_dgrad: dy is %d x %d, the forward of a %d x %d map gives %d x %d' % (oh, ow, h, wd, eh, ew))
    out = _out_like(out, (b, h, wd, cin), dy.device, 'conv3x3_dgrad')
    with torch.cuda.device(dy.device):
        check(lib().yr_conv3x3_dgrad(_ptr(dy), cout, _ptr(w), b, h, wd, cin, cout, int(stride), pt, pl, oh, ow, _ptr(out), cin, stream_ptr(dy.device)))
    return out


def conv3x3_wgrad_chunk(b, oh, ow, cin, cout):
    """Output rows (of the b * oh) per workgroup of the gradient's first stage: a function of these numbers only (0: refused sizes)."""
    return int(lib().yr_conv3x3_wgrad_chunk(int(b), int(oh), int(ow), int(cin), int(cout)))


def conv3x3_wgrad_workspace_bytes(b, oh, ow, cin, cout):
    return int(lib().yr_conv3x3_wgrad_workspace_bytes(int(b), int(oh), int(ow), int(cin), int(cout)))


def conv3x3_wgrad(x, dy, stride=1, padding='same', out=None, workspace=None):
    """The weight gradient of ``conv3x3_forward`` (yr_conv3x3_wgrad): x [B, H, W, cin], dy [B, OH, OW, cout] -> dw [9 * cin, cout]; two
    stages, no atomics, the same call gives the same bytes.  workspace: a uint8 tensor of at least
    conv3x3_wgrad_workspace_bytes(B, OH, OW, cin, cout) bytes (its contents do not matter); default: a fresh one.  Two launches."""
    b, h, wd, cin = _dw_map(x, 'x')
    pt, pl, oh, ow = depthwise_geometry(h, wd, 3, stride, padding)
    _require_cuda_f32(dy, 'dy')
    if dy.dim() != 4 or tuple(dy.shape[:3]) != (b, oh, ow) or dy.device != x.device or not 1 <= cin <= 4 or not 1 <= dy.shape[3] <= 64:
        raise ValueError('conv3x3_wgrad: x %s and dy %s on %s, expected x [B, H, W, 1..4] and dy %s + (1..64,) on %s'
                         % (tuple(x.shape), tuple(dy.shape), dy.device, (b, oh, ow), x.device))
    cout, dev = dy.shape[3], x.device
    out = _out_like(out, (9 * cin, cout), dev, 'conv3x3_wgrad')
    ws = _workspace_arg(workspace, conv3x3_wgrad_workspace_bytes(b, oh, ow, cin, cout), dev, 'conv3x3_wgrad')
    with torch.cuda.device(dev):
        check(lib().yr_conv3x3_wgrad(_ptr(x), cin, _ptr(dy), cout, b, h, wd, cin, cout, int(stride), pt, pl, oh, ow, _ptr(ws), ws.numel(), _ptr(out),
                                     stream_ptr(dev)))
    return out


BN_ACTS = {None: 0, 'none': 0, 'linear': 0, 'relu6': 1, 'swish': 2}      # YR_ACT_NONE, YR_ACT_RELU6, YR_ACT_SWISH


def _bn_act_id(act):
    key = act.lower() if isinstance(act, str) else act
    if key not in BN_ACTS:
        raise ValueError("bn_act: act must be None / 'none', 'relu6' or 'swish', not %r" % (act,))
    return BN_ACTS[key]


def _bn_vec(t, c, dev, name):
    _require_cuda_f32(t, name)
    if tuple(t.shape) != (c,) or t.device != dev:
        raise ValueError('%s has shape %s on %s, expected (%d,) on %s' % (name, tuple(t.shape), t.device, c, dev))


def bn_act_forward(z, scale, shift, act, out=None, keep_u=False):
    """Frozen BatchNorm + activation (yr_bn_act_forward): z [..., C] float32, scale / shift [C] -> a = act(z * scale + shift), act in
    {None, 'relu6', 'swish'}.  keep_u: also return u = z * scale + shift (what ``bn_act_backward`` needs) -> (a, u).  One launch."""
    pixels, c = _rows(z, 'z')
    _bn_vec(scale, c, z.device, 'scale')
    _bn_vec(shift, c, z.device, 'shift')
    out = _out_like(out, tuple(z.shape), z.device, 'bn_act_forward')
    u = torch.empty_like(z) if keep_u else None
    with torch.cuda.device(z.device):
        check(lib().yr_bn_act_forward(_ptr(z), c, _ptr(scale), _ptr(shift), pixels, c, _bn_act_id(act), _ptr(out), c, _ptr(u), c, stream_ptr(z.device)))
    return (out, u) if keep_u else out


def bn_act_backward(da, u, scale, act, out=None):
    """dz = da * act'(u) * scale (yr_bn_act_backward): da [..., C], u as ``bn_act_forward(keep_u=True)`` returned it (None for act
    None, whose derivative does not read it), scale [C].  ReLU6' is 1 on 0 < u < 6 (both strict).  One launch."""
    pixels, c = _rows(da, 'da')
    a = _bn_act_id(act)
    _bn_vec(scale, c, da.device, 'scale')
    if u is None:
        if a != 0:
            raise ValueError('bn_act_backward: u is needed for %r' % (act,))
    else:
        _require_cuda_f32(u, 'u')
        if tuple(u.shape) != tuple(da.shape) or u.device != da.device:
            raise ValueError('bn_act_backward: u %s on %s for da %s on %s' % (tuple(u.shape), u.device, tuple(da.shape), da.device))
    out = _out_like(out, tuple(da.shape), da.device, 'bn_act_backward')
    with torch.cuda.device(da.device):
        check(lib().yr_bn_act_backward(_ptr(da), c, _ptr(u), c, _ptr(scale), pixels, c, a, _ptr(out), c, stream_ptr(da.device)))
    return out


# ----------------------------------------------------------------------------- BatchNorm in training mode (csrc/bntrain.hip)
def bn_train_chunk(pixels, c):
    """Pixels per workgroup of the first stage of every per-channel sum: a function of these numbers only (0: refused sizes)."""
    return int(lib().yr_bn_train_chunk(int(pixels), int(c)))


def bn_train_workspace_bytes(pixels, c):
    """Bytes of workspace that ``bn_train_forward`` and ``bn_train_backward`` need (the same for both; 0: refused sizes)."""
    return int(lib().yr_bn_train_workspace_bytes(int(pixels), int(c)))


def _bn_train_workspace(workspace, pixels, c, dev, name):
    need = bn_train_workspace_bytes(pixels, c)
    if need == 0:
        raise ValueError('%s: %d pixels of %d channels are outside the contract' % (name, pixels, c))
    return _workspace_arg(workspace, need, dev, name)


def bn_train_forward(z, gamma, beta, eps=1e-3, momentum=0.9, act=None, moving_mean=None, moving_var=None, out=None, workspace=None):
    """BatchNorm on the statistics of the batch + activation (yr_bn_train_forward): z [..., C] float32, gamma / beta [C] ->
    (a, mean, invstd) with a = act((z - mean) * invstd * gamma + beta), mean and the biased variance taken over all leading axes,
    invstd = 1 / sqrt(var + eps); act in {None, 'relu6', 'swish'}.  moving_mean / moving_var [C] (both or neither) are updated in place:
    moving -= (moving - batch value) * (1 - momentum), the variance the unbiased one, as Keras stores it.  workspace: a uint8 tensor of
    at least bn_train_workspace_bytes(pixels, C) bytes (its contents do not matter); default: a fresh one.  Three launches."""
    pixels, c = _rows(z, 'z')
    dev = z.device
    _bn_vec(gamma, c, dev, 'gamma')
    _bn_vec(beta, c, dev, 'beta')
    if (moving_mean is None) != (moving_var is None):
        raise ValueError('bn_train_forward: moving_mean and moving_var go together')
    if moving_mean is not None:
        _bn_vec(moving_mean, c, dev, 'moving_mean')
        _bn_vec(moving_var, c, dev, 'moving_var')
    eps, momentum = float(eps), float(momentum)
    if not (0.0 <= eps < float('inf')) or not 0.0 <= momentum <= 1.0:
        raise ValueError('bn_train_forward: eps must be finite and >= 0 and momentum in [0, 1], not %r and %r' % (eps, momentum))
    a = _bn_act_id(act)
    out = _out_like(out, tuple(z.shape), dev, 'bn_train_forward')
    ws = _bn_train_workspace(workspace, pixels, c, dev, 'bn_train_forward')
    mean = torch.empty((c,), dtype=torch.float32, device=dev)
    invstd = torch.empty((c,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_bn_train_forward(_ptr(z), c, _ptr(gamma), _ptr(beta), pixels, c, eps, momentum, a, _ptr(out), c, _ptr(mean), _ptr(invstd),
                                        _ptr(moving_mean), _ptr(moving_var), _ptr(ws), ws.numel(), stream_ptr(dev)))
    return out, mean, invstd


def bn_train_backward(da, z, gamma, beta, mean, invstd, act, need_dz=True, out=None, workspace=None):
    """The gradients of ``bn_train_forward`` (yr_bn_train_backward): da, z [..., C], gamma / beta / mean / invstd [C] (the last two as the
    forward returned them) -> (dz or None, dgamma, dbeta).  need_dz=False skips the elementwise pass; dgamma and dbeta are the same bits.
    Two launches."""
    pixels, c = _rows(da, 'da')
    dev = da.device
    _require_cuda_f32(z, 'z')
    if tuple(z.shape) != tuple(da.shape) or z.device != dev:
        raise ValueError('bn_train_backward: z %s on %s for da %s on %s' % (tuple(z.shape), z.device, tuple(da.shape), dev))
    for t, name in ((gamma, 'gamma'), (beta, 'beta'), (mean, 'mean'), (invstd, 'invstd')):
        _bn_vec(t, c, dev, name)
    a = _bn_act_id(act)
    if need_dz:
        out = _out_like(out, tuple(da.shape), dev, 'bn_train_backward')
    elif out is not None:
        raise ValueError('bn_train_backward: out given with need_dz=False')
    ws = _bn_train_workspace(workspace, pixels, c, dev, 'bn_train_backward')
    dgamma = torch.empty((c,), dtype=torch.float32, device=dev)
    dbeta = torch.empty((c,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_bn_train_backward(_ptr(da), c, _ptr(z), c, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), pixels, c, a, _ptr(out), c,
                                         _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel(), stream_ptr(dev)))
    return out, dgamma, dbeta


# ----------------------------------------------------------------------------- the fusing operators (csrc/fusegrad.hip)
def _pool_k(k, h, w, name):
    k = int(k)
    if k not in (2, 4) or h < k or w < k:
        raise ValueError('%s: k in {2, 4} and a map of at least k x k, not k %d on %d x %d' % (name, k, h, w))
    return k


def maxpool_forward(x, k, out=None):
    """Keras MaxPooling2D((k, k)) (yr_maxpool_forward): x [B, H, W, C] float32, k in {2, 4} -> y [B, H // k, W // k, C]; rows and columns
    past the last whole window are not read.  One launch."""
    b, h, w, c = _dw_map(x, 'x')
    k = _pool_k(k, h, w, 'maxpool_forward')
    out = _out_like(out, (b, h // k, w // k, c), x.device, 'maxpool_forward')
    with torch.cuda.device(x.device):
        check(lib().yr_maxpool_forward(_ptr(x), c, b, h, w, c, k, _ptr(out), c, stream_ptr(x.device)))
    return out


def maxpool_backward(dy, x, k, out=None):
    """The input gradient of ``maxpool_forward`` (yr_maxpool_backward): dy [B, H // k, W // k, C], x the forward's input -> dx of x's
    shape: dy at the first maximum of each window (row-major scan, strict comparison), +0 everywhere else, the trailing strip included;
    every element written once.  One launch."""
    b, h, w, c = _dw_map(x, 'x')
    k = _pool_k(k, h, w, 'maxpool_backward')
    _require_cuda_f32(dy, 'dy')
    if tuple(dy.shape) != (b, h // k, w // k, c) or dy.device != x.device:
        raise ValueError('maxpool_backward: dy %s on %s, expected %s on %s' % (tuple(dy.shape), dy.device, (b, h // k, w // k, c), x.device))
    out = _out_like(out, (b, h, w, c), x.device, 'maxpool_backward')
    with torch.cuda.device(x.device):
        check(lib().yr_maxpool_backward(_ptr(dy), c, _ptr(x), c, b, h, w, c, k, _ptr(out), c, stream_ptr(x.device)))
    return out


def upsample2_forward(x, out=None):
    """Keras UpSampling2D() (yr_upsample2_forward): x [B, H, W, C] float32 -> y [B, 2H, 2W, C], nearest neighbour.  One launch."""
    b, h, w, c = _dw_map(x, 'x')
    out = _out_like(out, (b, 2 * h, 2 * w, c), x.device, 'upsample2_forward')
    with torch.cuda.device(x.device):
        check(lib().yr_upsample2_forward(_ptr(x), c, b, h, w, c, _ptr(out), c, stream_ptr(x.device)))
    return out


def upsample2_backward(dy, out=None):
    """The input gradient of ``upsample2_forward`` (yr_upsample2_backward): dy [B, 2H, 2W, C] -> dx [B, H, W, C], the four elements of
    each 2 x 2 block added in row-major order.  One launch."""
    b, h2, w2, c = _dw_map(dy, 'dy')
    if h2 % 2 or w2 % 2:
        raise ValueError('upsample2_backward: dy is %d x %d, expected even sides' % (h2, w2))
    out = _out_like(out, (b, h2 // 2, w2 // 2, c), dy.device, 'upsample2_backward')
    with torch.cuda.device(dy.device):
        check(lib().yr_upsample2_backward(_ptr(dy), c, b, h2 // 2, w2 // 2, c, _ptr(out), c, stream_ptr(dy.device)))
    return out


def wsum_chunk(pixels, c):
    """Pixels per workgroup of the first stage of ``wsum_backward``'s sums: a function of these numbers only (0: refused sizes)."""
    return int(lib().yr_wsum_chunk(int(pixels), int(c)))


def wsum_workspace_bytes(pixels, c):
    """Bytes of workspace that ``wsum_backward`` needs for d alpha (0: refused sizes)."""
    return int(lib().yr_wsum_workspace_bytes(int(pixels), int(c)))


def _wsum_args(name, first, what, xs, alpha):
    """-> (pixels, c, device) of ``first`` [..., C], called ``what`` in messages; xs: four tensors of its shape there (or None: not
    checked), alpha float32 [4] there"""
    pixels, c = _rows(first, what)
    dev = first.device
    if xs is not None:
        if not isinstance(xs, (list, tuple)) or len(xs) != 4:
            raise ValueError('%s: exactly four maps' % name)
        for i, x in enumerate(xs):
            _require_cuda_f32(x, 'xs[%d]' % i)
            if tuple(x.shape) != tuple(first.shape) or x.device != dev:
                raise ValueError('%s: xs[%d] %s on %s, expected %s on %s' % (name, i, tuple(x.shape), x.device, tuple(first.shape), dev))
    _bn_vec(alpha, 4, dev, 'alpha')
    return pixels, c, dev


def wsum_forward(xs, alpha, out=None):
    """The reference's WeightedSum of four maps (yr_wsum_forward): xs four float32 tensors [..., C] of one shape, alpha float32 [4] on
    their device -> y = ((alpha[0] xs[0] + alpha[1] xs[1]) + alpha[2] xs[2]) + alpha[3] xs[3], the float32 bits of YR_OP_WSUM.  One launch."""
    if not isinstance(xs, (list, tuple)) or len(xs) != 4:
        raise ValueError('wsum_forward: exactly four maps')
    pixels, c, dev = _wsum_args('wsum_forward', xs[0], 'xs[0]', xs, alpha)
    out = _out_like(out, tuple(xs[0].shape), dev, 'wsum_forward')
    with torch.cuda.device(dev):
        check(lib().yr_wsum_forward(_ptr(xs[0]), c, _ptr(xs[1]), c, _ptr(xs[2]), c, _ptr(xs[3]), c, _ptr(alpha), pixels, c, _ptr(out), c, stream_ptr(dev)))
    return out


def wsum_backward(dy, xs, alpha, need=(True, True, True, True), need_alpha=True, out=None, workspace=None):
    """The gradients of ``wsum_forward`` (yr_wsum_backward): dy [..., C]; xs the forward's four maps (None is allowed with
    need_alpha=False: they are not read then); alpha [4] -> (dxs, dalpha): dxs[i] = alpha[i] * dy for the i with need[i], None for the
    others; dalpha[i] = sum(dy * xs[i]) in a fixed order (no atomics: the same call gives the same bytes), None with need_alpha=False.
    out: a sequence of four tensors or Nones to receive the dxs; workspace: a uint8 tensor of at least wsum_workspace_bytes(pixels, C)
    bytes (its contents do not matter).  Defaults: fresh ones.  Two launches with need_alpha, one without, none when nothing is needed."""
    need = tuple(bool(v) for v in need)
    if len(need) != 4:
        raise ValueError('wsum_backward: need has four flags')
    if xs is None and need_alpha:
        raise ValueError('wsum_backward: d alpha needs the four maps')
    pixels, c, dev = _wsum_args('wsum_backward', dy, 'dy', xs if need_alpha else None, alpha)
    if out is None:
        out = (None,) * 4
    if len(out) != 4 or any(o is not None and not n for o, n in zip(out, need)):
        raise ValueError('wsum_backward: out is a sequence of four, None where need is False')
    dxs = [_out_like(o, tuple(dy.shape), dev, 'wsum_backward') if n else None for o, n in zip(out, need)]
    dalpha = ws = None
    if need_alpha:
        nbytes = wsum_workspace_bytes(pixels, c)
        if nbytes == 0:
            raise ValueError('wsum_backward: %d pixels of %d channels are outside the contract' % (pixels, c))
        ws = _workspace_arg(workspace, nbytes, dev, 'wsum_backward')
        dalpha = torch.empty((4,), dtype=torch.float32, device=dev)
    xp = [_ptr(x) for x in xs] if need_alpha else [None] * 4
    with torch.cuda.device(dev):
        check(lib().yr_wsum_backward(_ptr(dy), c, xp[0], c, xp[1], c, xp[2], c, xp[3], c, _ptr(alpha), pixels, c,
                                     _ptr(dxs[0]), c, _ptr(dxs[1]), c, _ptr(dxs[2]), c, _ptr(dxs[3]), c, _ptr(dalpha),
                                     _ptr(ws), ws.numel() if ws is not None else 0, stream_ptr(dev)))
    return dxs, dalpha


# ----------------------------------------------------------------------------- the squeeze-excite block (csrc/segrad.hip)
def se_chunk(b, n, c):
    """Pixels of one image per workgroup of the first stage of ``se_forward``'s and ``se_backward``'s sums over the map: a function of
    n = H * W and c only (b is checked: b * n < 2^40); 0: refused sizes."""
    return int(lib().yr_se_chunk(int(b), int(n), int(c)))


def se_workspace_bytes(b, n, c, r):
    """Bytes of workspace that ``se_forward`` and ``se_backward`` need (the same for both; 0: refused sizes)."""
    return int(lib().yr_se_workspace_bytes(int(b), int(n), int(c), int(r)))


def _se_args(name, x, w1, w2):
    """-> (b, h, w, c, r, device) of the map x [B, H, W, C] and the kernels w1 [C, R], w2 [R, C] there"""
    b, h, w, c = _dw_map(x, 'x')
    dev = x.device
    for t, what in ((w1, 'w1'), (w2, 'w2')):
        _require_cuda_f32(t, what)
    if w1.dim() != 2 or w1.shape[0] != c or tuple(w2.shape) != (w1.shape[1], c) or w1.device != dev or w2.device != dev:
        raise ValueError('%s: w1 %s and w2 %s, expected (%d, R) and (R, %d) on %s' % (name, tuple(w1.shape), tuple(w2.shape), c, c, dev))
    return b, h, w, c, int(w1.shape[1]), dev


def _se_workspace(workspace, b, n, c, r, dev, name):
    need = se_workspace_bytes(b, n, c, r)
    if need == 0:
        raise ValueError('%s: %d images of %d pixels, C = %d, R = %d are outside the contract' % (name, b, n, c, r))
    return _workspace_arg(workspace, need, dev, name)


def _se_mat(t, shape, dev, name):
    _require_cuda_f32(t, name)
    if tuple(t.shape) != tuple(shape) or t.device != dev:
        raise ValueError('%s has shape %s on %s, expected %s on %s' % (name, tuple(t.shape), t.device, tuple(shape), dev))


def se_forward(x, w1, b1, w2, b2, out=None, workspace=None):
    """The squeeze-excite block (yr_se_forward): x [B, H, W, C] float32, w1 [C, R] and b1 [R] (the Keras <name>_se_reduce kernel
    [1, 1, C, R] reshaped, and its bias), w2 [R, C] and b2 [C] (<name>_se_expand) -> (y, m, z1, g): m [B, C] the mean over the map,
    z1 [B, R] = b1 + m w1, g [B, C] = sigmoid(b2 + swish(z1) w2), y = x * g; m, z1 and g are what ``se_backward`` needs.  workspace: a
    uint8 tensor of at least se_workspace_bytes(B, H * W, C, R) bytes (its contents do not matter); default: a fresh one.  Three launches."""
    b, h, w, c, r, dev = _se_args('se_forward', x, w1, w2)
    _bn_vec(b1, r, dev, 'b1')
    _bn_vec(b2, c, dev, 'b2')
    out = _out_like(out, (b, h, w, c), dev, 'se_forward')
    ws = _se_workspace(workspace, b, h * w, c, r, dev, 'se_forward')
    m = torch.empty((b, c), dtype=torch.float32, device=dev)
    z1 = torch.empty((b, r), dtype=torch.float32, device=dev)
    g = torch.empty((b, c), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_se_forward(_ptr(x), c, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), b, h, w, c, r, _ptr(out), c, _ptr(m), _ptr(z1), _ptr(g),
                                  _ptr(ws), ws.numel(), stream_ptr(dev)))
    return out, m, z1, g


def se_backward(dy, x, w1, w2, m, z1, g, need_dx=True, need_params=True, out=None, workspace=None):
    """The gradients of ``se_forward`` (yr_se_backward): dy and x [B, H, W, C], w1 [C, R], w2 [R, C], and m, z1, g as the forward
    returned them -> (dx, dw1, db1, dw2, db2): dx of x's shape (None with need_dx=False: its pass over the map is not launched), the
    four parameter gradients in the parameters' shapes, summed over the batch in image order (all None with need_params=False: the
    batch sums are not computed).  The other outputs keep their bits either way; no atomics: the same call gives the same bytes.
    out: a tensor to receive dx; workspace: as ``se_forward``'s.  Four launches, three with need_dx or need_params alone, none with
    neither."""
    b, h, w, c, r, dev = _se_args('se_backward', x, w1, w2)
    _se_mat(dy, (b, h, w, c), dev, 'dy')
    _se_mat(m, (b, c), dev, 'm')
    _se_mat(z1, (b, r), dev, 'z1')
    _se_mat(g, (b, c), dev, 'g')
    if need_dx:
        out = _out_like(out, (b, h, w, c), dev, 'se_backward')
    elif out is not None:
        raise ValueError('se_backward: out given with need_dx=False')
    ws = _se_workspace(workspace, b, h * w, c, r, dev, 'se_backward')
    dw1 = db1 = dw2 = db2 = None
    if need_params:
        dw1, db1 = torch.empty((c, r), dtype=torch.float32, device=dev), torch.empty((r,), dtype=torch.float32, device=dev)
        dw2, db2 = torch.empty((r, c), dtype=torch.float32, device=dev), torch.empty((c,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_se_backward(_ptr(dy), c, _ptr(x), c, _ptr(w1), _ptr(w2), _ptr(m), _ptr(z1), _ptr(g), b, h, w, c, r, _ptr(out), c,
                                   _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(ws), ws.numel(), stream_ptr(dev)))
    return out, dw1, db1, dw2, db2


VOC_MAX_ROWS, VOC_MAX_GT = 4096, 512    # YR_VOC_MAX_ROWS, YR_VOC_MAX_GT of include/yoloret_hip.h


def _is_cuda_i32(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()


def voc_match(det, det_count, gt, gt_count, num_classes, iou=.5):
    """VOC matching of packed detections to ground truth, per image (the greedy loop of reference map.py:157-215 on the device).
    det [B,rows,6] int32, det_count [B] int32: what pack_detections returns; gt [B,G,5] float32 rows (xmin, ymin, xmax, ymax,
    label) of which the first gt_count[b] [B] int32 are valid (G may be 0) -> flags [B,rows] int32 (1 true positive, 0 false
    positive, -1 no verdict: beyond det_count or class outside [0, num_classes)), npos [B,num_classes] int32.  Launches only."""
    shapes = 'det %s, det_count %s, gt %s, gt_count %s' % tuple(tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
                                                                for t in (det, det_count, gt, gt_count))
    if not (_is_cuda_i32(det) and _is_cuda_i32(det_count) and _is_cuda_i32(gt_count)):
        raise ValueError('voc_match: det, det_count and gt_count must be contiguous int32 CUDA tensors (%s)' % shapes)
    if not (isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype == torch.float32 and gt.is_contiguous()):
        raise ValueError('voc_match: gt must be a contiguous float32 CUDA tensor (%s)' % shapes)
    if det.dim() != 3 or det.shape[2] != 6 or det.shape[0] < 1 or not 1 <= det.shape[1] <= VOC_MAX_ROWS:
        raise ValueError('voc_match: det must be [B,rows,6] with B >= 1 and 1 <= rows <= %d (%s)' % (VOC_MAX_ROWS, shapes))
    b, rows = det.shape[0], det.shape[1]
    if gt.dim() != 3 or gt.shape[0] != b or gt.shape[2] != 5 or gt.shape[1] > VOC_MAX_GT:
        raise ValueError('voc_match: gt must be [B=%d,G,5] with G <= %d (%s)' % (b, VOC_MAX_GT, shapes))
    if tuple(det_count.shape) != (b,) or tuple(gt_count.shape) != (b,):
        raise ValueError('voc_match: det_count and gt_count must be [B=%d] (%s)' % (b, shapes))
    if int(num_classes) < 1:
        raise ValueError('voc_match: num_classes must be at least 1, not %d' % num_classes)
    dev = det.device
    if not (det_count.device == dev and gt.device == dev and gt_count.device == dev):
        raise ValueError('voc_match: det on %s, det_count on %s, gt on %s, gt_count on %s: one device expected (%s)'
                         % (dev, det_count.device, gt.device, gt_count.device, shapes))
    flags = torch.empty((b, rows), dtype=torch.int32, device=dev)
    npos = torch.empty((b, int(num_classes)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().yr_voc_match(_ptr(det), _ptr(det_count), b, rows, int(num_classes), _ptr(gt) if gt.shape[1] else None,
                                 _ptr(gt_count), gt.shape[1], float(iou), _ptr(flags), _ptr(npos), stream_ptr(dev)))
    return flags, npos


ENC_MAX_BOXES = 256     # YR_ENC_MAX_BOXES of include/yoloret_hip.h
_GRID_STEPS = (32, 16, 8)


def label_shapes(batch, input_hw, num_classes, num_scales):
    """The shapes [B,gh,gw,3,5+C] of the y_true tensors of `num_scales` scales (utils.py:327-336)."""
    return [(int(batch), int(input_hw[0]) // _GRID_STEPS[l], int(input_hw[1]) // _GRID_STEPS[l], 3, 5 + int(num_classes))
            for l in range(num_scales)]


def label_args(true_boxes, input_hw, anchors, num_classes, num_scales):
    """The argument checks of encode_labels that need no device (ValueError) -> (B, T, in_h, in_w, float32 anchors [9,2], shapes)."""
    if not isinstance(true_boxes, torch.Tensor) or true_boxes.dtype != torch.float32:
        raise ValueError('encode_labels: true_boxes must be a float32 tensor, not %s'
                         % (true_boxes.dtype if isinstance(true_boxes, torch.Tensor) else type(true_boxes).__name__))
    if true_boxes.dim() != 3 or true_boxes.shape[2] != 5 or true_boxes.shape[0] < 1:
        raise ValueError('encode_labels: true_boxes has shape %s, expected [B,T,5] with B >= 1' % (tuple(true_boxes.shape),))
    b, t = int(true_boxes.shape[0]), int(true_boxes.shape[1])
    if not 1 <= t <= ENC_MAX_BOXES:
        raise ValueError('encode_labels: T = %d rows per image, 1..%d expected' % (t, ENC_MAX_BOXES))
    if num_scales not in (1, 2, 3):
        raise ValueError('encode_labels: num_scales must be 1, 2 or 3, not %r' % (num_scales,))
    in_h, in_w = int(input_hw[0]), int(input_hw[1])
    if in_h <= 0 or in_w <= 0 or in_h % 32 or in_w % 32:
        raise ValueError('encode_labels: input shape %dx%d, positive multiples of 32 expected' % (in_h, in_w))
    if int(num_classes) < 0:
        raise ValueError('encode_labels: num_classes must not be negative (%d)' % num_classes)
    anchors = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(-1, 2))
    if anchors.shape[0] != 9:
        raise ValueError('encode_labels: %d anchors, all 9 expected' % anchors.shape[0])
    shapes = label_shapes(b, (in_h, in_w), num_classes, num_scales)
    for shp in shapes:
        if int(np.prod(shp, dtype=np.int64)) > 1 << 31:
            raise ValueError('encode_labels: a label tensor %s has more than 2^31 elements' % (shp,))
    return b, t, in_h, in_w, anchors, shapes


def encode_labels(true_boxes, input_hw, anchors, num_classes, num_scales, out=None, skipped=None):
    """preprocess_true_boxes (utils.py:298-376) for a whole batch on the device.  true_boxes: float32 CUDA tensor [B,T,5] of rows
    (x_min, y_min, x_max, y_max, class) in pixels of the network input, zero rows last, T <= 256; anchors: all 9 (w,h) anchors
    -> the tuple of `num_scales` float32 tensors [B,gh,gw,3,5+C] on that device, byte for byte what the host function returns
    image by image (contract and quirks: include/yoloret_hip.h).  They are fresh tensors unless `out` (a sequence of num_scales
    contiguous float32 tensors of those shapes) is given; every element is written, nothing needs zeroing.  `skipped`: an int32
    [B] tensor that receives the number of rows per image that could not be written: rows with a non-finite value (removed from
    the list before anything else) plus rows whose class or cell is out of range (they keep their place in the list, only their
    write is dropped).  Launches only, on the current stream of that device."""
    b, t, in_h, in_w, anchors, shapes = label_args(true_boxes, input_hw, anchors, num_classes, num_scales)
    if not (true_boxes.is_cuda and true_boxes.is_contiguous()):
        raise ValueError('encode_labels: true_boxes must be a contiguous CUDA tensor (it is on %s)' % true_boxes.device)
    dev = true_boxes.device
    if out is None:
        out = [torch.empty(shp, dtype=torch.float32, device=dev) for shp in shapes]
    else:
        out = list(out)
        if len(out) != num_scales:
            raise ValueError('encode_labels: %d out tensors for %d scales' % (len(out), num_scales))
        for o, shp in zip(out, shapes):
            if not (isinstance(o, torch.Tensor) and o.dtype == torch.float32 and o.is_contiguous() and o.device == dev and tuple(o.shape) == shp):
                raise ValueError('encode_labels: out tensors must be contiguous float32 %s on %s' % (shapes, dev))
    if skipped is not None and not (_is_cuda_i32(skipped) and skipped.device == dev and tuple(skipped.shape) == (b,)):
        raise ValueError('encode_labels: skipped must be a contiguous int32 [B=%d] tensor on %s' % (b, dev))
    yp = [_ptr(out[l]) if l < num_scales else None for l in range(3)]
    with torch.cuda.device(dev):
        check(lib().yr_encode_labels(_ptr(true_boxes), b, t, in_h, in_w, anchors.ctypes.data_as(ctypes.c_void_p), int(num_classes),
                                     int(num_scales), yp[0], yp[1], yp[2], _ptr(skipped), stream_ptr(dev)))
    return tuple(out)


def correct_boxes(box_xy, box_wh, input_hw, image_hw):
    _require_cuda_f32(box_xy, 'box_xy')
    _require_cuda_f32(box_wh, 'box_wh')
    b = box_xy.shape[0]
    n = box_xy[0].numel() // 2
    boxes = torch.empty(tuple(box_xy.shape[:-1]) + (4,), dtype=torch.float32, device=box_xy.device)
    if box_wh.shape != box_xy.shape or box_wh.device != box_xy.device:
        raise ValueError('correct_boxes: box_xy %s and box_wh %s differ' % (tuple(box_xy.shape), tuple(box_wh.shape)))
    with torch.cuda.device(box_xy.device):
        check(lib().yr_correct_boxes(_ptr(box_xy), _ptr(box_wh), b, n, int(input_hw[0]), int(input_hw[1]),
                                     _ptr(image_hw), _ptr(boxes), stream_ptr(box_xy.device)))
    return boxes


def letterbox(image_u8, input_hw, out=None):
    """image_u8: uint8 CUDA tensor [ih,iw,3] -> float32 [H,W,3] letterboxed network input; a batch of equally sized
    images [B,ih,iw,3] -> [B,H,W,3] in one launch."""
    if not (isinstance(image_u8, torch.Tensor) and image_u8.is_cuda and image_u8.dtype == torch.uint8
            and image_u8.dim() in (3, 4) and image_u8.shape[-1] == 3 and image_u8.is_contiguous()):
        raise ValueError('image must be a contiguous uint8 CUDA tensor [h,w,3] or [B,h,w,3]')
    h, w = int(input_hw[0]), int(input_hw[1])
    batched = image_u8.dim() == 4
    out = _out_like(out, ((image_u8.shape[0],) if batched else ()) + (h, w, 3), image_u8.device, 'letterbox')
    with torch.cuda.device(image_u8.device):
        check(lib().yr_letterbox_batch(_ptr(image_u8), image_u8.shape[0] if batched else 1, image_u8.shape[-3],
                                       image_u8.shape[-2], _ptr(out), h, w, stream_ptr(image_u8.device)))
    return out


# ----------------------------------------------------------------------------- ragged batched ingest
INGEST_LETTERBOX, INGEST_VALIDATE, INGEST_MAX_BOXES = 0, 1, 256     # YR_INGEST_* of include/yoloret_hip.h


class _RaggedTable:
    """The table of one ragged batch: ``host`` is the structured array [B] (DTYPE), ``packed_bytes`` the size of the packed source,
    ``device`` the uint8 tensor [B * DTYPE.itemsize] that holds its bytes on the GPU once it has been uploaded."""

    def __init__(self, host, input_hw, packed_bytes):
        self.host, self.input_hw, self.packed_bytes = host, (int(input_hw[0]), int(input_hw[1])), int(packed_bytes)
        self.batch = int(host.shape[0])
        self.device = None

    def upload(self, device):
        """The table alone, in a copy of its own (tests and tools; a pipeline uploads it with the images: RaggedStager)."""
        self.device = torch.from_numpy(self.host.view(np.uint8).copy()).to(device)
        return self


class IngestTable(_RaggedTable):
    """The geometry table of yr_ingest_geometry (INGEST_GEOM_DTYPE: src_off, ih, iw, nh, nw, dy, dx, nh_f, nw_f, dy_f, dx_f; 64 bytes an
    image); ``mode``: the rule it was computed with.  Uploaded by RaggedStager.upload."""
    DTYPE, MADE_BY = INGEST_GEOM_DTYPE, 'ingest_geometry + RaggedStager.upload / IngestTable.upload'

    def __init__(self, host, mode, input_hw, packed_bytes):
        super().__init__(host, input_hw, packed_bytes)
        self.mode = int(mode)


def _ragged_args(name, packed_u8, table, cls, input_hw):
    """The checks of a packed source and its uploaded table of class ``cls`` -> (device, H, W, B)."""
    if not (isinstance(packed_u8, torch.Tensor) and packed_u8.is_cuda and packed_u8.dtype == torch.uint8 and packed_u8.is_contiguous()):
        raise ValueError('%s: the packed source must be a contiguous uint8 CUDA tensor' % name)
    if not isinstance(table, cls) or table.device is None:
        raise ValueError('%s: the table must be an uploaded %s (%s)' % (name, cls.__name__, cls.MADE_BY))
    dev = packed_u8.device
    h, w = int(input_hw[0]), int(input_hw[1])
    b = table.batch
    if (h, w) != table.input_hw:
        raise ValueError('%s: the table was computed for %dx%d, not %dx%d' % ((name,) + table.input_hw + (h, w)))
    if table.device.device != dev or table.device.dtype != torch.uint8 or table.device.numel() != b * cls.DTYPE.itemsize:
        raise ValueError('%s: the table\'s device copy must be %d bytes on %s' % (name, b * cls.DTYPE.itemsize, dev))
    if packed_u8.numel() < table.packed_bytes - 15:
        raise ValueError('%s: the packed source holds %d bytes, the table addresses %d' % (name, packed_u8.numel(), table.packed_bytes))
    return dev, h, w, b


def _ragged_boxes(name, boxes, box_count, max_boxes, b, dev):
    """The checks of the box list of a ragged batch -> (max_in, boxes_out [B,max_boxes,5], kept [B]), fresh tensors."""
    if not (isinstance(boxes, torch.Tensor) and boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.device == dev
            and boxes.dim() == 3 and boxes.shape[0] == b and boxes.shape[2] == 5 and 1 <= boxes.shape[1] <= INGEST_MAX_BOXES):
        raise ValueError('%s: boxes must be a contiguous float32 tensor [B=%d,max_in,5] on %s with 1 <= max_in <= %d'
                         % (name, b, dev, INGEST_MAX_BOXES))
    if not (_is_cuda_i32(box_count) and box_count.device == dev and tuple(box_count.shape) == (b,)):
        raise ValueError('%s: box_count must be a contiguous int32 [B=%d] tensor on %s' % (name, b, dev))
    if int(max_boxes) < 1:
        raise ValueError('%s: max_boxes must be at least 1, not %d' % (name, max_boxes))
    return (int(boxes.shape[1]), torch.empty((b, int(max_boxes), 5), dtype=torch.float32, device=dev),
            torch.empty((b,), dtype=torch.int32, device=dev))


def ingest_geometry(dims, input_hw, mode):
    """dims: B x (ih, iw) -> IngestTable: per image the offset in the packed source (images back to back, each offset a multiple
    of 16) and the letterbox window in the rule of ``mode`` - INGEST_LETTERBOX (utils.py:67-83, what ``letterbox`` computes) or
    INGEST_VALIDATE (utils.py:239-252, the float32 geometry of the validation data path).  Host arithmetic inside the library; no
    device is touched.  YoloretHipError naming the image where one collapses to zero size."""
    dims = np.ascontiguousarray(np.asarray(dims, np.int64).reshape(-1, 2).astype(np.int32))
    if dims.shape[0] == 0:
        raise ValueError('ingest_geometry: no image')
    host = np.zeros(dims.shape[0], INGEST_GEOM_DTYPE)
    packed = ctypes.c_int64(0)
    check(lib().yr_ingest_geometry(int(mode), dims.shape[0], dims.ctypes.data_as(ctypes.c_void_p), int(input_hw[0]), int(input_hw[1]),
                                   host.ctypes.data_as(ctypes.c_void_p), ctypes.byref(packed)))
    return IngestTable(host, mode, input_hw, packed.value)


def ingest_batch(packed_u8, geom, input_hw, boxes=None, box_count=None, max_boxes=20, out=None):
    """One launch for a ragged batch.  packed_u8: uint8 CUDA tensor holding the decoded images at the offsets of ``geom`` (an
    uploaded IngestTable for ``input_hw``) -> float32 [B,H,W,3]: ``letterbox`` image by image in INGEST_LETTERBOX mode, the
    validation pipeline's image (utils.py:239-252,277) in INGEST_VALIDATE mode.  With ``boxes`` (float32 CUDA [B,max_in,5] rows
    (xmin, ymin, xmax, ymax, label) in source pixels, max_in <= 256) and ``box_count`` (int32 [B]), VALIDATE mode only:
    -> (images, boxes_out [B,max_boxes,5] mapped, clipped, filtered and cut as utils.py:253-293, kept [B] int32)."""
    dev, h, w, b = _ragged_args('ingest_batch', packed_u8, geom, IngestTable, input_hw)
    out = _out_like(out, (b, h, w, 3), dev, 'ingest_batch')
    max_in, boxes_out, kept = 0, None, None
    if boxes is not None:
        if geom.mode != INGEST_VALIDATE:
            raise ValueError('ingest_batch: boxes are mapped in INGEST_VALIDATE mode only')
        max_in, boxes_out, kept = _ragged_boxes('ingest_batch', boxes, box_count, max_boxes, b, dev)
    with torch.cuda.device(dev):
        check(lib().yr_ingest_batch(geom.mode, _ptr(packed_u8), _ptr(geom.device), b, _ptr(out), h, w, _ptr(boxes), _ptr(box_count), max_in,
                                    _ptr(boxes_out), _ptr(kept), int(max_boxes), stream_ptr(dev)))
    return out if boxes is None else (out, boxes_out, kept)


class RaggedStager:
    """Host side of the ragged ingest: packs a list of decoded uint8 images [h,w,3] and their geometry table into ONE pinned host
    buffer (reused, grown on demand) and uploads both with one non-blocking copy on the current stream.  An event recorded behind
    the copy is waited for before the buffer is written again: without it the next batch's bytes could overtake a copy in flight."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._host = None
        self._event = None

    def upload(self, images, input_hw, mode):
        """-> (packed uint8 CUDA tensor, uploaded IngestTable): the arguments of ``ingest_batch``."""
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        for i, im in enumerate(images):
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('RaggedStager: image %d has shape %s, [h,w,3] expected' % (i, im.shape))
        return self.upload_table(images, ingest_geometry([im.shape[:2] for im in images], input_hw, mode))

    def upload_table(self, images, table):
        """The same for a table the caller made (an IngestTable or an AugmentTable of these images, in this order)
        -> (packed uint8 CUDA tensor, the table, uploaded)."""
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        if table.batch != len(images) or any(tuple(im.shape) != (int(g['ih']), int(g['iw']), 3) for im, g in zip(images, table.host)):
            raise ValueError('RaggedStager: the table was not computed for these %d images' % len(images))
        tbytes = table.host.nbytes
        total = table.packed_bytes + tbytes
        if self._event is not None:
            self._event.synchronize()      # the previous copy has read the buffer
            self._event = None
        if self._host is None or self._host.numel() < total:
            self._host = torch.empty(max(total, 2 * (self._host.numel() if self._host is not None else 0)), dtype=torch.uint8, pin_memory=True)
        hv = self._host.numpy()
        for im, off in zip(images, table.host['src_off']):
            hv[off:off + im.size] = im.reshape(-1)
        hv[table.packed_bytes:total] = table.host.view(np.uint8)
        with torch.cuda.device(self.device):
            dev = torch.empty(total, dtype=torch.uint8, device=self.device)
            dev.copy_(self._host[:total], non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record(torch.cuda.current_stream(self.device))
        table.device = dev[table.packed_bytes:total]
        return dev[:table.packed_bytes], table


# ----------------------------------------------------------------------------- training data transform
AUG_HUE, AUG_SAT, AUG_GAMMA, AUG_CONTRAST, AUG_NOFLIP, AUG_ALL = 1, 2, 4, 8, 16, 31     # YR_AUG_* of include/yoloret_hip.h
AUGMENT_DEFAULTS = dict(jitter=.3, min_scale=.25, max_scale=2., hue=.5, sat=.5, min_gamma=.8, max_gamma=2., cont=.1)   # utils.py:130-140
AUGMENT_DRAWS = ('j1', 'j2', 'scale', 'dx', 'dy', 'flip', 'hue', 'sat', 'gamma', 'contrast')     # the order of one image's ten draws


class AugmentTable(_RaggedTable):
    """The table of one ragged batch under get_random_data(train=True) (yr_augment_geometry; AUGMENT_GEOM_DTYPE, 96 bytes an image);
    ``stages``: the mask it was computed with.  Uploaded by RaggedStager.upload_table."""
    DTYPE, MADE_BY = AUGMENT_GEOM_DTYPE, 'augment_geometry + RaggedStager.upload_table / AugmentTable.upload'

    def __init__(self, host, stages, input_hw, packed_bytes):
        super().__init__(host, input_hw, packed_bytes)
        self.stages = int(stages)


def augment_stages(flip=True, hue=.5, sat=.5, min_gamma=.8, max_gamma=2., cont=.1):
    """The stage mask of the reference's own conditions (utils.py:212,218,220,224,226)."""
    return ((0 if flip else AUG_NOFLIP) | (AUG_HUE if hue > 0 else 0) | (AUG_SAT if sat > 0 else 0)
            | (AUG_GAMMA if min_gamma < max_gamma else 0) | (AUG_CONTRAST if cont > 0 else 0))


def augment_geometry(dims, input_hw, draws, stages=None, flip=True, **params):
    """dims: B x (ih, iw); draws: B x 10 uniforms in [0, 1) in the order AUGMENT_DRAWS -> AugmentTable: utils.py:171-181 and the
    colour draws of :218-227 in float32, inside the library (host arithmetic, no device touched).  ``params``: jitter, min_scale,
    max_scale, hue, sat, min_gamma, max_gamma, cont (AUGMENT_DEFAULTS).  ``stages``: the mask of AUG_* bits; None derives it from
    the parameters and ``flip`` as the reference does.  YoloretHipError naming the image where a resized side truncates to 0 or a
    crop / pad precondition of TensorFlow's fails."""
    unknown = set(params) - set(AUGMENT_DEFAULTS)
    if unknown:
        raise TypeError('augment_geometry: unknown parameters %s' % sorted(unknown))
    p = dict(AUGMENT_DEFAULTS, **params)
    if stages is None:
        stages = augment_stages(flip, p['hue'], p['sat'], p['min_gamma'], p['max_gamma'], p['cont'])
    dims = np.ascontiguousarray(np.asarray(dims, np.int64).reshape(-1, 2).astype(np.int32))
    if dims.shape[0] == 0:
        raise ValueError('augment_geometry: no image')
    draws = np.ascontiguousarray(np.asarray(draws, np.float32))
    if draws.shape != (dims.shape[0], 10):
        raise ValueError('augment_geometry: draws must be [B=%d,10], not %s' % (dims.shape[0], draws.shape))
    host = np.zeros(dims.shape[0], AUGMENT_GEOM_DTYPE)
    packed = ctypes.c_int64(0)
    check(lib().yr_augment_geometry(dims.shape[0], dims.ctypes.data_as(ctypes.c_void_p), int(input_hw[0]), int(input_hw[1]),
                                    draws.ctypes.data_as(ctypes.c_void_p), int(stages), *[float(p[k]) for k in
                                    ('jitter', 'min_scale', 'max_scale', 'hue', 'sat', 'min_gamma', 'max_gamma', 'cont')],
                                    host.ctypes.data_as(ctypes.c_void_p), ctypes.byref(packed)))
    return AugmentTable(host, stages, input_hw, packed.value)


def augment_workspace_bytes(batch, input_hw):
    return int(lib().yr_augment_workspace_bytes(int(batch), int(input_hw[0]), int(input_hw[1])))


def augment_batch(packed_u8, table, input_hw, boxes=None, box_count=None, max_boxes=20, out=None, workspace=None):
    """get_random_data(train=True) for a ragged batch, two launches.  packed_u8: uint8 CUDA tensor holding the decoded images at
    the offsets of ``table`` (an uploaded AugmentTable for ``input_hw``) -> float32 [B,H,W,3].  With ``boxes`` (float32 CUDA
    [B,max_in,5] rows (xmin, ymin, xmax, ymax, label) in source pixels, max_in <= 256) and ``box_count`` (int32 [B]):
    -> (images, boxes_out [B,max_boxes,5], kept [B] int32) as utils.py:208-217,258-293.  random_jpeg_quality, which the reference
    applies by default, is the stage behind this one: ``jpeg_roundtrip_batch``.  ``workspace``: a uint8 CUDA tensor of
    augment_workspace_bytes, made here when None."""
    dev, h, w, b = _ragged_args('augment_batch', packed_u8, table, AugmentTable, input_hw)
    if h * w % 4:
        raise ValueError('augment_batch: H * W must be a multiple of 4, not %dx%d' % (h, w))
    out = _out_like(out, (b, h, w, 3), dev, 'augment_batch')
    workspace = _workspace_arg(workspace, augment_workspace_bytes(b, (h, w)), dev, 'augment_batch')
    max_in, boxes_out, kept = (0, None, None) if boxes is None else _ragged_boxes('augment_batch', boxes, box_count, max_boxes, b, dev)
    with torch.cuda.device(dev):
        check(lib().yr_augment_batch(_ptr(packed_u8), _ptr(table.device), b, table.stages, _ptr(out), h, w, _ptr(boxes), _ptr(box_count), max_in,
                                     _ptr(boxes_out), _ptr(kept), int(max_boxes), _ptr(workspace), workspace.numel(), stream_ptr(dev)))
    return out if boxes is None else (out, boxes_out, kept)


def jpeg_workspace_bytes(batch, input_hw):
    return int(lib().yr_jpeg_workspace_bytes(int(batch), int(input_hw[0]), int(input_hw[1])))


def jpeg_roundtrip_batch(images, quality, workspace=None):
    """tf.image.adjust_jpeg_quality for a batch IN PLACE, two launches (yr_jpeg_roundtrip_batch): images float32 CUDA [B,H,W,3] with
    H and W multiples of 16, quality int32 [B] (a CUDA tensor, or an array that is copied to the device; values outside 1..100 are
    clamped on the device) -> ``images``, every element the float32 image's JPEG encode at that quality (4:2:0) and decode, bit
    for bit libjpeg's arithmetic.  ``workspace``: a uint8 CUDA tensor of jpeg_workspace_bytes, made here when None."""
    _require_cuda_f32(images, 'jpeg_roundtrip_batch: images')
    if images.dim() != 4 or images.shape[3] != 3 or images.shape[0] < 1:
        raise ValueError('jpeg_roundtrip_batch: images must be [B,H,W,3], not %s' % (tuple(images.shape),))
    dev = images.device
    b, h, w = (int(n) for n in images.shape[:3])
    if h % 16 or w % 16 or h == 0 or w == 0:
        raise ValueError('jpeg_roundtrip_batch: H and W must be multiples of 16 (whole MCUs), not %dx%d' % (h, w))
    if not isinstance(quality, torch.Tensor):
        quality = np.asarray(quality)
        if quality.dtype.kind not in 'iu':
            raise ValueError('jpeg_roundtrip_batch: quality must hold integers, not %s' % quality.dtype)
        quality = torch.from_numpy(np.ascontiguousarray(quality.astype(np.int32))).to(dev)
    if not (_is_cuda_i32(quality) and quality.device == dev and tuple(quality.shape) == (b,)):
        raise ValueError('jpeg_roundtrip_batch: quality must be a contiguous int32 [B=%d] tensor on %s' % (b, dev))
    workspace = _workspace_arg(workspace, jpeg_workspace_bytes(b, (h, w)), dev, 'jpeg_roundtrip_batch')
    with torch.cuda.device(dev):
        check(lib().yr_jpeg_roundtrip_batch(_ptr(images), _ptr(quality), b, h, w, _ptr(workspace), workspace.numel(), stream_ptr(dev)))
    return images


def image_hw_tensor(image_shape, batch, device):
    """image_shape: (h,w) or [B,2] -> int32 [B,2] device tensor."""
    if isinstance(image_shape, torch.Tensor):
        t = image_shape.to(device=device, dtype=torch.int32).reshape(-1, 2)
    else:
        t = torch.as_tensor(np.asarray(image_shape).reshape(-1, 2).astype(np.int32), device=device)
    if t.shape[0] == 1 and batch > 1:
        t = t.expand(batch, 2)
    if t.shape[0] != batch:
        raise ValueError('image_shape must be (h,w) or one (h,w) per image')
    return t.contiguous()


# ----------------------------------------------------------------------------- serialised plans
PLAN_MAGIC = b'YRPLAN\0\0'


def pack_plan(ops, bufs, weights, in_hw, out_hwc, tuning=None):
    """ctypes YrOp / YrBuf arrays + float32 parameter blob (+ {batch: [cfg per op]}) -> the byte blob
    yr_create_from_blob reads (layout: include/yoloret_hip.h)."""
    import struct
    tuning = tuning or {}
    weights = np.ascontiguousarray(weights, np.float32)
    head = PLAN_MAGIC + struct.pack('<6IQ2i9i3i', ABI_VERSION, len(ops), len(bufs), ctypes.sizeof(YrOp), ctypes.sizeof(YrBuf),
                                    len(tuning), weights.size, int(in_hw[0]), int(in_hw[1]),
                                    *[int(v) for hwc in out_hwc for v in hwc], 0, 0, 0)
    assert len(head) == 96
    parts = [head, bytes(ops), bytes(bufs), weights.tobytes()]
    for batch in sorted(tuning):
        tab = np.asarray([batch] + list(tuning[batch]), np.int32)
        assert tab.size == 1 + len(ops)
        parts.append(tab.tobytes())
    return b''.join(parts)


class PlanHandle:
    """A model instantiated from a serialised plan through yr_create_from_blob - nothing of the graph compiler is
    involved (what a C / C++ / cgo / JNI host does; this class is the ctypes rendition of INTEGRATION.md's recipe).
    __call__(images [B,H,W,3] float32 CUDA) -> [y1, y2, y3] raw logits [B,G,G,A*(C+5)]."""

    def __init__(self, blob, device=None):
        blob = bytes(blob) if not isinstance(blob, (bytes, bytearray)) else blob
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = ctypes.c_void_p()
        buf = (ctypes.c_char * len(blob)).from_buffer_copy(blob)
        with torch.cuda.device(self.device):
            check(lib().yr_create_from_blob(buf, len(blob), ctypes.byref(self._h)))
        in_hw = (ctypes.c_int32 * 2)()
        out = (ctypes.c_int32 * 9)()
        check(lib().yr_plan_io_dims(self._h, in_hw, out))
        self.input_hw = (in_hw[0], in_hw[1])
        self.output_hwc = [tuple(out[3 * i:3 * i + 3]) for i in range(3)]
        self._ws = None

    def __call__(self, x):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and tuple(x.shape[1:]) == self.input_hw + (3,)):
            raise ValueError('input must be a float32 CUDA tensor [B,%d,%d,3]' % self.input_hw)
        x = x.contiguous()
        b = x.shape[0]
        L = lib()
        with torch.cuda.device(x.device):
            need = L.yr_workspace_bytes(self._h, b)
            if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
                self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
            ys = [torch.empty((b,) + hwc, dtype=torch.float32, device=x.device) for hwc in self.output_hwc]
            check(L.yr_forward(self._h, _ptr(x), b, _ptr(ys[0]), _ptr(ys[1]), _ptr(ys[2]), _ptr(self._ws),
                               self._ws.numel(), stream_ptr(x.device)))
        return ys

    def __del__(self):
        try:
            if self._h:
                lib().yr_destroy(self._h)
        except Exception:
            pass
