"""ctypes binding of libJoshUpscale.so (the C ABI in include/joshupscale_amd.h).

Host-side mirror, in Python, of what the reference exposes to its callers:

* :class:`Runtime` <-> ``JoshUpscale::core::Runtime`` / ``createRuntime``
  (reference core/public/JoshUpscale/core.h:64-92): ``process_image`` is
  ``processImage`` on BGRX frames.
* :class:`Session` <-> the recurrent drivers of the reference's Python scripts
  (scripts/inference/onnx/inference.py:46-94,
  scripts/inference/tensorrt/inference.py:60-193): ``run(image)`` takes one
  ``[H, W, 3|4]`` uint8 BGR(X) frame and returns the upscaled frame, the state
  living inside the runtime.

There is NO CPU fallback: if the HIP library is missing or no GPU is visible the
constructors raise.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

_LIB_NAME = "libJoshUpscale.so"
# The same objects with the test and measurement hooks of include/joshupscale_amd_test.h compiled in
# (ju_debug_*, ju_read_tensor, ju_time_steps).  The product library exports none of them.
_TEST_LIB_NAME = "libJoshUpscale_test.so"
_LIBS: dict = {}

LOC_CPU, LOC_DEVICE, LOC_GRAPHICS_RESOURCE = 0, 1, 2
DTYPE_DEFAULT, DTYPE_F16, DTYPE_BF16 = -1, 0, 1
# the 64->64 block convolutions of the generator on e4m3 operands (csrc/fp8.h), every
# other layer and the residual stream fp16
DTYPE_FP8 = 2
DTYPE_NAMES = {DTYPE_F16: "fp16", DTYPE_BF16: "bf16", DTYPE_FP8: "fp8"}


class JuImage(C.Structure):
    """``ju_image`` == ``JoshUpscale::core::Image`` (core.h:32-38)."""
    _fields_ = [("ptr", C.c_void_p), ("location", C.c_uint8),
                ("stride", C.c_ssize_t), ("width", C.c_size_t),
                ("height", C.c_size_t)]


# 4:2:0 frames of ju_process_frame (include/joshupscale_amd.h; formulas: INTEGRATION.md, "YUV frames"); P010 / I010:
# 10-bit samples in 16-bit words (uint16 planes; P010 the value << 6, I010 the value in the low bits)
FMT_BGRX, FMT_I420, FMT_NV12, FMT_P010, FMT_I010 = 0, 1, 2, 3, 4
# 4:2:2 (packed YUY2 / UYVY, planar I422 / I210, semi-planar P210) and 4:4:4 (I444, I410)
FMT_YUY2, FMT_UYVY, FMT_I422, FMT_P210, FMT_I210, FMT_I444, FMT_I410 = 16, 17, 18, 19, 20, 24, 25
_FMT_DEEP = (FMT_P010, FMT_I010, FMT_P210, FMT_I210, FMT_I410)
_FMT_PACKED = (FMT_YUY2, FMT_UYVY)
# RGB in other layouts and depths (tests/rgb_reference.py; `colorspace` is ignored).  Packed, ONE array: BGR24 / RGB24
# [H, W, 3] uint8, RGBX [H, W, 4] uint8, BGRX64 [H, W, 4] uint16, BGR96F [H, W, 3] float32 (0..255).  Planar, three [H, W]
# arrays R, G, B: RGBP8 uint8, RGBP10 / RGBP16 uint16, RGBPH float16, RGBPS float32 (0..1).
(FMT_BGR24, FMT_RGB24, FMT_RGBX, FMT_BGRX64, FMT_RGBP8, FMT_RGBP10, FMT_RGBP16, FMT_RGBPH, FMT_RGBPS,
 FMT_BGR96F) = range(32, 42)
# format: (samples per packed pixel, or 0 for three planes; the planes' dtype)
_FMT_RGB = {FMT_BGR24: (3, np.uint8), FMT_RGB24: (3, np.uint8), FMT_RGBX: (4, np.uint8), FMT_BGRX64: (4, np.uint16),
            FMT_RGBP8: (0, np.uint8), FMT_RGBP10: (0, np.uint16), FMT_RGBP16: (0, np.uint16),
            FMT_RGBPH: (0, np.float16), FMT_RGBPS: (0, np.float32), FMT_BGR96F: (3, np.float32)}
# Packed 10-bit (tests/packed10_reference.py), ONE array of little-endian words each: V210 uint32 [H, 4 ceil(W / 6)] (six
# pixels in four words; the array cannot tell W), Y210 uint16 [H, 2W] (Y0 U Y1 V, value << 6), Y410 / X2RGB10 / X2BGR10
# uint32 [H, W] (three 10-bit fields from bit 0 on: U, Y, V / B, G, R / R, G, B).  `colorspace` is ignored for the last two.
FMT_V210, FMT_Y210, FMT_Y410, FMT_X2RGB10, FMT_X2BGR10 = 48, 49, 50, 45, 44
_FMT_PACKED10 = (FMT_V210, FMT_Y210, FMT_Y410, FMT_X2RGB10, FMT_X2BGR10)


def v210_row_words(width: int) -> int:
    """32-bit words of a V210 row of ``width`` pixels: whole groups of six pixels, four words each."""
    return 4 * ((width + 5) // 6)


def packed10_shape(fmt: int, width: int, height: int):
    """``(dtype, shape)`` of the one array of a packed 10-bit frame (rows without padding)."""
    if fmt == FMT_V210:
        return np.uint32, (height, v210_row_words(width))
    if fmt == FMT_Y210:
        return np.uint16, (height, 2 * width)
    return np.uint32, (height, width)


CS_BT601_LIMITED, CS_BT601_FULL, CS_BT709_LIMITED, CS_BT709_FULL = 0, 1, 2, 3
CS_BT2020_LIMITED, CS_BT2020_FULL = 4, 5                         # BT.2020 non-constant luminance
# the chroma siting, or-ed into a frame's colorspace (bits 8-9): MPEG-2 / H.264 (the default), JPEG / MPEG-1, H.273 type 2
CHROMA_LEFT, CHROMA_CENTER, CHROMA_TOPLEFT = 0 << 8, 1 << 8, 2 << 8


class JuFrame(C.Structure):
    """``ju_frame``: a BGRX, YUV (FMT_I420 .. FMT_I410) or RGB (FMT_BGR24 .. FMT_BGR96F) frame, host or device."""
    _fields_ = [("format", C.c_int), ("colorspace", C.c_int), ("location", C.c_uint8),
                ("width", C.c_size_t), ("height", C.c_size_t),
                ("planes", C.c_void_p * 3), ("strides", C.c_ssize_t * 3)]


# the source stage (docs/source_stage.md): the filters of ju_set_source_size / ju_set_output_size (JU_SCALE_*; 1 is
# reserved and refused) and the limits.  A cubic filter's support is twice the triangle's: it reduces by 8 at the most.
SCALE_TRIANGLE, SCALE_CATMULL_ROM, SCALE_MITCHELL = 0, 2, 3
SCALE_FILTERS = (SCALE_TRIANGLE, SCALE_CATMULL_ROM, SCALE_MITCHELL)
SOURCE_AXIS_MIN, SOURCE_AXIS_MAX, SOURCE_RATIO_MAX = 2, 8192, 16
CUBIC_DOWN_MAX = 8


def scale_filter_problem(filter: int) -> str:
    """``""`` for a known filter, else the C layer's message."""
    if filter in SCALE_FILTERS:
        return ""
    return (f"unknown filter {filter} (the filters are JU_SCALE_TRIANGLE = 0, JU_SCALE_CATMULL_ROM = 2 and "
            "JU_SCALE_MITCHELL = 3)")


def _ratio_words(filter: int, source_side: bool) -> str:
    if filter == SCALE_TRIANGLE:
        return f" and within a factor of {SOURCE_RATIO_MAX} of"
    if source_side:
        return f", at most {CUBIC_DOWN_MAX} times and at least a {SOURCE_RATIO_MAX}th of"
    return f", at most {SOURCE_RATIO_MAX} times and at least an {CUBIC_DOWN_MAX}th of"


def source_size_problem(src_width: int, src_height: int, input_width: int, input_height: int,
                        filter: int = SCALE_TRIANGLE) -> str:
    """The limits of ``ju_set_source_size`` for a model input of ``input_width x input_height``, with the C layer's
    message; ``""`` when the source size may be set."""
    unknown = scale_filter_problem(filter)
    if unknown:
        return unknown
    down = SOURCE_RATIO_MAX if filter == SCALE_TRIANGLE else CUBIC_DOWN_MAX

    def ok(n, m):
        return SOURCE_AXIS_MIN <= n <= SOURCE_AXIS_MAX and n <= down * m and m <= SOURCE_RATIO_MAX * n
    if ok(src_width, input_width) and ok(src_height, input_height):
        return ""
    return (f"source size {src_width}x{src_height}: each axis must be {SOURCE_AXIS_MIN} .. {SOURCE_AXIS_MAX}"
            f"{_ratio_words(filter, True)} the model's input {input_width}x{input_height}")


# the output stage (docs/output_stage.md): the limits of ju_set_output_size
OUTPUT_AXIS_MIN, OUTPUT_AXIS_MAX, OUTPUT_RATIO_MAX = 2, 16384, 16


def output_size_problem(width: int, height: int, model_width: int, model_height: int, filter: int = SCALE_TRIANGLE) -> str:
    """The limits of ``ju_set_output_size`` for a model output of ``model_width x model_height``, with the C layer's
    message; ``""`` when the output size may be set."""
    unknown = scale_filter_problem(filter)
    if unknown:
        return unknown
    down = OUTPUT_RATIO_MAX if filter == SCALE_TRIANGLE else CUBIC_DOWN_MAX

    def ok(m, n):
        return OUTPUT_AXIS_MIN <= m <= OUTPUT_AXIS_MAX and n <= down * m and m <= OUTPUT_RATIO_MAX * n
    if ok(width, model_width) and ok(height, model_height):
        return ""
    return (f"output size {width}x{height}: each axis must be {OUTPUT_AXIS_MIN} .. {OUTPUT_AXIS_MAX}"
            f"{_ratio_words(filter, False)} the model's output {model_width}x{model_height}")


def tiled_output_size_problem(width: int, height: int, src_width: int, src_height: int, filter: int = SCALE_TRIANGLE) -> str:
    """The limits of ``ju_tiled_set_output_size`` for a tiled source of ``src_width x src_height``, with the C layer's
    message: those of ``ju_set_output_size`` with the blended frame, four times the source, in the model output's place;
    ``""`` when the output size may be set."""
    bw, bh = 4 * src_width, 4 * src_height
    problem = output_size_problem(width, height, bw, bh, filter)
    if not problem or scale_filter_problem(filter):
        return problem
    return f"{problem} (of a tiled object: the blended frame {bw}x{bh}, four times the tiled source size)"


# the alpha channel (docs/alpha.md): the modes of ju_set_alpha (JU_ALPHA_*)
ALPHA_ZERO, ALPHA_OPAQUE, ALPHA_SOURCE = 0, 1, 2
ALPHA_MODES = (ALPHA_ZERO, ALPHA_OPAQUE, ALPHA_SOURCE)
# where an alpha slot lies in rows of pixels (the kinds of ju_debug_alpha_scale / ju_debug_alpha_fill): byte 3 of
# four-byte pixels, word 3 of eight-byte pixels, bits 30-31 of 32-bit words; a source may have none (opaque)
ALPHA_KIND_BYTE, ALPHA_KIND_WORD, ALPHA_KIND_BITS, ALPHA_KIND_NONE = 0, 1, 2, 3


def alpha_problem(mode: int, filter: int, in_width: int, in_height: int, out_width: int, out_height: int) -> str:
    """The limits of ``ju_set_alpha`` for a runtime whose input frames are ``in_width x in_height`` and whose output
    frames are ``out_width x out_height``, with the C layer's message; ``""`` when the setting may be made.  Under
    ``ALPHA_SOURCE`` ``ju_set_source_size`` and ``ju_set_output_size`` hold the sizes they would leave to the same."""
    if mode not in ALPHA_MODES:
        return (f"unknown alpha mode {mode} (the modes are JU_ALPHA_ZERO = 0, JU_ALPHA_OPAQUE = 1 and "
                "JU_ALPHA_SOURCE = 2)")
    unknown = scale_filter_problem(filter)
    if unknown:
        return unknown
    if mode != ALPHA_SOURCE:
        return ""
    down = SOURCE_RATIO_MAX if filter == SCALE_TRIANGLE else CUBIC_DOWN_MAX

    def ok(n, m):
        return (OUTPUT_AXIS_MIN <= n <= OUTPUT_AXIS_MAX and OUTPUT_AXIS_MIN <= m <= OUTPUT_AXIS_MAX and n <= down * m and
                m <= SOURCE_RATIO_MAX * n)
    if ok(in_width, out_width) and ok(in_height, out_height):
        return ""
    return (f"alpha from the source: the input frame {in_width}x{in_height} and the output frame {out_width}x{out_height} "
            f"must be {OUTPUT_AXIS_MIN} .. {OUTPUT_AXIS_MAX} on each axis, the input at most {down} times the output and "
            f"the output at most {SOURCE_RATIO_MAX} times the input (the alpha scaler goes from one straight to the other)")


def tiled_alpha_problem(mode: int, filter: int, src_width: int, src_height: int, out_width: int = 0, out_height: int = 0) -> str:
    """The limits of ``ju_tiled_set_alpha`` for a tiled source of ``src_width x src_height`` whose output size is
    ``out_width x out_height`` (``(0, 0)``: none set), with the C layer's message: :func:`alpha_problem` with the tiled
    source size as the input frame and the output size -- else the blended frame, four times the source -- as the output
    frame.  ``ju_tiled_set_output_size`` holds the size it would leave to the same."""
    if (out_width, out_height) == (0, 0):
        out_width, out_height = 4 * src_width, 4 * src_height
    return alpha_problem(mode, filter, src_width, src_height, out_width, out_height)


LOG_CALLBACK = C.CFUNCTYPE(None, C.c_char_p, C.c_int, C.c_char_p, C.c_void_p)


class JoshUpscaleError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


class JuSceneInfo(C.Structure):
    """``ju_scene_info``: one decision of the scene detector (docs/scene_detect.md)."""
    _fields_ = [("step", C.c_uint64), ("sad", C.c_uint64), ("score", C.c_uint64), ("cut", C.c_uint32),
                ("reserved", C.c_uint32)]


SCENE_OFF, SCENE_REPORT, SCENE_RESET = 0, 1, 2
SCENE_RING = 64


class JuTiledInfo(C.Structure):
    """``ju_tiled_info``: the sizes and the tile grid of a tiled runtime (docs/tiled.md)."""
    _fields_ = [("src_width", C.c_size_t), ("src_height", C.c_size_t), ("out_width", C.c_size_t),
                ("out_height", C.c_size_t), ("tile_width", C.c_size_t), ("tile_height", C.c_size_t),
                ("tiles_x", C.c_int), ("tiles_y", C.c_int), ("overlap", C.c_int)]


# the argument structs of the compute-kernel hooks (include/joshupscale_amd_test.h; docs/exact_tests.md)
class JuDebugPlan(C.Structure):
    """``ju_debug_plan``: the developer launch plan of one hook launch (conv_stages -1, the rest 0: the launcher's choice)."""
    _fields_ = [(n, C.c_int) for n in ("flow_tile", "res_block", "conv_stages", "splitk_rows", "splitk_blocks", "conv_nb",
                                       "conv_rw")]


class JuDebugConv(C.Structure):
    """``ju_debug_conv_args``."""
    _fields_ = [("kernel", C.c_int), ("dtype", C.c_int), ("inp", C.c_void_p), ("res", C.c_void_p), ("out", C.c_void_p),
                ("weights", C.c_void_p), ("bias", C.c_void_p)] + \
               [(n, C.c_int) for n in ("H", "W", "cin", "cin_real", "cout", "taps", "relu")] + [("slope", C.c_float)] + \
               [(n, C.c_int) for n in ("out_head", "pool", "upsample", "nb", "rw", "in_pitch", "out_pitch", "res_pitch", "items")] + \
               [("in_item_bytes", C.c_longlong), ("out_item_bytes", C.c_longlong), ("plan", JuDebugPlan),
                ("plan_text", C.c_void_p), ("plan_capacity", C.c_size_t)]


class JuDebugFlowBlock(C.Structure):
    """``ju_debug_flow_block_args``."""
    _fields_ = [("dtype", C.c_int), ("inp", C.c_void_p), ("out", C.c_void_p), ("weights1", C.c_void_p), ("bias1", C.c_void_p),
                ("weights2", C.c_void_p), ("bias2", C.c_void_p)] + \
               [(n, C.c_int) for n in ("H", "W", "cin", "cin_real", "cmid", "upsample", "pool", "out_head", "residual", "act1",
                                       "act2")] + [("slope", C.c_float)] + \
               [(n, C.c_int) for n in ("in_pitch", "out_pitch", "items")] + \
               [("in_item_bytes", C.c_longlong), ("out_item_bytes", C.c_longlong), ("plan", JuDebugPlan),
                ("plan_text", C.c_void_p), ("plan_capacity", C.c_size_t)]


class JuDebugResample(C.Structure):
    """``ju_debug_resample_args``."""
    _fields_ = [("op", C.c_int), ("dtype", C.c_int), ("inp", C.c_void_p), ("out", C.c_void_p)] + \
               [(n, C.c_int) for n in ("H", "W", "C", "items")]


class JuDebugWarp(C.Structure):
    """``ju_debug_warp_args``."""
    _fields_ = [("dtype", C.c_int), ("state", C.c_void_p), ("flow", C.c_void_p), ("frame", C.c_void_p),
                ("frame_stride", C.c_ssize_t), ("out", C.c_void_p)] + \
               [(n, C.c_int) for n in ("out_pitch", "H", "W", "PW", "pad_top", "pad_left")] + \
               [("sums", C.c_void_p), ("pre_warp_out", C.c_void_p), ("out_u8", C.c_void_p), ("out_stride", C.c_ssize_t)]


def hooks_default() -> bool:
    """``JU_TEST_HOOKS=1`` (set by tests/conftest.py and the developer tools): the process works
    through libJoshUpscale_test.so.  Unset -- every caller of the product -- it is the product library."""
    return os.environ.get("JU_TEST_HOOKS", "0") == "1"


def library_path(hooks: Optional[bool] = None) -> str:
    """In-tree HIP library (``hooks``: its test flavour); ``JU_LIBRARY`` points at another build
    (A/B timing: such a build carries the hooks or not as it was linked)."""
    override = os.environ.get("JU_LIBRARY")
    if override:
        return override
    hooks = hooks_default() if hooks is None else hooks
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                        _TEST_LIB_NAME if hooks else _LIB_NAME)


_P = C.POINTER
_PRODUCT_SIGS = {
    "ju_create": (C.c_int, [C.c_int, C.c_char_p, _P(C.c_void_p)]),
    "ju_create_from_memory": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, _P(C.c_void_p)]),
    "ju_validate_model": (C.c_int, [C.c_void_p, C.c_size_t]),
    "ju_destroy": (None, [C.c_void_p]),
    "ju_process": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage)]),
    "ju_process_batch": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage), C.c_int]),
    "ju_process_group": (C.c_int, [_P(C.c_void_p), _P(JuImage), _P(JuImage), C.c_int]),
    "ju_process_group_frames": (C.c_int, [_P(C.c_void_p), _P(JuFrame), _P(JuFrame), C.c_int]),
    "ju_prepare_batch": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage), C.c_int, _P(C.c_int)]),
    "ju_set_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_enqueue": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage)]),
    "ju_synchronize": (C.c_int, [C.c_void_p]),
    "ju_prepare_frames": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage), _P(C.c_int)]),
    "ju_process_frame": (C.c_int, [C.c_void_p, _P(JuFrame), _P(JuFrame)]),
    "ju_process_frames": (C.c_int, [C.c_void_p, _P(JuFrame), _P(JuFrame), C.c_int]),
    "ju_enqueue_frame": (C.c_int, [C.c_void_p, _P(JuFrame), _P(JuFrame)]),
    "ju_get_size": (C.c_int, [C.c_void_p] + [_P(C.c_size_t)] * 4),
    "ju_reset": (C.c_int, [C.c_void_p]),
    "ju_set_scene_detect": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    "ju_get_scene_detect": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_uint32)]),
    "ju_get_scene_info": (C.c_int, [C.c_void_p, _P(JuSceneInfo), C.c_int, _P(C.c_int)]),
    "ju_set_scene_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_set_scene_group": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_set_stage_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_set_stage_group": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_set_source_size": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]),
    "ju_get_source_size": (C.c_int, [C.c_void_p, _P(C.c_size_t), _P(C.c_size_t)]),
    "ju_set_source_mask": (C.c_int, [C.c_void_p, _P(JuImage)]),
    "ju_set_output_size": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]),
    "ju_get_output_size": (C.c_int, [C.c_void_p, _P(C.c_size_t), _P(C.c_size_t)]),
    "ju_set_alpha": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ju_get_alpha": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_int)]),
    "ju_set_alpha_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_set_alpha_group": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_tiled_set_alpha": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "ju_tiled_get_alpha": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_int)]),
    "ju_tiled_create": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, _P(C.c_void_p)]),
    "ju_tiled_create_from_memory": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                              _P(C.c_void_p)]),
    "ju_tiled_destroy": (None, [C.c_void_p]),
    "ju_tiled_reset": (C.c_int, [C.c_void_p]),
    "ju_tiled_set_deep_from_state": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_tiled_set_output_size": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]),
    "ju_tiled_get_output_size": (C.c_int, [C.c_void_p, _P(C.c_size_t), _P(C.c_size_t)]),
    "ju_tiled_set_source_mask": (C.c_int, [C.c_void_p, _P(JuImage)]),
    "ju_tiled_process": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage)]),
    "ju_tiled_process_frame": (C.c_int, [C.c_void_p, _P(JuFrame), _P(JuFrame)]),
    "ju_tiled_process_batch": (C.c_int, [C.c_void_p, _P(JuImage), _P(JuImage), C.c_int]),
    "ju_tiled_process_frames": (C.c_int, [C.c_void_p, _P(JuFrame), _P(JuFrame), C.c_int]),
    "ju_tiled_set_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "ju_tiled_get_info": (C.c_int, [C.c_void_p, _P(JuTiledInfo)]),
    "ju_tiled_get_tile": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_size_t), _P(C.c_size_t)]),
    "ju_tiled_get_stat": (C.c_int, [C.c_void_p, C.c_char_p, _P(C.c_double)]),
    "ju_tiled_set_scene_detect": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    "ju_tiled_get_scene_detect": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_uint32)]),
    "ju_tiled_get_scene_info": (C.c_int, [C.c_void_p, _P(JuSceneInfo), C.c_int, _P(C.c_int)]),
    "ju_last_error": (C.c_char_p, []),
    "ju_set_log_callback": (None, [LOG_CALLBACK, C.c_void_p]),
    "ju_get_gl_device_index": (C.c_int, [_P(C.c_int)]),
    "ju_get_gl_image": (C.c_int, [C.c_uint32, C.c_int, _P(JuImage)]),
    "ju_release_gl_image": (None, [_P(JuImage)]),
    "ju_get_dtype": (C.c_int, [C.c_void_p]),
    "ju_get_stat": (C.c_int, [C.c_void_p, C.c_char_p, _P(C.c_double)]),
    "ju_version": (C.c_char_p, []),
    "ju_comm_unique_id": (C.c_int, [C.c_void_p]),
    "ju_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _P(C.c_void_p)]),
    "ju_comm_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "ju_comm_allreduce_max": (C.c_int, [C.c_void_p, _P(C.c_double)]),
    "ju_comm_count": (C.c_int, [C.c_void_p, _P(C.c_int)]),
    "ju_comm_destroy": (None, [C.c_void_p]),
}
# include/joshupscale_amd_test.h
_HOOK_SIGS = {
    "ju_debug_fake_gl_texture": (C.c_int, [C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]),
    "ju_debug_fake_gl_counters": (None, [_P(C.c_int)] * 4),
    "ju_debug_e4m3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "ju_debug_yuv": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t,
                               _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_yuv10": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t,
                                 _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_yuv_sampled": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t,
                                       _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_rgb": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t, _P(C.c_void_p),
                               _P(C.c_ssize_t)]),
    "ju_debug_packed10": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t,
                                    _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_yuv_items": (C.c_int, [C.c_int, _P(C.c_int), _P(C.c_int), C.c_size_t, C.c_size_t, _P(C.c_void_p),
                                     _P(C.c_ssize_t), _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_yuv_items_sized": (C.c_int, [C.c_int, _P(C.c_int), _P(C.c_int), _P(C.c_size_t), _P(C.c_size_t), _P(C.c_void_p),
                                           _P(C.c_ssize_t), _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_source": (C.c_int, [C.c_int, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t,
                                  C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t]),
    "ju_debug_output": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                  C.c_int, _P(C.c_void_p), _P(C.c_ssize_t)]),
    "ju_debug_scene": (C.c_int, [C.c_int, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_uint32, C.c_int, _P(JuSceneInfo), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "ju_debug_scene_pass": (C.c_int, [C.c_int, _P(C.c_void_p), _P(C.c_ssize_t), C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_int, _P(JuSceneInfo), _P(C.c_uint32),
                                      _P(C.c_int32)]),
    "ju_debug_scene_group": (C.c_int, [C.c_int, _P(C.c_void_p), _P(C.c_ssize_t), C.c_size_t, C.c_size_t, _P(C.c_void_p),
                                       _P(C.c_void_p), _P(C.c_int), _P(C.c_uint64), _P(C.c_uint32), _P(C.c_int),
                                       _P(JuSceneInfo), _P(C.c_uint32)]),
    "ju_debug_scene_clear_items": (C.c_int, [C.c_int, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_size_t), _P(C.c_void_p),
                                             _P(C.c_size_t)]),
    "ju_debug_scale": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_ssize_t,
                                 C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ju_debug_alpha_scale": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                       C.c_ssize_t, C.c_size_t, C.c_size_t]),
    "ju_debug_alpha_fill": (C.c_int, [C.c_int, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t]),
    "ju_debug_alpha_problem": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "ju_debug_tiled_alpha_problem": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "ju_debug_scale_items": (C.c_int, [C.c_int, C.c_int, _P(C.c_void_p), _P(C.c_ssize_t), C.c_size_t, C.c_size_t,
                                       _P(C.c_void_p), _P(C.c_ssize_t), C.c_size_t, C.c_size_t]),
    "ju_debug_scale_members": (C.c_int, [C.c_int, _P(C.c_int), _P(C.c_void_p), _P(C.c_ssize_t), C.c_size_t, C.c_size_t,
                                         _P(C.c_void_p), _P(C.c_ssize_t), _P(C.c_size_t), _P(C.c_size_t)]),
    "ju_debug_temporal": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                    C.c_float, C.c_float, C.c_float, C.c_int, C.c_uint, C.c_void_p, C.c_size_t]),
    "ju_debug_tile_split": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                      _P(C.c_void_p), C.c_int]),
    "ju_debug_tile_stitch": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                       _P(C.c_void_p), C.c_int]),
    "ju_debug_tile_stitch_state": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                             _P(C.c_void_p), C.c_int]),
    "ju_debug_tile_stitch_scale": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t,
                                             C.c_size_t, C.c_size_t, C.c_int, _P(C.c_void_p), C.c_int]),
    "ju_debug_tile_stitch_scale_state": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t,
                                                   C.c_size_t, C.c_size_t, C.c_int, _P(C.c_void_p), C.c_int]),
    "ju_debug_tile_stitch_mask": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                            _P(C.c_void_p), C.c_int, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t,
                                            C.c_size_t, C.c_size_t]),
    "ju_debug_tile_stitch_mask_scale": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t,
                                                  C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P(C.c_void_p), C.c_int,
                                                  C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t]),
    "ju_debug_mask_box": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P(C.c_int)]),
    "ju_debug_tile_split_scene": (C.c_int, [C.c_void_p, C.c_ssize_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                            _P(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, _P(JuSceneInfo), C.c_int,
                                            C.c_uint32, C.c_int]),
    "ju_debug_tile_split_frames": (C.c_int, [_P(C.c_void_p), _P(C.c_ssize_t), C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                             C.c_size_t, C.c_int, _P(C.c_void_p), C.c_size_t, C.c_int]),
    "ju_debug_tiled_pass_plan": (C.c_int, [C.c_int, C.c_int, C.c_char_p, _P(C.c_int), C.c_int, _P(C.c_int)]),
    "ju_debug_scene_clear_tiles": (C.c_int, [C.c_int, C.c_void_p, _P(C.c_void_p), _P(C.c_size_t), _P(C.c_void_p),
                                             _P(C.c_size_t)]),
    "ju_debug_conv": (C.c_int, [_P(JuDebugConv)]),
    "ju_debug_flow_block": (C.c_int, [_P(JuDebugFlowBlock)]),
    "ju_debug_resample": (C.c_int, [_P(JuDebugResample)]),
    "ju_debug_warp": (C.c_int, [_P(JuDebugWarp)]),
    "ju_read_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "ju_time_steps": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, _P(C.c_double), _P(C.c_int), _P(C.c_double)]),
    "ju_plan_report": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, _P(C.c_size_t)]),
    "ju_debug_set": (C.c_int, [C.c_char_p, C.c_int]),
}
PRODUCT_SYMBOLS = tuple(sorted(_PRODUCT_SIGS))
HOOK_SYMBOLS = tuple(sorted(_HOOK_SIGS))


def load_library(hooks: Optional[bool] = None) -> C.CDLL:
    """Load the HIP library; fails loudly (no fallback) when it is not built.  ``hooks`` selects the
    test flavour (default: ``JU_TEST_HOOKS``); a library that lacks a hook raises when the hook is used."""
    hooks = hooks_default() if hooks is None else hooks
    path = library_path(hooks)
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make` (or "
            "`python -c 'import __graft_entry__ as g; g.build()'`). "
            "joshupscale_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in _PRODUCT_SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in _HOOK_SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if hooks:
                raise ImportError(f"{path} does not export {name}: not a -DJU_TEST_HOOKS build") from None
            continue
        fn.restype = res
        fn.argtypes = args
    _LIBS[path] = lib
    return lib


def _hook(lib: C.CDLL, name: str):
    try:
        return getattr(lib, name)
    except AttributeError:
        raise RuntimeError(f"{name} is a test hook (include/joshupscale_amd_test.h): the product library does not "
                           "export it; set JU_TEST_HOOKS=1 or pass hooks=True to work through "
                           "libJoshUpscale_test.so") from None


def _check(lib: C.CDLL, rc: int) -> None:
    if rc != 0:
        raise JoshUpscaleError(rc, lib.ju_last_error().decode(errors="replace"))


def validate_model(model: bytes) -> None:
    """Check a container with the C++ loader (``ju_validate_model``): no GPU needed.
    Raises :class:`JoshUpscaleError` with the loader's message."""
    lib = load_library()
    buf = bytes(model)
    _check(lib, lib.ju_validate_model(buf, len(buf)))


class Runtime:
    """One recurrent SR stream on one GPU (``JoshUpscale::core::Runtime``)."""

    def __init__(self, model, device: int = 0, dtype: int = DTYPE_DEFAULT, hooks: Optional[bool] = None):
        """``model``: path of a .jupw file, or its bytes.  ``hooks``: through libJoshUpscale_test.so
        (``read_tensor`` / ``time_steps`` need it; default: ``JU_TEST_HOOKS``)."""
        self._lib = load_library(hooks)
        self._h = C.c_void_p()
        if isinstance(model, (bytes, bytearray, memoryview)):
            buf = bytes(model)
            _check(self._lib, self._lib.ju_create_from_memory(
                device, buf, len(buf), dtype, C.byref(self._h)))
        else:
            if dtype != DTYPE_DEFAULT:
                with open(model, "rb") as f:
                    buf = f.read()
                _check(self._lib, self._lib.ju_create_from_memory(
                    device, buf, len(buf), dtype, C.byref(self._h)))
            else:
                _check(self._lib, self._lib.ju_create(
                    device, os.fsencode(model), C.byref(self._h)))
        w = [C.c_size_t() for _ in range(4)]
        _check(self._lib, self._lib.ju_get_size(self._h, *[C.byref(x) for x in w]))
        self.input_width, self.input_height, self.output_width, self.output_height = (
            x.value for x in w)
        self.device = device

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ju_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- the boundary ------------------------------------------------------
    @property
    def dtype(self) -> int:
        return self._lib.ju_get_dtype(self._h)

    def process(self, inp: JuImage, out: JuImage) -> None:
        """Raw ``processImage`` on two image descriptors (synchronous)."""
        _check(self._lib, self._lib.ju_process(self._h, C.byref(inp), C.byref(out)))

    def process_batch(self, inputs, outputs) -> None:
        """``ju_process_batch``: consecutive frames of the stream in one synchronous call (frame look-ahead --
        every input must hold its pixels now); the bytes of ``process`` called frame by frame."""
        n = len(inputs)
        if len(outputs) != n:
            raise ValueError("as many outputs as inputs")
        ins, outs = (JuImage * n)(*inputs), (JuImage * n)(*outputs)
        _check(self._lib, self._lib.ju_process_batch(self._h, ins, outs, n))

    def prepare_batch(self, inputs, outputs) -> int:
        """``ju_prepare_batch``: capture the graphs of a tuple of device frame buffers that will go through
        ``process_batch`` as one pass; returns the graphs captured (0: the tuple will not run as one pass)."""
        n = len(inputs)
        if len(outputs) != n:
            raise ValueError("as many outputs as inputs")
        ins, outs = (JuImage * n)(*inputs), (JuImage * n)(*outputs)
        got = C.c_int()
        _check(self._lib, self._lib.ju_prepare_batch(self._h, ins, outs, n, C.byref(got)))
        return got.value

    def set_lookahead(self, frames: int) -> None:
        """``ju_set_lookahead``: frames per look-ahead pass of ``process_batch`` (1 = frame by frame, at most 8)."""
        _check(self._lib, self._lib.ju_set_lookahead(self._h, int(frames)))

    def enqueue(self, inp: JuImage, out: JuImage) -> None:
        _check(self._lib, self._lib.ju_enqueue(self._h, C.byref(inp), C.byref(out)))

    def synchronize(self) -> None:
        _check(self._lib, self._lib.ju_synchronize(self._h))

    def prepare_frames(self, inp: JuImage, out: JuImage) -> int:
        """``ju_prepare_frames``: capture the graphs of a device frame-buffer pair now
        (the reference captures in its constructor); returns the graphs captured."""
        n = C.c_int()
        _check(self._lib, self._lib.ju_prepare_frames(self._h, C.byref(inp), C.byref(out), C.byref(n)))
        return n.value

    def reset(self) -> None:
        _check(self._lib, self._lib.ju_reset(self._h))

    # -- the scene detector (docs/scene_detect.md) --------------------------------
    def set_scene_detect(self, mode: int, threshold_milli: int = 10000) -> None:
        """``ju_set_scene_detect``: ``SCENE_OFF``, ``SCENE_REPORT`` (record cuts) or ``SCENE_RESET`` (and restart the
        recurrence at them, on the GPU); ``threshold_milli`` in thousandths of a code value per byte, 1 .. 255000
        (10000 = ffmpeg scdet's default).  An unknown mode or a threshold out of range raises
        :class:`JoshUpscaleError` with the C layer's message."""
        mode, threshold_milli = int(mode), int(threshold_milli)
        if not 0 <= threshold_milli < 2 ** 32:
            raise ValueError("threshold_milli must fit 32 bits")
        _check(self._lib, self._lib.ju_set_scene_detect(self._h, mode, threshold_milli))

    def get_scene_detect(self) -> Tuple[int, int]:
        """``ju_get_scene_detect``: ``(mode, threshold_milli)``; the threshold is 0 while the mode is off."""
        mode, thr = C.c_int(), C.c_uint32()
        _check(self._lib, self._lib.ju_get_scene_detect(self._h, C.byref(mode), C.byref(thr)))
        return mode.value, thr.value

    def scene_info(self, count: int = SCENE_RING) -> list:
        """``ju_get_scene_info``: waits for the stream; the most recent ``min(count, 64, steps seen)`` decisions, oldest
        first, as dicts ``{"step", "sad", "score", "cut"}``."""
        count = max(0, int(count))
        recs = (JuSceneInfo * max(count, 1))()
        got = C.c_int()
        _check(self._lib, self._lib.ju_get_scene_info(self._h, recs, count, C.byref(got)))
        return [{"step": r.step, "sad": r.sad, "score": r.score, "cut": int(r.cut)} for r in recs[:got.value]]

    def set_scene_lookahead(self, on) -> None:
        """``ju_set_scene_lookahead``: 1 = ``process_batch`` / ``process_frames`` form look-ahead passes while the detector
        is on, and the passes carry it (docs/scene_detect.md "Passes"); 0 (the default) = such frames run one by one.  A
        value other than 0 or 1 raises :class:`JoshUpscaleError` with the C layer's message."""
        _check(self._lib, self._lib.ju_set_scene_lookahead(self._h, int(on)))

    def set_scene_group(self, on) -> None:
        """``ju_set_scene_group``: 1 = this runtime rides in the passes of ``process_group`` / ``process_group_frames``
        while its detector is on, and the passes carry it (docs/scene_detect.md "Group passes"); 0 (the default) = it
        runs on its own.  A value other than 0 or 1 raises :class:`JoshUpscaleError` with the C layer's message."""
        _check(self._lib, self._lib.ju_set_scene_group(self._h, int(on)))

    def set_stage_lookahead(self, on) -> None:
        """``ju_set_stage_lookahead``: 1 = ``process_batch`` / ``process_frames`` form look-ahead passes while a source
        size, a mask or an output size is set, and the passes carry those stages (docs/source_stage.md and
        docs/output_stage.md, "Passes"); 0 (the default) = such frames run one by one.  A value other than 0 or 1 raises
        :class:`JoshUpscaleError` with the C layer's message."""
        _check(self._lib, self._lib.ju_set_stage_lookahead(self._h, int(on)))

    def set_stage_group(self, on) -> None:
        """``ju_set_stage_group``: 1 = this runtime rides in the passes of ``process_group`` / ``process_group_frames``
        while a source size, a mask or an output size is set, and the pass carries its stages (docs/source_stage.md and
        docs/output_stage.md, "Group passes"); 0 (the default) = such a member runs on its own.  Independent of
        ``set_stage_lookahead``.  A value other than 0 or 1 raises :class:`JoshUpscaleError` with the C layer's message."""
        _check(self._lib, self._lib.ju_set_stage_group(self._h, int(on)))

    # -- the source stage (docs/source_stage.md) ----------------------------------
    def set_source_size(self, width: int, height: int, filter: int = SCALE_TRIANGLE) -> None:
        """``ju_set_source_size``: input frames are ``width x height`` from now on and are scaled to the model's input on
        the GPU by ``filter`` (``SCALE_TRIANGLE``, ``SCALE_CATMULL_ROM`` or ``SCALE_MITCHELL``); ``(0, 0)`` turns it off.
        The limits and an unknown filter raise ``ValueError`` with the C layer's message before any native call."""
        width, height, filter = int(width), int(height), int(filter)
        off = (width, height) == (0, 0)
        problem = scale_filter_problem(filter) if off else \
            source_size_problem(width, height, self.input_width, self.input_height, filter)
        if problem:
            raise ValueError("ju_set_source_size: " + problem)
        self._alpha_allows("ju_set_source_size", (self.input_width, self.input_height) if off else (width, height),
                           self.frame_output_size())
        _check(self._lib, self._lib.ju_set_source_size(self._h, width, height, filter))

    def get_source_size(self) -> Tuple[int, int]:
        """``ju_get_source_size``: ``(width, height)``, ``(0, 0)`` while no source size is set."""
        w, h = C.c_size_t(), C.c_size_t()
        _check(self._lib, self._lib.ju_get_source_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_source_mask(self, mask) -> None:
        """``ju_set_source_mask``: ``mask`` is a ``[H, W, 4]`` uint8 BGRX array of any size, a :class:`JuImage` (host or
        device), or ``None`` to remove the mask.  The runtime copies it."""
        if mask is None:
            _check(self._lib, self._lib.ju_set_source_mask(self._h, None))
            return
        if not isinstance(mask, JuImage):
            if mask.dtype != np.uint8 or mask.ndim != 3 or mask.shape[2] != 4 or mask.strides[2] != 1 or mask.strides[1] != 4:
                raise ValueError("expected a [H, W, 4] uint8 BGRX mask with contiguous pixels")
            mask = host_image(mask)
        _check(self._lib, self._lib.ju_set_source_mask(self._h, C.byref(mask)))

    # -- the output stage (docs/output_stage.md) ----------------------------------
    def set_output_size(self, width: int, height: int, filter: int = SCALE_TRIANGLE) -> None:
        """``ju_set_output_size``: output frames are ``width x height`` from now on, the upscaled frame scaled on the GPU
        by ``filter`` (as for ``set_source_size``); ``(0, 0)`` turns it off.  The limits raise ``ValueError`` with the C layer's message before any native call."""
        width, height, filter = int(width), int(height), int(filter)
        off = (width, height) == (0, 0)
        problem = output_size_problem(self.output_width if off else width, self.output_height if off else height,
                                      self.output_width, self.output_height, filter)
        if problem:
            raise ValueError("ju_set_output_size: " + problem)
        self._alpha_allows("ju_set_output_size", self.frame_input_size(),
                           (self.output_width, self.output_height) if off else (width, height))
        _check(self._lib, self._lib.ju_set_output_size(self._h, width, height, filter))

    def get_output_size(self) -> Tuple[int, int]:
        """``ju_get_output_size``: ``(width, height)``, ``(0, 0)`` while no output size is set."""
        w, h = C.c_size_t(), C.c_size_t()
        _check(self._lib, self._lib.ju_get_output_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def frame_output_size(self) -> Tuple[int, int]:
        """``(width, height)`` of the frames the runtime hands out now: the output size set, else the model's output."""
        w, h = self.get_output_size()
        return (w, h) if w else (self.output_width, self.output_height)

    def frame_input_size(self) -> Tuple[int, int]:
        """``(width, height)`` of the frames the runtime takes now: the source size set, else the model's input."""
        w, h = self.get_source_size()
        return (w, h) if w else (self.input_width, self.input_height)

    # -- the alpha channel (docs/alpha.md) -----------------------------------------
    def set_alpha(self, mode: int, filter: int = SCALE_TRIANGLE) -> None:
        """``ju_set_alpha``: what the alpha slot of output frames holds -- ``ALPHA_ZERO`` (0, the default: every route
        as without the call), ``ALPHA_OPAQUE`` (the format's top code) or ``ALPHA_SOURCE`` (the input frame's alpha,
        scaled by ``filter`` from the input frame's size straight to the output frame's size).  The filter is checked in
        every mode.  An unknown mode or filter and, under ``ALPHA_SOURCE``, frame sizes beyond the scaler raise
        ``ValueError`` with the C layer's message before any native call; the setting stays as it was."""
        mode, filter = int(mode), int(filter)
        problem = alpha_problem(mode, filter, *self.frame_input_size(), *self.frame_output_size())
        if problem:
            raise ValueError("ju_set_alpha: " + problem)
        _check(self._lib, self._lib.ju_set_alpha(self._h, mode, filter))

    def get_alpha(self) -> Tuple[int, int]:
        """``ju_get_alpha``: ``(mode, filter)`` as set; ``(ALPHA_ZERO, SCALE_TRIANGLE)`` on a fresh runtime."""
        mode, filter = C.c_int(), C.c_int()
        _check(self._lib, self._lib.ju_get_alpha(self._h, C.byref(mode), C.byref(filter)))
        return mode.value, filter.value

    def set_alpha_lookahead(self, on) -> None:
        """``ju_set_alpha_lookahead``: 1 = ``process_batch`` / ``process_frames`` form look-ahead passes while the alpha
        mode is not ``ALPHA_ZERO`` (the stage and scene settings decide as in mode 0), and each frame's alpha launch
        follows its colour inside the pass (docs/alpha.md "Passes"); 0 (the default) = such frames run one by one.
        ``reset`` and ``set_alpha`` keep it.  A value other than 0 or 1 raises :class:`JoshUpscaleError` with the C
        layer's message."""
        _check(self._lib, self._lib.ju_set_alpha_lookahead(self._h, int(on)))

    def set_alpha_group(self, on) -> None:
        """``ju_set_alpha_group``: 1 = this runtime rides in the passes of ``process_group`` / ``process_group_frames``
        while its alpha mode is not ``ALPHA_ZERO``, and the pass makes its alpha launch with this member's own mode,
        filter and sizes (docs/alpha.md "Passes"); 0 (the default) = such a member runs on its own.  Independent of
        ``set_alpha_lookahead``.  A value other than 0 or 1 raises :class:`JoshUpscaleError` with the C layer's message."""
        _check(self._lib, self._lib.ju_set_alpha_group(self._h, int(on)))

    def _alpha_allows(self, who: str, in_size, out_size) -> None:
        """What ``set_source_size`` / ``set_output_size`` ask before they change a size: under ``ALPHA_SOURCE`` the alpha
        scaler must still reach from the one frame size to the other."""
        mode, filter = self.get_alpha()
        problem = alpha_problem(mode, filter, *in_size, *out_size)
        if problem:
            raise ValueError(f"{who}: {problem}")

    def process_image(self, frame_bgrx: np.ndarray,
                      out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host frames: ``[H, W, 4]`` uint8 in, ``[4H, 4W, 4]`` uint8 out (``[OH, OW, 4]`` while an output size is
        set).  Any row stride (also negative, i.e. a ``[::-1]`` view) is passed through."""
        if frame_bgrx.dtype != np.uint8 or frame_bgrx.ndim != 3 or frame_bgrx.shape[2] != 4:
            raise ValueError("expected a [H, W, 4] uint8 BGRX frame")
        if frame_bgrx.strides[2] != 1 or frame_bgrx.strides[1] != 4:
            frame_bgrx = np.ascontiguousarray(frame_bgrx)
        if out is None:
            ow, oh = self.frame_output_size()
            out = np.empty((oh, ow, 4), np.uint8)
        if out.strides[2] != 1 or out.strides[1] != 4:
            raise ValueError("output must have contiguous pixels")
        self.process(host_image(frame_bgrx), host_image(out))
        return out

    def process_frame(self, inp: JuFrame, out: JuFrame) -> None:
        """``ju_process_frame``: one step on frames of any format (synchronous)."""
        _check(self._lib, self._lib.ju_process_frame(self._h, C.byref(inp), C.byref(out)))

    def process_frames(self, inputs, outputs) -> None:
        """``ju_process_frames``: consecutive frames of the stream, of any format, in one synchronous call (frame
        look-ahead -- every input must hold its pixels now); the bytes of ``process_frame`` called frame by frame.
        Lists of unequal length raise before any native call."""
        inputs, outputs = list(inputs), list(outputs)
        n = len(inputs)
        if len(outputs) != n:
            raise ValueError("process_frames: as many outputs as inputs")
        ins, outs = (JuFrame * n)(*inputs), (JuFrame * n)(*outputs)
        _check(self._lib, self._lib.ju_process_frames(self._h, ins, outs, n))

    def enqueue_frame(self, inp: JuFrame, out: JuFrame) -> None:
        """``ju_enqueue_frame``: device frames only; ``synchronize`` waits."""
        _check(self._lib, self._lib.ju_enqueue_frame(self._h, C.byref(inp), C.byref(out)))

    def process_yuv(self, y: np.ndarray, u: Optional[np.ndarray] = None, v: Optional[np.ndarray] = None, fmt: int = FMT_I420,
                    colorspace: int = CS_BT709_LIMITED, out_format: Optional[int] = None, width: Optional[int] = None):
        """Host planes in, host planes out.  ``fmt`` FMT_I420 / FMT_I010: ``y, u, v``; FMT_NV12 / FMT_P010: ``y, uv``
        (``v`` None); the 10-bit formats take and return ``uint16`` planes.  ``out_format`` (default: ``fmt``):
        FMT_I420 / FMT_I010 -> ``(y, u, v)``, FMT_NV12 / FMT_P010 -> ``(y, uv)``, FMT_BGRX -> the ``[4H, 4W, 4]`` BGRX
        frame.  The packed 10-bit formats (FMT_V210 / FMT_Y210 / FMT_Y410): ``y`` is the one array of words (``u``, ``v``
        None; FMT_V210 needs ``width``), and such an ``out_format`` returns a one-element tuple with its array."""
        out_format = fmt if out_format is None else out_format
        planes = [y] if fmt in _FMT_PACKED10 else ([y, u] if fmt in (FMT_NV12, FMT_P010) else [y, u, v])
        inp = host_frame(fmt, planes, colorspace, width=width)
        ow, oh = self.frame_output_size()
        sample = np.uint16 if out_format in (FMT_P010, FMT_I010) else np.uint8
        if out_format == FMT_BGRX:
            res = [np.empty((oh, ow, 4), np.uint8)]
        elif out_format in _FMT_PACKED10:
            dt, shape = packed10_shape(out_format, ow, oh)
            res = [np.empty(shape, dt)]
        elif out_format in (FMT_NV12, FMT_P010):
            res = [np.empty((oh, ow), sample), np.empty((oh // 2, ow), sample)]
        else:
            res = [np.empty((oh, ow), sample), np.empty((oh // 2, ow // 2), sample),
                   np.empty((oh // 2, ow // 2), sample)]
        self.process_frame(inp, host_frame(out_format, res, colorspace, width=ow if out_format == FMT_V210 else None))
        return res[0] if out_format == FMT_BGRX else tuple(res)

    def process_rgb(self, planes, fmt: int, out_format: Optional[int] = None):
        """Host planes of an RGB format in (``host_frame``'s arrays: ONE array for a packed format, ``[r, g, b]`` for a
        planar one -- a single array may be passed bare), host planes out.  ``out_format`` (default: ``fmt``): an RGB
        format or FMT_BGRX.  Returns the ``[4H, 4W, ...]`` array of a packed format (FMT_BGRX included), the tuple
        ``(r, g, b)`` of a planar one."""
        out_format = fmt if out_format is None else out_format
        planes = [planes] if isinstance(planes, np.ndarray) else list(planes)
        ow, oh = self.frame_output_size()
        if out_format == FMT_BGRX:
            res = [np.empty((oh, ow, 4), np.uint8)]
        elif out_format in _FMT_RGB:
            samples, dt = _FMT_RGB[out_format]
            res = [np.empty((oh, ow, samples), dt)] if samples else [np.empty((oh, ow), dt) for _ in range(3)]
        elif out_format in (FMT_X2RGB10, FMT_X2BGR10):
            res = [np.empty((oh, ow), np.uint32)]
        else:
            raise ValueError("process_rgb: out_format must be FMT_BGRX or an RGB format")
        self.process_frame(host_frame(fmt, planes), host_frame(out_format, res))
        return res[0] if len(res) == 1 else tuple(res)

    def device_image(self, ptr: int, width: int, height: int,
                     stride: Optional[int] = None) -> JuImage:
        return JuImage(ptr, LOC_DEVICE, width * 4 if stride is None else stride,
                       width, height)

    # -- introspection -------------------------------------------------------
    def read_tensor(self, name: str) -> np.ndarray:
        n = C.c_size_t()
        read = _hook(self._lib, "ju_read_tensor")
        _check(self._lib, read(self._h, name.encode(), None, 0, C.byref(n)))
        arr = np.empty(n.value, np.float32)
        _check(self._lib, read(self._h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.size, C.byref(n)))
        return arr

    def plan_report(self) -> list:
        """``ju_plan_report`` (test flavour): the launch plans this runtime's flow-net launchers really used, one
        dict per distinct launch -- ``kernel`` plus the line's fields as integers (``heights``: a tuple)."""
        report = _hook(self._lib, "ju_plan_report")
        n = C.c_size_t()
        _check(self._lib, report(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        _check(self._lib, report(self._h, buf, n.value + 1, C.byref(n)))
        plans = []
        for line in buf.value.decode().splitlines():
            kernel, *fields = line.split()
            d = {"kernel": kernel}
            for f in fields:
                k, v = f.split("=")
                d[k] = tuple(int(x) for x in v.split(",")) if k == "heights" else int(v)
            plans.append(d)
        return plans

    @property
    def recurrent(self) -> bool:
        """False for a flow-free model (flow_arch "none", ``model_file.remove_flow``): no state,
        every frame is upscaled on its own and ``reset`` does nothing."""
        return self.stat("recurrent") != 0

    @property
    def output(self) -> str:
        """What the frames show: ``"frame"``, the generator's frame, or ``"pre_warp"``, the warped previous
        frame of an output_flow model (``model_file.output_flow``).  Fixed by the model file."""
        return {0: "frame", 1: "pre_warp"}[int(self.stat("output_select"))]

    def stat(self, key: str) -> float:
        """``ju_get_stat``: "graph_replays", "eager_runs", "direct_graphs",
        "resident_tower", "resident_flow", "launches_per_frame", "recurrent", "output_select", "lookahead_frames",
        "lookahead_host_frames", "lookahead_yuv_frames", "source_scaled", "source_mask", "source_stage_frames",
        "output_scaled", "source_filter", "output_filter", "scene_mode", "scene_frames", "scene_cuts", "scene_lookahead",
        "scene_pass_frames", "stage_lookahead", "lookahead_staged_frames", "group_frames", "group_yuv_frames",
        "scene_group", "scene_group_frames", "stage_group", "group_staged_frames", "alpha_mode", "alpha_filter",
        "alpha_frames", "alpha_lookahead", "lookahead_alpha_frames", "alpha_group", "group_alpha_frames"."""
        v = C.c_double()
        _check(self._lib, self._lib.ju_get_stat(self._h, key.encode(), C.byref(v)))
        return v.value

    def time_steps(self, tag: str, iters: int) -> Tuple[float, int, float]:
        """(ms per launch, launches per repetition, FLOPs per repetition)."""
        ms, n, fl = C.c_double(), C.c_int(), C.c_double()
        _check(self._lib, _hook(self._lib, "ju_time_steps")(
            self._h, tag.encode(), iters, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """``ju_comm_unique_id``: the RCCL communicator id rank 0 hands to the other ranks."""
    lib = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib, lib.ju_comm_unique_id(buf))
    return buf.raw


class Comm:
    """``ju_comm``: the C layer's RCCL communicator (one rank per GPU).  Its one job is the
    start-up broadcast of the model container (BASELINE.json config 4)."""

    def __init__(self, unique_id: bytes, rank: int, world_size: int, device: int):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be COMM_ID_BYTES long")
        self._lib = load_library()
        self._h = C.c_void_p()
        self.rank, self.world_size = rank, world_size
        _check(self._lib, self._lib.ju_comm_create(unique_id, rank, world_size, device, C.byref(self._h)))

    def broadcast(self, blob: Optional[bytes], size: int, root: int = 0) -> bytes:
        """Every rank passes ``size``; ``root`` also the bytes.  Returns the bytes."""
        buf = C.create_string_buffer(bytes(blob), size) if self.rank == root else C.create_string_buffer(size)
        _check(self._lib, self._lib.ju_comm_broadcast(self._h, buf, size, root))
        return buf.raw

    def allreduce_max(self, value: float) -> float:
        v = C.c_double(value)
        _check(self._lib, self._lib.ju_comm_allreduce_max(self._h, C.byref(v)))
        return v.value

    def count(self) -> int:
        n = C.c_int()
        _check(self._lib, self._lib.ju_comm_count(self._h, C.byref(n)))
        return n.value

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ju_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass


def process_group(runtimes, inputs, outputs) -> None:
    """``ju_process_group``: one frame for each runtime in one synchronous call -- the bytes of ``runtimes[i].process(
    inputs[i], outputs[i])`` in list order, the flow nets of the frames computed in shared passes (``runtimes[0]``
    leads).  The runtimes must be distinct, on one device, built from the same model bytes with the same dtype, and go
    through one library.  Unequal lists and items that are not :class:`Runtime` raise before any native call."""
    runtimes, inputs, outputs = list(runtimes), list(inputs), list(outputs)
    n = len(runtimes)
    if len(inputs) != n or len(outputs) != n:
        raise ValueError("process_group: as many inputs and outputs as runtimes")
    if not all(isinstance(rt, Runtime) for rt in runtimes):
        raise TypeError("process_group: every member must be a Runtime")
    if n == 0:
        return
    lib = runtimes[0]._lib
    if any(rt._lib is not lib for rt in runtimes):
        raise ValueError("process_group: the runtimes were created through different libraries")
    hs = (C.c_void_p * n)(*[rt._h.value for rt in runtimes])
    ins, outs = (JuImage * n)(*inputs), (JuImage * n)(*outputs)
    _check(lib, lib.ju_process_group(hs, ins, outs, n))


def process_group_frames(runtimes, inputs, outputs) -> None:
    """``ju_process_group_frames``: :func:`process_group` on :class:`JuFrame` frames of any format -- the bytes of
    ``runtimes[i].process_frame(inputs[i], outputs[i])`` in list order; formats, colour spaces, locations and strides
    are independent per member and side.  Unequal lists and items that are not :class:`Runtime` raise before any
    native call."""
    runtimes, inputs, outputs = list(runtimes), list(inputs), list(outputs)
    n = len(runtimes)
    if len(inputs) != n or len(outputs) != n:
        raise ValueError("process_group_frames: as many inputs and outputs as runtimes")
    if not all(isinstance(rt, Runtime) for rt in runtimes):
        raise TypeError("process_group_frames: every member must be a Runtime")
    if n == 0:
        return
    lib = runtimes[0]._lib
    if any(rt._lib is not lib for rt in runtimes):
        raise ValueError("process_group_frames: the runtimes were created through different libraries")
    hs = (C.c_void_p * n)(*[rt._h.value for rt in runtimes])
    ins, outs = (JuFrame * n)(*inputs), (JuFrame * n)(*outputs)
    _check(lib, lib.ju_process_group_frames(hs, ins, outs, n))


class TiledRuntime:
    """``ju_tiled``: frames of ``src_width x src_height`` -- larger than the model -- upscaled tile by tile, the tiles
    blended across their seams on the GPU (docs/tiled.md).  ``model``: the bytes of a .jupw file (or its path);
    ``overlap``: source pixels neighbouring tiles share at least, ``0 .. min(W, H) // 4`` for a model of ``W x H``."""

    def __init__(self, model, device: int = 0, dtype: int = DTYPE_DEFAULT, src_width: int = 0, src_height: int = 0,
                 overlap: int = 16, hooks: Optional[bool] = None):
        self._lib = load_library(hooks)
        self._h = C.c_void_p()
        if not isinstance(model, (bytes, bytearray, memoryview)):
            with open(model, "rb") as f:
                model = f.read()
        buf = bytes(model)
        _check(self._lib, self._lib.ju_tiled_create_from_memory(device, buf, len(buf), dtype, int(src_width), int(src_height),
                                                                int(overlap), C.byref(self._h)))
        self.device = device
        i = self.info()
        self.src_width, self.src_height, self.out_width, self.out_height = (i["src_width"], i["src_height"],
                                                                            i["out_width"], i["out_height"])

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ju_tiled_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def process(self, inp: JuImage, out: JuImage) -> None:
        """``ju_tiled_process``: one frame on two BGRX image descriptors, host or device (synchronous)."""
        _check(self._lib, self._lib.ju_tiled_process(self._h, C.byref(inp), C.byref(out)))

    def process_frame(self, inp: JuFrame, out: JuFrame) -> None:
        """``ju_tiled_process_frame``: one frame on frames of any format, host or device (synchronous)."""
        _check(self._lib, self._lib.ju_tiled_process_frame(self._h, C.byref(inp), C.byref(out)))

    # -- look-ahead passes (docs/tiled.md "Look-ahead passes") ----------
    def process_batch(self, inputs, outputs) -> None:
        """``ju_tiled_process_batch``: consecutive frames of the tiled stream as BGRX image descriptors in one synchronous
        call (every input must hold its pixels now); the bytes and the state of ``process`` called frame by frame."""
        inputs, outputs = list(inputs), list(outputs)
        n = len(inputs)
        if len(outputs) != n:
            raise ValueError("process_batch: as many outputs as inputs")
        ins, outs = (JuImage * n)(*inputs), (JuImage * n)(*outputs)
        _check(self._lib, self._lib.ju_tiled_process_batch(self._h, ins, outs, n))

    def process_frames(self, inputs, outputs) -> None:
        """``ju_tiled_process_frames``: consecutive frames of the tiled stream, of any format, host or device, in one
        synchronous call (every input must hold its pixels now); the bytes and the state of ``process_frame`` called
        frame by frame.  Passes of at most :meth:`set_lookahead` frames: one split launch per pass, a host output copied
        out under the next frame's group passes.  Lists of unequal length raise before any native call."""
        inputs, outputs = list(inputs), list(outputs)
        n = len(inputs)
        if len(outputs) != n:
            raise ValueError("process_frames: as many outputs as inputs")
        ins, outs = (JuFrame * n)(*inputs), (JuFrame * n)(*outputs)
        _check(self._lib, self._lib.ju_tiled_process_frames(self._h, ins, outs, n))

    def set_lookahead(self, frames: int) -> None:
        """``ju_tiled_set_lookahead``: frames per look-ahead pass, 1 .. 8, clamped (1 = every frame as
        ``process_frame``).  ``reset`` keeps it."""
        _check(self._lib, self._lib.ju_tiled_set_lookahead(self._h, int(frames)))

    def run(self, frame_bgrx: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host frames: ``[src_height, src_width, 4]`` uint8 BGRX in, ``[4 src_height, 4 src_width, 4]`` out -- or
        :meth:`frame_output_size` while an output size is set.  Any row stride (also negative, i.e. a ``[::-1]`` view) is
        passed through."""
        if frame_bgrx.dtype != np.uint8 or frame_bgrx.ndim != 3 or frame_bgrx.shape[2] != 4:
            raise ValueError("expected a [H, W, 4] uint8 BGRX frame")
        if frame_bgrx.strides[2] != 1 or frame_bgrx.strides[1] != 4:
            frame_bgrx = np.ascontiguousarray(frame_bgrx)
        if out is None:
            ow, oh = self.frame_output_size()
            out = np.empty((oh, ow, 4), np.uint8)
        if out.strides[2] != 1 or out.strides[1] != 4:
            raise ValueError("output must have contiguous pixels")
        self.process(host_image(frame_bgrx), host_image(out))
        return out

    def reset(self) -> None:
        """``ju_tiled_reset``: zeroes every tile's recurrent state (keeps ``set_deep_from_state``)."""
        _check(self._lib, self._lib.ju_tiled_reset(self._h))

    def set_deep_from_state(self, on) -> None:
        """``ju_tiled_set_deep_from_state``: 1 = a deep output format (P010, BGRX64, RGBPH, ...) is encoded from the blend
        of the tiles' f16 states, where the model's state is its frame in float (``stat("hbd_from_state")``); 0, the
        default, = from the blended 8-bit frame (docs/tiled.md "Deep outputs").  Another value is refused."""
        _check(self._lib, self._lib.ju_tiled_set_deep_from_state(self._h, int(on)))

    # -- an output size (docs/tiled.md "An output size") ----------
    def set_output_size(self, width: int, height: int, filter: int = SCALE_TRIANGLE) -> None:
        """``ju_tiled_set_output_size``: output frames are ``width x height`` from now on, the blended frame scaled by
        ``filter`` (``SCALE_TRIANGLE``, ``SCALE_CATMULL_ROM`` or ``SCALE_MITCHELL``) inside the blend's launch; ``(0, 0)``
        turns it off.  The limits raise ``ValueError`` with the C layer's message before any native call.
        ``out_width`` / ``out_height`` stay the blended size."""
        width, height, filter = int(width), int(height), int(filter)
        off = (width, height) == (0, 0)
        problem = tiled_output_size_problem(self.out_width if off else width, self.out_height if off else height,
                                            self.src_width, self.src_height, filter)
        if problem:
            raise ValueError("ju_tiled_set_output_size: " + problem)
        problem = tiled_alpha_problem(*self.get_alpha(), self.src_width, self.src_height, width, height)
        if problem:                                                       # (alpha from the source: both settings stay)
            raise ValueError("ju_tiled_set_output_size: " + problem)
        _check(self._lib, self._lib.ju_tiled_set_output_size(self._h, width, height, filter))

    def get_output_size(self) -> Tuple[int, int]:
        """``ju_tiled_get_output_size``: ``(width, height)``, ``(0, 0)`` while no output size is set."""
        w, h = C.c_size_t(), C.c_size_t()
        _check(self._lib, self._lib.ju_tiled_get_output_size(self._h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def frame_output_size(self) -> Tuple[int, int]:
        """``(width, height)`` of the frames the object hands out now: the output size set, else the blended size."""
        w, h = self.get_output_size()
        return (w, h) if w else (self.out_width, self.out_height)

    # -- the alpha channel (docs/tiled.md "Alpha") ----------
    def set_alpha(self, mode: int, filter: int = SCALE_TRIANGLE) -> None:
        """``ju_tiled_set_alpha``: :meth:`Runtime.set_alpha` for tiled frames -- ``ALPHA_SOURCE`` scales the input frame's
        alpha by ``filter`` from the tiled source size straight to :meth:`frame_output_size`, in one launch behind the
        stitch; the tiles never see it.  An unknown mode or filter and sizes beyond the alpha scaler raise ``ValueError``
        with the C layer's message before any native call; the setting stays as it was.  ``reset`` keeps it."""
        mode, filter = int(mode), int(filter)
        problem = tiled_alpha_problem(mode, filter, self.src_width, self.src_height, *self.get_output_size())
        if problem:
            raise ValueError("ju_tiled_set_alpha: " + problem)
        _check(self._lib, self._lib.ju_tiled_set_alpha(self._h, mode, filter))

    def get_alpha(self) -> Tuple[int, int]:
        """``ju_tiled_get_alpha``: ``(mode, filter)`` as set; ``(ALPHA_ZERO, SCALE_TRIANGLE)`` on a fresh object."""
        mode, filter = C.c_int(), C.c_int()
        _check(self._lib, self._lib.ju_tiled_get_alpha(self._h, C.byref(mode), C.byref(filter)))
        return mode.value, filter.value

    # -- a source mask (docs/tiled.md "A mask") ----------
    def set_source_mask(self, mask) -> None:
        """``ju_tiled_set_source_mask``: ``mask`` is a ``[MH, MW, 4]`` uint8 BGRX array of any size, a :class:`JuImage`
        (host or device), or ``None`` to remove the mask, as :meth:`Runtime.set_source_mask` takes it.  From now on the
        source frame is drawn back over the blended frame through it, inside the stitch's launch.  The object copies it."""
        if mask is None:
            _check(self._lib, self._lib.ju_tiled_set_source_mask(self._h, None))
            return
        if not isinstance(mask, JuImage):
            if mask.dtype != np.uint8 or mask.ndim != 3 or mask.shape[2] != 4 or mask.strides[2] != 1 or mask.strides[1] != 4:
                raise ValueError("expected a [H, W, 4] uint8 BGRX mask with contiguous pixels")
            mask = host_image(mask)
        _check(self._lib, self._lib.ju_tiled_set_source_mask(self._h, C.byref(mask)))

    # -- the scene detector of the tiled stream (docs/tiled.md "Scene cuts") ----------
    def set_scene_detect(self, mode: int, threshold_milli: int = 10000) -> None:
        """``ju_tiled_set_scene_detect``: ``SCENE_OFF``, ``SCENE_REPORT`` (record cuts) or ``SCENE_RESET`` (and restart
        every tile's recurrence at them, on the GPU).  ONE detector on the source frame; ``threshold_milli`` as for
        :meth:`Runtime.set_scene_detect`.  An unknown mode or a threshold out of range raises
        :class:`JoshUpscaleError` with the C layer's message."""
        mode, threshold_milli = int(mode), int(threshold_milli)
        if not 0 <= threshold_milli < 2 ** 32:
            raise ValueError("threshold_milli must fit 32 bits")
        _check(self._lib, self._lib.ju_tiled_set_scene_detect(self._h, mode, threshold_milli))

    def get_scene_detect(self) -> Tuple[int, int]:
        """``ju_tiled_get_scene_detect``: ``(mode, threshold_milli)``; the threshold is 0 while the mode is off."""
        mode, thr = C.c_int(), C.c_uint32()
        _check(self._lib, self._lib.ju_tiled_get_scene_detect(self._h, C.byref(mode), C.byref(thr)))
        return mode.value, thr.value

    def scene_info(self, count: int = SCENE_RING) -> list:
        """``ju_tiled_get_scene_info``: the most recent ``min(count, 64, steps seen)`` decisions of the tiled stream,
        oldest first, as dicts ``{"step", "sad", "score", "cut"}``."""
        count = max(0, int(count))
        recs = (JuSceneInfo * max(count, 1))()
        got = C.c_int()
        _check(self._lib, self._lib.ju_tiled_get_scene_info(self._h, recs, count, C.byref(got)))
        return [{"step": r.step, "sad": r.sad, "score": r.score, "cut": int(r.cut)} for r in recs[:got.value]]

    def info(self) -> dict:
        """``ju_tiled_get_info`` as a dict of the struct's fields."""
        i = JuTiledInfo()
        _check(self._lib, self._lib.ju_tiled_get_info(self._h, C.byref(i)))
        return {name: int(getattr(i, name)) for name, _ in JuTiledInfo._fields_}

    def tile(self, index: int) -> Tuple[int, int]:
        """``ju_tiled_get_tile``: the origin ``(x, y)`` of a tile (row-major over the tile grid) in source pixels."""
        x, y = C.c_size_t(), C.c_size_t()
        _check(self._lib, self._lib.ju_tiled_get_tile(self._h, int(index), C.byref(x), C.byref(y)))
        return x.value, y.value

    def stat(self, key: str) -> float:
        """``ju_tiled_get_stat``: "tiles", "frames", "group_frames" (summed over the tiles), "deep_from_state" (the
        setting), "hbd_from_state" (the model's property), "deep_state_frames" (frames blended from the states),
        "lookahead", "pass_calls", "pass_frames", "pass_split_launches" and "pass_overlapped_copies" (``process_frames``),
        "scene_mode", "scene_frames" and "scene_cuts" (the tiled stream's detector; the counters are cumulative),
        "output_scaled", "output_filter" and "output_scaled_frames" (``set_output_size``; frames that took a fused
        blend-and-scale kernel), "source_mask", "source_mask_frames" and "mask_box_x0" .. "mask_box_y1"
        (``set_source_mask``; the box in blended coordinates)."""
        v = C.c_double()
        _check(self._lib, self._lib.ju_tiled_get_stat(self._h, key.encode(), C.byref(v)))
        return v.value


def gl_image(texture: int, output: bool) -> JuImage:
    """``ju_get_gl_image`` (``getGLImage``, reference core.h:61-62): a registered OpenGL
    texture as a GRAPHICS_RESOURCE image.  Release with :func:`release_gl_image`."""
    lib = load_library()
    img = JuImage()
    _check(lib, lib.ju_get_gl_image(texture, 1 if output else 0, C.byref(img)))
    return img


def release_gl_image(img: JuImage) -> None:
    load_library().ju_release_gl_image(C.byref(img))


def host_image(arr: np.ndarray) -> JuImage:
    """Describe a ``[H, W, 4]`` uint8 numpy array (any row stride) as an image."""
    return JuImage(arr.ctypes.data, LOC_CPU, arr.strides[0], arr.shape[1], arr.shape[0])


def _frame(fmt: int, colorspace: int, location: int, width: int, height: int, ptrs, strides) -> JuFrame:
    f = JuFrame()
    f.format, f.colorspace, f.location, f.width, f.height = fmt, colorspace, location, width, height
    for k, (p, s) in enumerate(zip(ptrs, strides)):
        f.planes[k], f.strides[k] = p, s
    return f


def host_frame(fmt: int, planes, colorspace: int = CS_BT709_LIMITED, width: Optional[int] = None) -> JuFrame:
    """Describe numpy planes as a host frame.  FMT_BGRX: ``[bgrx [H, W, 4]]``; FMT_I420: ``[y [H, W], u, v
    [H/2, W/2]]``; FMT_NV12: ``[y [H, W], uv [H/2, W]]``; FMT_I010 / FMT_P010: the same shapes as ``uint16``.
    FMT_YUY2 / FMT_UYVY: ONE ``[H, 2W]`` uint8 array; FMT_I422 / FMT_I210: ``[y [H, W], u, v [H, W/2]]``; FMT_P210:
    ``[y [H, W], uv [H, W]]``; FMT_I444 / FMT_I410: ``[y, u, v [H, W]]`` (the 10-bit formats ``uint16``).
    The RGB formats: FMT_BGR24 / FMT_RGB24 ONE ``[H, W, 3]`` uint8 array, FMT_RGBX ``[H, W, 4]`` uint8, FMT_BGRX64
    ``[H, W, 4]`` uint16, FMT_BGR96F ``[H, W, 3]`` float32; FMT_RGBP8 / FMT_RGBP10 / FMT_RGBP16 / FMT_RGBPH / FMT_RGBPS
    three ``[H, W]`` arrays ``[r, g, b]`` of uint8 / uint16 / uint16 / float16 / float32 (``colorspace`` is ignored).
    Packed 10-bit, ONE array: FMT_Y410 / FMT_X2RGB10 / FMT_X2BGR10 ``[H, W]`` uint32, FMT_Y210 ``[H, 2W]`` uint16, FMT_V210
    ``[H, 4 ceil(W / 6)]`` uint32 or a wider one whose extra columns are padding -- the array cannot tell W, so
    ``width=W`` is required for FMT_V210 (and only there).  Any
    row stride (a ``[::-1]`` view is bottom-up; the frame's strides are the arrays' byte strides); the columns must be
    contiguous.  The arrays must outlive the call."""
    if fmt in _FMT_PACKED10:
        planes = list(planes)
        if len(planes) != 1:
            raise ValueError("a packed 10-bit frame is one array")
        y = planes[0]
        dt = np.dtype(np.uint16 if fmt == FMT_Y210 else np.uint32)
        if y.dtype != dt or y.ndim != 2 or y.strides[1] != dt.itemsize:
            raise ValueError(f"a packed 10-bit frame of this format is one 2-D {dt.name} array with contiguous columns")
        if fmt == FMT_V210:
            if width is None:
                raise ValueError("a V210 frame needs width=W: its array holds whole groups of six pixels")
            if width < 2 or width % 2 or y.shape[1] < v210_row_words(width):
                raise ValueError("a V210 frame is [H, 4 ceil(W / 6)] uint32 (or wider: padding), W even")
        elif fmt == FMT_Y210:
            if y.shape[1] == 0 or y.shape[1] % 4:
                raise ValueError("a Y210 frame is one [H, 2W] uint16 array, W even")
            width = y.shape[1] // 2
        else:
            width = y.shape[1]
        return _frame(fmt, colorspace, LOC_CPU, width, y.shape[0], [y.ctypes.data], [y.strides[0]])
    if fmt in _FMT_RGB:
        samples, dt = _FMT_RGB[fmt]
        planes = list(planes)
        if len(planes) != (1 if samples else 3):
            raise ValueError("a packed RGB frame is one array, a planar one three arrays [r, g, b]")
        y = planes[0]
        for p in planes:
            if p.dtype != np.dtype(dt):
                raise ValueError(f"planes of this format must be {np.dtype(dt).name}")
            if p.shape != y.shape or p.ndim != (3 if samples else 2) or (samples and p.shape[2] != samples):
                raise ValueError("a packed RGB frame is [H, W, samples], a planar one three equal [H, W] arrays")
            if p.strides[1] != p.itemsize * max(samples, 1) or (samples and p.strides[2] != p.itemsize):
                raise ValueError("planes need contiguous columns")
        return _frame(fmt, colorspace, LOC_CPU, y.shape[1], y.shape[0], [p.ctypes.data for p in planes],
                      [p.strides[0] for p in planes])
    deep = fmt in _FMT_DEEP
    for p in planes:
        if p.dtype != (np.uint16 if deep else np.uint8) or p.strides[1] != (4 if fmt == FMT_BGRX else (2 if deep else 1)):
            raise ValueError("planes must be uint8 (the 10-bit formats: uint16) with contiguous columns")
    y = planes[0]
    if fmt in _FMT_PACKED and (len(planes) != 1 or y.ndim != 2 or y.shape[1] % 4):
        raise ValueError("a packed 4:2:2 frame is one [H, 2W] uint8 array, W even")
    width = y.shape[1] // 2 if fmt in _FMT_PACKED else y.shape[1]
    return _frame(fmt, colorspace, LOC_CPU, width, y.shape[0], [p.ctypes.data for p in planes],
                  [p.strides[0] for p in planes])


def device_frame(fmt: int, width: int, height: int, ptrs, strides=None,
                 colorspace: int = CS_BT709_LIMITED) -> JuFrame:
    """A device frame from raw device pointers (or torch tensors: their ``data_ptr()``); ``strides`` default to
    dense rows in bytes (BGRX 4W, Y W, I420 / I422 chroma W/2, NV12 chroma W, I444 chroma W, YUY2 / UYVY 2W; the 10-bit
    formats twice that; RGB: W x the bytes of a packed pixel, or of a planar sample; packed 10-bit: 4W, FMT_V210
    16 ceil(W / 6))."""
    ptrs = [p.data_ptr() if hasattr(p, "data_ptr") else int(p) for p in ptrs]
    if strides is None and fmt in _FMT_RGB:
        samples, dt = _FMT_RGB[fmt]
        strides = [width * np.dtype(dt).itemsize * max(samples, 1)] * (1 if samples else 3)
    if strides is None and fmt in _FMT_PACKED10:
        strides = [4 * v210_row_words(width) if fmt == FMT_V210 else 4 * width]
    if strides is None:
        strides = {FMT_BGRX: [4 * width], FMT_I420: [width, width // 2, width // 2],
                   FMT_NV12: [width, width], FMT_P010: [2 * width, 2 * width],
                   FMT_I010: [2 * width, width, width],
                   FMT_YUY2: [2 * width], FMT_UYVY: [2 * width], FMT_I422: [width, width // 2, width // 2],
                   FMT_P210: [2 * width, 2 * width], FMT_I210: [2 * width, width, width],
                   FMT_I444: [width, width, width], FMT_I410: [2 * width, 2 * width, 2 * width]}[fmt]
    return _frame(fmt, colorspace, LOC_DEVICE, width, height, ptrs, strides)


class Session:
    """Recurrent driver with the reference scripts' call shape
    (scripts/inference/onnx/inference.py:46-94): ``Session(model).run(image)``.
    Accepts ``[H, W, 3]`` BGR (as ``cv2.imread`` yields) or ``[H, W, 4]`` BGRX and
    returns the same number of channels."""

    def __init__(self, model, device: int = 0, dtype: int = DTYPE_DEFAULT, hooks: Optional[bool] = None):
        self.runtime = Runtime(model, device, dtype, hooks)

    def run(self, image: np.ndarray) -> np.ndarray:
        if image.ndim == 4 and image.shape[0] == 1:
            image = image[0]
        ch = image.shape[2]
        if ch == 3:
            frame = np.empty(image.shape[:2] + (4,), np.uint8)
            frame[..., :3] = image
            frame[..., 3] = 255
        else:
            frame = image
        out = self.runtime.process_image(np.ascontiguousarray(frame, dtype=np.uint8))
        return out[..., :3].copy() if ch == 3 else out

    def reset(self) -> None:
        self.runtime.reset()

    def set_source_size(self, width: int, height: int, filter: int = SCALE_TRIANGLE) -> None:
        """``run`` takes ``width x height`` images from now on (``Runtime.set_source_size``)."""
        self.runtime.set_source_size(width, height, filter)

    def get_source_size(self) -> Tuple[int, int]:
        return self.runtime.get_source_size()

    def set_source_mask(self, mask) -> None:
        """The source shows through ``mask`` in every frame ``run`` returns (``Runtime.set_source_mask``)."""
        self.runtime.set_source_mask(mask)

    def set_output_size(self, width: int, height: int, filter: int = SCALE_TRIANGLE) -> None:
        """``run`` returns ``width x height`` images from now on (``Runtime.set_output_size``)."""
        self.runtime.set_output_size(width, height, filter)

    def get_output_size(self) -> Tuple[int, int]:
        return self.runtime.get_output_size()

    def set_alpha(self, mode: int, filter: int = SCALE_TRIANGLE) -> None:
        """The alpha of the ``[H, W, 4]`` images ``run`` returns (``Runtime.set_alpha``)."""
        self.runtime.set_alpha(mode, filter)

    def get_alpha(self) -> Tuple[int, int]:
        return self.runtime.get_alpha()
