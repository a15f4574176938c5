"""Shared pieces of the output_flow tests (test infrastructure): the byte an output_flow model writes, stated on the
oracle's pre_warp and on the engine's own generator input."""
import numpy as np

from helpers import M, O, gen_in_to_reference, oracle_config


def expected_frame(pre_warp: np.ndarray) -> np.ndarray:
    """BGRX frame of a float pre_warp [4H, 4W, 3]: trunc((p + 0.5) * 255) with an explicit clip to 0..255
    (O.postprocess alone wraps out-of-range values), X = 0."""
    b = np.clip(np.trunc((np.asarray(pre_warp, np.float64) + 0.5) * 255.0), 0, 255).astype(np.uint8)
    return O.bgr_to_bgrx(b)


def oracle_frames(cfg: M.ModelConfig, wts, frames, fp8_tower: bool = False):
    """The float64 oracle over a clip: (the plain model's frames, the variant's expected frames, pre_warp tensors).
    The oracle steps the plain model; the variant only shows another tensor of the same step."""
    sess = O.Session(wts, oracle_config(dataclass_plain(cfg), fp8_tower=fp8_tower))
    plain, variant, pre = [], [], []
    for f in frames:
        plain.append(sess.run(f).copy())
        pre.append(np.array(sess.last.pre_warp, np.float64))
        variant.append(expected_frame(pre[-1]))
    return plain, variant, pre


def dataclass_plain(cfg: M.ModelConfig) -> M.ModelConfig:
    import dataclasses
    return dataclasses.replace(cfg, output="frame")


def frame_of_gen_in(gen_in: np.ndarray, h: int, w: int) -> np.ndarray:
    """The exact definition: the frame from the engine's generator-input record as read back (float32 of the
    compute type's values, what the generator reads):  b = trunc(clamp((v + 0.5f) * 255.0f, 0, 255)) in float32."""
    ref = gen_in_to_reference(np.asarray(gen_in, np.float32), h, w)
    hr = ref[..., 3:].reshape(h, w, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(4 * h, 4 * w, 3)
    x = (hr + np.float32(0.5)) * np.float32(255.0)
    assert x.dtype == np.float32
    return O.bgr_to_bgrx(np.clip(x, np.float32(0.0), np.float32(255.0)).astype(np.uint8))
