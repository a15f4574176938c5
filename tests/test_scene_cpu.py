"""The scene detector without a GPU: the Python definition (tests/scene_reference.py; docs/scene_detect.md) on the known
clip and at its limits; the refusals' message in C and in the definition; the new entry points; NULL runtimes."""

import ctypes as C
import os
import re

import numpy as np

import scene_reference as S
from helpers import M
from joshupscale_amd import runtime as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 30, 48
N = 3 * H * W
# D_t / N of the known clip, to the digits the definition was written down with (docs/scene_detect.md)
KNOWN_SCORES = [0, 0, 0.02, 0.10, 24.53, 20.23, 0.01, 24.39, 18.73, 0.03, 123.4, 0, 142.1]


def known():
    clip = S.known_clip(M.synthetic_frames, H, W)
    return clip, S.run(clip, S.KNOWN_THRESHOLD)


def test_the_known_clip_cuts_at_4_7_10_and_12():
    clip, recs = known()
    assert clip.shape == (13, H, W, 4) and [r["step"] for r in recs] == list(range(13))
    for r, want in zip(recs, KNOWN_SCORES):
        digits = 1 if want > 100 else 2
        assert round(r["score"] / N, digits) == want, (r, want)
    assert S.cuts(recs) == S.KNOWN_CUTS == [4, 7, 10, 12]
    flagged = [r["score"] for r in recs if r["cut"]]
    unflagged = [r["score"] for r in recs if not r["cut"]]
    assert 1000 * min(flagged) > S.KNOWN_THRESHOLD * N > 1000 * max(unflagged)
    # the frame behind each cut (a large S again, but about the S before it) and the second white frame do not cut
    assert [recs[t]["cut"] for t in (5, 8, 11)] == [0, 0, 0]
    assert recs[5]["sad"] > recs[4]["score"] // 2 and recs[11]["sad"] == 0 and recs[11]["score"] == 0
    # frames 0 and 1: no score by the no-predecessor rule, though frame 1 has a sum
    assert recs[0]["sad"] == 0 and recs[1]["sad"] > 0 and recs[0]["score"] == recs[1]["score"] == 0


def test_a_restart_forgets_the_predecessors_and_keeps_the_step_count():
    clip, recs = known()
    det = S.Detector(S.KNOWN_THRESHOLD)
    got = [det.feed(f) for f in clip[:4]]
    det.restart()                                       # (ju_reset in front of frame 4: the cut there is not seen ...)
    got += [det.feed(f) for f in clip[4:]]
    assert [r["step"] for r in got] == list(range(13))
    assert got[:4] == recs[:4] and got[6:] == recs[6:]  # (... and from its third frame on the detector is the same)
    assert [got[4]["cut"], got[5]["cut"], got[4]["sad"]] == [0, 0, 0] and got[5]["sad"] == recs[5]["sad"]


def test_static_clips_never_cut():
    rng = np.random.default_rng(1)
    for frame in (np.zeros((H, W, 4), np.uint8), np.full((H, W, 4), 255, np.uint8),
                  rng.integers(0, 256, (H, W, 4), dtype=np.uint8)):
        recs = S.run([frame] * 6, S.THRESHOLD_MIN)      # (the lowest threshold there is)
        assert S.cuts(recs) == [] and all(r["sad"] == 0 and r["score"] == 0 for r in recs)


def test_equality_cuts_and_one_less_does_not():
    n = 3 * 2 * 2                                       # a 2 x 2 frame; D = 30, so threshold N = 1000 D at 2500
    a = np.zeros((2, 2, 4), np.uint8)
    b = a.copy()
    b[0, 0, :3] = 10                                    # S = 30
    for thr, want in ((2500, 1), (2501, 0), (2499, 1)):
        recs = S.run([a, a, b], thr)
        assert recs[2]["sad"] == 30 and recs[2]["score"] == 30 and 1000 * 30 == 2500 * n
        assert recs[2]["cut"] == want, thr
    assert S.decide(30, 0, 2, n, 2500) == (30, 1) and S.decide(29, 0, 2, n, 2500) == (29, 0)
    assert S.decide(30, 0, 1, n, 1) == (0, 0)           # (no t-2: no score)
    # the score is the smaller of S and its change
    assert S.decide(100, 90, 2, n, 1)[0] == 10 and S.decide(100, 250, 2, n, 1)[0] == 100


def test_a_2400_square_black_white_pair_exceeds_32_bits():
    black = np.zeros((2400, 2400, 4), np.uint8)
    white = np.full((2400, 2400, 4), 255, np.uint8)
    s = S.sad(white, black)
    assert s == 3 * 2400 * 2400 * 255 and s > 2 ** 32
    recs = S.run([black, black, white], S.THRESHOLD_MAX)
    assert recs[2]["sad"] == s and recs[2]["cut"] == 1   # 1000 D == 255000 N: the highest threshold still cuts here


def test_the_x_byte_never_matters():
    clip, recs = known()
    other = clip.copy()
    other[..., 3] = np.random.default_rng(2).integers(0, 256, other.shape[:3], dtype=np.uint8)
    assert S.run(other, S.KNOWN_THRESHOLD) == recs


def c_refusal(lib, mode, thr):
    rc = lib.ju_debug_scene(2, None, 0, 0, 0, None, None, mode, thr, 0, None, None, 0, None, 0)
    return rc, lib.ju_last_error().decode() if rc else ""


def test_the_refusals_and_their_message_match_between_c_and_the_definition(hip_library):
    for mode, thr in [(0, 0), (0, 10 ** 9), (1, 1), (2, 255000), (1, 10000), (2, 22000)]:
        assert S.problem(mode, thr) == ""
        assert c_refusal(hip_library, mode, thr) == (0, "")
    for mode, thr in [(3, 10000), (-1, 10000), (1, 0), (2, 0), (1, 255001), (2, 2 ** 32 - 1)]:
        text = S.problem(mode, thr)
        assert text
        assert ("mode must be" in text) == (mode not in (0, 1, 2)) and ("threshold_milli must be 1 .. 255000" in text) == (mode in (1, 2))
        assert c_refusal(hip_library, mode, thr) == (1, "std::invalid_argument: ju_set_scene_detect: " + text)


def test_null_runtimes_are_refused_without_a_gpu(hip_library, product_library):
    for lib in (hip_library, product_library):
        mode, thr, got = C.c_int(7), C.c_uint32(7), C.c_int(7)
        recs = (R.JuSceneInfo * 4)()
        assert lib.ju_set_scene_detect(None, R.SCENE_RESET, 10000) == 1          # JU_ERR_INVALID_ARGUMENT
        assert "runtime is NULL" in lib.ju_last_error().decode()
        assert lib.ju_get_scene_info(None, recs, 4, C.byref(got)) == 1 and got.value == 0
        assert "runtime is NULL" in lib.ju_last_error().decode()
        assert lib.ju_get_scene_detect(None, C.byref(mode), C.byref(thr)) == 1


def test_new_entry_points_are_declared_and_exported(hip_library, product_library):
    header = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    test_header = open(os.path.join(ROOT, "include", "joshupscale_amd_test.h")).read()
    for name in ("ju_set_scene_detect", "ju_get_scene_detect", "ju_get_scene_info"):
        assert re.search(r"JU_API\s+int\s+" + name + r"\s*\(", header)
        assert name in R.PRODUCT_SYMBOLS and name not in R.HOOK_SYMBOLS
        assert hasattr(product_library, name) and hasattr(hip_library, name)
    assert re.search(r"JU_API\s+int\s+ju_debug_scene\s*\(", test_header) and "ju_debug_scene" not in header
    assert "ju_debug_scene" in R.HOOK_SYMBOLS and not hasattr(product_library, "ju_debug_scene")
    assert (R.SCENE_OFF, R.SCENE_REPORT, R.SCENE_RESET) == (S.OFF, S.REPORT, S.RESET) == (0, 1, 2)
    for name, value in (("JU_SCENE_OFF", 0), ("JU_SCENE_REPORT", 1), ("JU_SCENE_RESET", 2)):
        assert re.search(name + r"\s*=\s*%d\b" % value, header)
    assert C.sizeof(R.JuSceneInfo) == 32 and R.SCENE_RING == S.RING == 64
    for name in ("set_scene_detect", "get_scene_detect", "scene_info"):
        assert callable(getattr(R.Runtime, name))
