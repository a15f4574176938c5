"""Look-ahead passes of a tiled object without a GPU (docs/tiled.md "Look-ahead passes"): the declared surface, the pass
planner (csrc/tile_pass_plan.h) against its restatement (tests/tiled_pass_reference.py) -- through the no-device hook and
from a stand-alone host program under the address and undefined-behaviour sanitizers -- the properties a plan must have,
and the words of the refusals that precede any device call."""

import ctypes as C
import os
import re
import struct
import subprocess

from helpers import ROOT
from joshupscale_amd import runtime as R
import tiled_pass_reference as P

JU_ERR_INVALID_ARGUMENT = 1
W, H = 48, 30                                    # helpers.small_config()


# ---- the surface -----------------------------------------------------------------------------------------------------------
def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"JU_API\s+[\w\s\*]+?\b(ju_\w+)\s*\(", text))


def test_the_surface_is_declared_and_mirrored():
    text = open(os.path.join(ROOT, "include", "joshupscale_amd.h")).read()
    for name in ("ju_tiled_process_batch", "ju_tiled_process_frames", "ju_tiled_set_lookahead"):
        assert name in declared("joshupscale_amd.h") and name not in declared("joshupscale_amd_test.h")
        assert name in R.PRODUCT_SYMBOLS and name not in R.HOOK_SYMBOLS
    for name in ("ju_debug_tile_split_frames", "ju_debug_tiled_pass_plan"):
        assert name in declared("joshupscale_amd_test.h") and name not in declared("joshupscale_amd.h")
        assert name in R.HOOK_SYMBOLS and name not in R.PRODUCT_SYMBOLS
    assert re.search(r"int ju_tiled_process_batch\(ju_tiled \*tiled, const ju_image \*inputs, const ju_image \*outputs, int count\);", text)
    assert re.search(r"int ju_tiled_process_frames\(ju_tiled \*tiled, const ju_frame \*inputs, const ju_frame \*outputs, int count\);", text)
    assert re.search(r"int ju_tiled_set_lookahead\(ju_tiled \*tiled, int frames\);", text)
    for method in ("process_batch", "process_frames", "set_lookahead"):
        assert callable(getattr(R.TiledRuntime, method))
    at = text.index("JU_API int ju_tiled_process_batch")
    comment = text[text.rindex("/*", 0, at):at]
    for key in ('"lookahead"', '"pass_calls"', '"pass_frames"', '"pass_split_launches"', '"pass_overlapped_copies"'):
        assert key in comment, key
    assert "frame i: ..." in comment and "JU_LOOKAHEAD" in comment
    # the lines that said a tiled object has no look-ahead passes are gone
    assert "Not provided for a tiled object: look-ahead" not in text
    doc = open(os.path.join(ROOT, "docs", "tiled.md")).read()
    assert "## Look-ahead passes" in doc and "ju_tiled_process_frames" in doc and "tile_split_frames_kernel" in doc
    scope = doc[doc.index("## Out of scope"):]
    assert not re.search(r"^- look-ahead passes", scope, re.M | re.I)
    for left_out in ("ju_prepare_", "ju_tiled_enqueue", "plugin surface"):
        assert left_out in scope, left_out
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ju_tiled_process_frames" in integration and "ju_tiled_set_lookahead" in integration
    kernels = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "tile_kernels.hip")).read()
    assert "tile_split_frames_kernel" in kernels and "launchTileSplitFrames" in kernels and "splitLane" in kernels
    body = kernels[kernels.index("__device__ __forceinline__ void splitLane"):kernels.index("---- the split with the tiled stream's scene detector")]
    assert "asm" not in body
    header = open(os.path.join(ROOT, "joshupscale_amd", "csrc", "tile_pass_plan.h")).read()
    assert "hip" not in header.replace("no HIP", "").lower()


# ---- the planner -------------------------------------------------------------------------------------------------------------
def c_plan(lib, count, cap, clash):
    starts = (C.c_int * max(count, 1))(*([-1] * max(count, 1)))
    n = C.c_int(-1)
    rc = lib.ju_debug_tiled_pass_plan(count, cap, P.matrix(count, clash), starts, count, C.byref(n))
    assert rc == 0, lib.ju_last_error()
    return list(starts[:n.value])


def test_the_plans_of_the_header_have_the_properties_of_a_plan(hip_library):
    """What csrc/tile_pass_plan.h gives through the no-device hook, held to the properties themselves (and the restatement
    to the same plans)."""
    seen_lengths = set()
    for count, cap, clash in P.cases():
        starts = c_plan(hip_library, count, cap, clash)
        assert starts == P.plan(count, cap, clash), (count, cap, sorted(clash))
        assert starts == sorted(set(starts)) and (starts[:1] == [0] if count else starts == [])
        ends = starts + [count]
        passes = [(a, b - a) for a, b in zip(ends, ends[1:])]
        assert passes == P.passes(count, cap, clash) and sum(n for _, n in passes) == count
        for at, n in passes:
            assert 1 <= n <= cap
            assert not any((i, j) in clash for j in range(at, at + n) for i in range(at, j))   # no clash inside a pass
            nxt = at + n
            if nxt < count:                                        # greedy: the next frame could not have joined
                assert n == cap or any((i, nxt) in clash for i in range(at, nxt))
            seen_lengths.add(n)
        if not clash:
            assert passes == [(a, min(cap, count - a)) for a in range(0, count, cap)]
    assert seen_lengths == set(range(1, 9))
    assert P.passes(11, 8) == [(0, 8), (8, 3)] and P.passes(11, 3) == [(0, 3), (3, 3), (6, 3), (9, 2)]
    assert P.passes(4, 8, {(1, 2)}) == [(0, 2), (2, 2)]           # outputs[1] over inputs[2]: two passes
    assert [P.clamp_cap(f) for f in (-3, 0, 1, 2, 8, 9, 1 << 30)] == [1, 1, 1, 2, 8, 8, 8]


def test_the_no_device_hook_gives_the_same_plans(hip_library):
    cases = P.cases()
    assert len(cases) > 700 and sum(1 for _, _, clash in cases if clash) > 500
    for count, cap, clash in cases:
        assert c_plan(hip_library, count, cap, clash) == P.plan(count, cap, clash), (count, cap, sorted(clash))
    assert c_plan(hip_library, 5, 0, set()) == [0, 1, 2, 3, 4] and c_plan(hip_library, 5, -7, set()) == [0, 1, 2, 3, 4]
    # a capacity smaller than the plan: the count all the same, the first entries only
    starts, n = (C.c_int * 2)(-1, -1), C.c_int()
    assert hip_library.ju_debug_tiled_pass_plan(9, 2, P.matrix(9, set()), starts, 2, C.byref(n)) == 0
    assert n.value == 5 and list(starts) == [0, 2]


def test_the_header_agrees_with_the_restatement_under_the_sanitizers(tmp_path):
    exe, data = str(tmp_path / "tile_pass_plan"), str(tmp_path / "cases.bin")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "tile_pass_plan.cpp"), "-o", exe])
    cases = P.cases()
    with open(data, "wb") as f:
        for count, cap, clash in cases:
            f.write(struct.pack("<2i", count, cap))
            f.write(P.matrix(count, clash))
    out = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert not out.stderr.strip(), out.stderr
    lines = out.stdout.strip().splitlines()
    plans = [[] if l == "-" else [int(v) for v in l.split()] for l in lines if not l.startswith("clamp")]
    assert len(plans) == len(cases)
    for got, (count, cap, clash) in zip(plans, cases):
        assert got == P.plan(count, cap, clash), (count, cap, sorted(clash))
    clamps = {int(a): int(b) for a, b in (l[len("clamp "):].split(": ") for l in lines if l.startswith("clamp"))}
    assert clamps == {f: P.clamp_cap(f) for f in (-3, 0, 1, 2, 8, 9, 1 << 30)}


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_the_refusals_messages(hip_library):
    """All of these come before any device call, so they are the same words without a GPU."""
    lib = hip_library

    def refused(rc, word):
        text = lib.ju_last_error().decode()
        assert rc == JU_ERR_INVALID_ARGUMENT and word in text, (rc, word, text)

    refused(lib.ju_tiled_process_batch(None, None, None, 0), "tiled runtime is NULL")
    refused(lib.ju_tiled_process_frames(None, None, None, 0), "tiled runtime is NULL")
    refused(lib.ju_tiled_set_lookahead(None, 4), "tiled runtime is NULL")
    n, starts = C.c_int(), (C.c_int * 4)()
    refused(lib.ju_debug_tiled_pass_plan(4, 8, P.matrix(4, set()), starts, 4, None), "ju_debug_tiled_pass_plan: null argument")
    refused(lib.ju_debug_tiled_pass_plan(4, 8, None, starts, 4, C.byref(n)), "null argument")
    refused(lib.ju_debug_tiled_pass_plan(4, 8, P.matrix(4, set()), None, 4, C.byref(n)), "null argument")
    refused(lib.ju_debug_tiled_pass_plan(-1, 8, P.matrix(4, set()), starts, 4, C.byref(n)), "count outside 0 .. 4096")
    refused(lib.ju_debug_tiled_pass_plan(4097, 8, P.matrix(4, set()), starts, 4, C.byref(n)), "count outside 0 .. 4096")
    assert lib.ju_debug_tiled_pass_plan(0, 8, None, None, 0, C.byref(n)) == 0 and n.value == 0
    # the kernel's hook, on addresses that are never touched: every refusal precedes the first device call
    fake = 0x10000
    tiles = (C.c_void_p * 9)(*[fake + 0x100000 * (k + 1) for k in range(9)])
    odd = (C.c_void_p * 9)(*[fake + 0x100000 * (k + 1) + (8 if k == 5 else 0) for k in range(9)])
    slot = 9 * 5888

    def call(srcs=(fake, fake + 0x40000, fake + 0x80000), strides=(400, -416, 404), frames=3, sw=100, sh=70, ov=4, t=tiles, slot=slot, n=9):
        s = None if srcs is None else (C.c_void_p * len(srcs))(*srcs)
        st = None if strides is None else (C.c_ssize_t * len(strides))(*strides)
        return lib.ju_debug_tile_split_frames(s, st, frames, sw, sh, W, H, ov, t, slot, n)

    for kw, word in [(dict(frames=0), "1 .. 8 frames"), (dict(frames=9), "1 .. 8 frames"), (dict(srcs=None), "null buffer"),
                     (dict(strides=None), "null buffer"), (dict(t=None), "null buffer"), (dict(ov=8), "overlap"),
                     (dict(sw=47), "source size"), (dict(n=4), "9 tiles"), (dict(t=odd), "tile 5"),
                     (dict(srcs=(fake, None, fake)), "null buffer (frame 1)"),
                     (dict(srcs=(fake, fake, fake + 2)), "multiples of 4 (frame 2)"),
                     (dict(strides=(400, 402, 400)), "multiples of 4 (frame 1)"),
                     (dict(strides=(400, 400, -396)), "|stride| smaller than a row (frame 2)"),
                     (dict(slot=slot + 8), "the slot stride must be a multiple of 16 and hold a tile"),
                     (dict(slot=W * H * 4 - 16), "the slot stride must be a multiple of 16 and hold a tile")]:
        refused(call(**kw), word)
        assert "ju_debug_tile_split_frames: " in lib.ju_last_error().decode() or "tile_split_frames: " in lib.ju_last_error().decode()
