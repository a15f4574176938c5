"""joshupscale_amd/csrc/scene_clock.h (the scene detector's clock: the record's step, its ring slot, the has-predecessor
bits, the steps a query returns) from a stand-alone host program, tests/cxx/scene_clock.cpp, under the address and
undefined-behaviour sanitizers.  No GPU, no HIP header: the header is plain C++.  The expectation is derived here, from the
definition (docs/scene_detect.md), and tests/scene_reference.py's Detector is held to the same numbering."""

import os
import subprocess

import numpy as np

import scene_reference as S
from helpers import ROOT

QUERIES = (0, 1, 63, 64, 65, 1000)


def script():
    """Single steps, passes of 1 .. 8 steps, restart() at step 0, after one step and after many, 200 steps (the 64-slot
    ring wraps three times), a new start, and the queries at every stage."""
    ops = [("r",)] + [("q", c) for c in QUERIES]            # restart at step 0; queries of an empty ring
    ops += [("s",), ("r",), ("s",), ("s",), ("s",)]          # restart after one step
    ops += [("q", c) for c in QUERIES]
    for n in range(1, 9):
        ops += [("a", n), ("q", n), ("q", n + 1)]
    ops += [("r",), ("a", 1), ("a", 1), ("a", 3)]             # restart after many; has-predecessor bits under passes
    ops += [("s",)] * 200
    ops += [("q", c) for c in QUERIES]
    ops += [("r",), ("a", 8), ("s",), ("q", 64), ("q", 65)]
    ops += [("n",), ("q", 5), ("s",), ("a", 2), ("q", 5)]     # a mode change: step 0 again
    return ops


def expected(ops):
    """The definition: slot = step mod RING; bits 0, 1, 3 for 0, 1, >= 2 frames in memory; the window is the last
    min(count, RING, steps) steps, oldest first."""
    seen = steps = 0
    lines = []
    for op in ops:
        bits = (0, 1, 3)[min(seen, 2)]
        if op[0] == "s":
            lines.append(f"step {steps} {steps % S.RING} {bits} {min(seen, 2)}")
            seen, steps = seen + 1, steps + 1
        elif op[0] == "a":
            lines.append(f"pass {op[1]} {steps} {steps % S.RING} {bits} {min(seen, 2)}")
            seen, steps = seen + op[1], steps + op[1]
        elif op[0] == "r":
            seen = 0
        elif op[0] == "n":
            seen = steps = 0
        else:
            n = min(op[1], S.RING, steps)
            lines.append(f"window {op[1]}:" + "".join(f" {s}" for s in range(steps - n, steps)))
    return lines + ["scene_clock ok"]


def test_scene_clock_host_program(tmp_path):
    exe = str(tmp_path / "scene_clock")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "joshupscale_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "scene_clock.cpp"), "-o", exe])
    ops = script()
    out = subprocess.run([exe], input=" ".join(str(t) for op in ops for t in op), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().split("\n")
    want = expected(ops)
    assert sum(1 for op in ops if op[0] == "s") >= 200 > 3 * S.RING  # (the script: the ring wraps three times)
    assert got == want, next((g, w) for g, w in zip(got + [None], want + [None]) if g != w)


def test_reference_detector_numbers_its_steps_the_same_way():
    """tests/scene_reference.py Detector over the same script: the record's step and the frames in its memory are the
    clock's, across restart() -- a pass of n steps is n feeds."""
    ops = [op for op in script() if op[0] != "q"]
    cut = next(i for i, op in enumerate(ops) if op[0] == "n")  # (a mode change makes a new Detector: not part of it)
    frame = np.zeros((2, 2, 4), np.uint8)
    det = S.Detector(S.KNOWN_THRESHOLD)
    lines = []
    for op in ops[:cut]:
        bits = (0, 1, 3)[min(det.seen, 2)]
        if op[0] == "r":
            det.restart()
            continue
        n = 1 if op[0] == "s" else op[1]
        recs = [det.feed(frame) for _ in range(n)]
        assert [r["step"] for r in recs] == list(range(recs[0]["step"], recs[0]["step"] + n))
        head = "step" if op[0] == "s" else f"pass {n}"
        lines.append(f"{head} {recs[0]['step']} {recs[0]['step'] % S.RING} {bits} {min(det.seen - n, 2)}")
    assert lines == [line for line in expected(ops[:cut]) if line != "scene_clock ok"]
