"""What look-ahead passes give scaled and masked frames (docs/source_stage.md and docs/output_stage.md, "Passes"):
psp-quality bf16 (480x270 -> 1920x1080), ju_process_frames in calls of --passes (8) frames over a ring of 16 frame
buffers, noise frames.  Three cases, three runtimes each:

  nv12-720p      device NV12 1280x720  -> device NV12 1280x720   (a source size and an output size)
  bgrx-2160p     device BGRX 1280x720  -> device BGRX 3840x2160  (the same, the frames scaled in place)
  host-p010      host NV12 480x270     -> host P010 3840x2160    (an output size alone, deep frames from the state)

  off       ju_set_stage_lookahead 0: every frame on its own through the staged route -- what the parent commit does
  on        ju_set_stage_lookahead 1: the same calls in look-ahead passes
  unstaged  a runtime without stage settings fed model-size frames of the same formats and locations, in passes: the
            ceiling the stages' own kernels and copies keep "on" below

All runtimes live in one process and are timed in turn, --runs rounds of --frames frames each after --warmup, so that the
clock and the other work on the machine are shared alike; the yardstick for "on" is "off" of the same process.  Prints
one JSON line: frames/s of every round, the median and the spread, and the counters that show which route the frames took.
--tree PATH imports the package (and with it the library) from another checkout -- the parent commit's build, whose
runtime has no setting: the "on" rows are then left out.  --profile N instead runs N frames of the bgrx-2160p and
nv12-720p "on" and "off" runtimes only, for a `rocprofv3 --kernel-trace --stats` run of its own."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch's HIP runtime first, as bench.py does)

if "--tree" in sys.argv:  # (before the package is imported: another checkout's)
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]))

from joshupscale_amd import model_file as M  # noqa: E402
from joshupscale_amd import runtime as R  # noqa: E402

RING = 16
CS = R.CS_BT709_LIMITED
# case: (input format, location, (w, h) or None = the model's; output format, location, (w, h) or None)
CASES = {"nv12-720p": (R.FMT_NV12, "device", (1280, 720), R.FMT_NV12, "device", (1280, 720)),
         "bgrx-2160p": (R.FMT_BGRX, "device", (1280, 720), R.FMT_BGRX, "device", (3840, 2160)),
         "host-p010": (R.FMT_NV12, "host", None, R.FMT_P010, "host", (3840, 2160))}


def planes_of(fmt, w, h, rng):
    """Noise planes of one frame as numpy arrays."""
    if fmt == R.FMT_BGRX:
        return [rng.integers(0, 256, (h, w, 4), dtype=np.uint8)]
    if fmt == R.FMT_NV12:
        return [rng.integers(16, 236, (h, w), dtype=np.uint8), rng.integers(16, 241, (h // 2, w), dtype=np.uint8)]
    return [np.zeros((h, w), np.uint16), np.zeros((h // 2, w), np.uint16)]  # (FMT_P010: outputs only)


class Ring:
    """RING frames of one side: the planes (host arrays, or device tensors) and their ju_frames."""

    def __init__(self, fmt, location, w, h, dev, seed):
        rng = np.random.default_rng(seed)
        self.keep, self.frames = [], []
        for _ in range(RING):
            planes = planes_of(fmt, w, h, rng)
            if location == "host":
                self.keep.append(planes)
                self.frames.append(R.host_frame(fmt, planes, CS))
                continue
            rows = [p.reshape(p.shape[0], -1).view(np.uint8) for p in planes]
            held = [torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in rows]
            self.keep.append(held)
            self.frames.append(R._frame(fmt, CS, R.LOC_DEVICE, w, h, [t.data_ptr() for t in held], [t.shape[1] for t in held]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--tree", default="")
    args = ap.parse_args()
    if not 2 <= args.passes <= 8 or RING % args.passes:
        ap.error("--passes takes 2, 4 or 8")
    n = args.passes
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    has_setting = hasattr(R.Runtime, "set_stage_lookahead")
    rows = {}
    for name in args.cases.split(","):
        fin, lin, src, fout, lout, out = CASES[name]
        for variant in ("off", "on", "unstaged"):
            if variant == "on" and not has_setting:
                continue
            if args.profile and (variant == "unstaged" or name == "host-p010"):
                continue
            staged = variant != "unstaged"
            rt = R.Runtime(blob, 0, R.DTYPE_BF16, hooks=False)
            rt.set_lookahead(n)
            iw, ih = (src if staged and src else (w, h))
            ow, oh = (out if staged and out else (4 * w, 4 * h))
            if staged and src:
                rt.set_source_size(iw, ih)
            if staged and out:
                rt.set_output_size(ow, oh)
            if variant == "on":
                rt.set_stage_lookahead(1)
            ins, outs = Ring(fin, lin, iw, ih, dev, 1234), Ring(fout, lout, ow, oh, dev, 99)
            calls = [((R.JuFrame * n)(*ins.frames[lo:lo + n]), (R.JuFrame * n)(*outs.frames[lo:lo + n])) for lo in range(0, RING, n)]
            rows[name + "/" + variant] = (rt, calls, (ins, outs))
    torch.cuda.synchronize()

    def run(key, frames):
        rt, calls, _keep = rows[key]
        proc, hnd = rt._lib.ju_process_frames, rt._h
        for i in range(frames // n):
            a, b = calls[i % len(calls)]
            if proc(hnd, a, b, n):
                raise RuntimeError(rt._lib.ju_last_error().decode())

    def stat(rt, key):
        try:
            return rt.stat(key)
        except R.JoshUpscaleError:
            return None

    if args.profile:
        for key in rows:
            run(key, args.profile // n * n)
        print(json.dumps({"profiled": list(rows), "frames_each": args.profile // n * n}))
        return
    frames = args.frames // n * n
    for key in rows:
        run(key, max(args.warmup // n, 3 * (RING // n)) * n)      # (every tuple seen three times: eager, captured, replayed)
    rates = {key: [] for key in rows}
    for _ in range(args.runs):
        for key in rows:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, frames)
            torch.cuda.synchronize()
            rates[key].append(frames / (time.perf_counter() - t0))
    median = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps({
        "tool": "stage_pass_bench", "preset": args.preset, "dtype": "bf16", "pass_frames": n, "frames": frames, "runs": args.runs,
        "tree": args.tree or ".", "has_setting": has_setting,
        "frames_per_s": {k: {"runs": [round(x, 1) for x in v], "median": round(median[k], 1),
                             "spread_percent": round(100.0 * (max(v) - min(v)) / median[k], 2)} for k, v in rates.items()},
        "on_over_off_percent": {k.split("/")[0]: round(100.0 * (median[k] / median[k.split("/")[0] + "/off"] - 1.0), 2)
                                for k in rows if k.endswith("/on")},
        "lookahead_frames": {k: stat(rows[k][0], "lookahead_frames") for k in rows},
        "lookahead_staged_frames": {k: stat(rows[k][0], "lookahead_staged_frames") for k in rows},
        "source_stage_frames": {k: stat(rows[k][0], "source_stage_frames") for k in rows},
        "graph_captures": {k: stat(rows[k][0], "graph_captures") for k in rows},
        "fallbacks": {k: stat(rows[k][0], "fallbacks") for k in rows}}))


if __name__ == "__main__":
    main()
