"""Frames/s of ju_process_frame with the source stage (docs/source_stage.md) against the same call on model-size
frames, psp-quality at 480x270, device NV12 in, device NV12 out.

Variants, interleaved in rounds of --frames-per-round synchronous calls on runtimes of one process, so that the clock
and the other work on the machine are shared alike:

  nv12_model    a runtime without the stage, 480x270 NV12 frames (the staged path as it was)
  nv12_scaled   a runtime with ju_set_source_size(1920, 1080), 1920x1080 NV12 frames: decode at source size + scale
  nv12_masked   the same with the mask of tests/golden/obs_mask.png set as well: + blend, NV12 encoded from the blended frame
  bgrx_model    ju_process on model-size device BGRX frames through the direct path, for scale (the stage gives it up)

--filter NAME[,NAME...] (triangle, catmull-rom, mitchell; default triangle) chooses the filter of nv12_scaled and
nv12_masked; with several names both exist once per filter, the name ending in the filter's (the triangle's has no suffix),
all in the same process and the same rounds.

Prints one JSON line.  --profile N instead runs N frames of nv12_masked (of every filter) only, for a `rocprofv3 --kernel-trace --stats`
run (the program after `--`)."""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (torch's HIP runtime first, as bench.py does)

from joshupscale_amd import model_file as M  # noqa: E402
from joshupscale_amd import runtime as R  # noqa: E402
import source_reference as S  # noqa: E402
import yuv_reference as Y  # noqa: E402

CS = R.CS_BT709_LIMITED
FILTERS = {"triangle": R.SCALE_TRIANGLE, "catmull-rom": R.SCALE_CATMULL_ROM, "mitchell": R.SCALE_MITCHELL}


def nv12_device(frames, dev, keep):
    """Device NV12 frames of BGRX host frames."""
    out = []
    for f in frames:
        y, u, v = Y.encode(f, CS)
        planes = [torch.from_numpy(y).to(dev), torch.from_numpy(Y.to_nv12(u, v)).to(dev)]
        keep.append(planes)
        out.append(R.device_frame(R.FMT_NV12, f.shape[1], f.shape[0], planes, colorspace=CS))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--source", default="1920x1080")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames-per-round", type=int, default=300)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--filter", default="triangle")
    args = ap.parse_args()
    filters = [(name, FILTERS[name]) for name in args.filter.split(",")]
    suffix = lambda fname, filt: "" if filt == R.SCALE_TRIANGLE else "_" + fname
    sw, sh = (int(x) for x in args.source.split("x"))
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    keep = []
    big = M.synthetic_frames(4, sh, sw, seed=1234, kind="smooth")
    small = M.synthetic_frames(4, h, w, seed=1234, kind="smooth")
    mask = S.read_png_palette_1bit(os.path.join(ROOT, "tests", "golden", "obs_mask.png"))
    out_planes = [torch.zeros((4 * h, 4 * w), dtype=torch.uint8, device=dev),
                  torch.zeros((2 * h, 4 * w), dtype=torch.uint8, device=dev)]
    out_nv12 = R.device_frame(R.FMT_NV12, 4 * w, 4 * h, out_planes, colorspace=CS)
    out_bgrx = torch.zeros((4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
    d_small = [torch.from_numpy(f).to(dev) for f in small]
    scaled = [base + suffix(*f) for f in filters for base in ("nv12_scaled", "nv12_masked")]
    runtimes = {name: R.Runtime(blob, 0, R.DTYPE_BF16, hooks=False) for name in ["nv12_model"] + scaled + ["bgrx_model"]}
    inputs = {"nv12_model": nv12_device(small, dev, keep)}
    big_frames = nv12_device(big, dev, keep)
    for fname, filt in filters:
        for base in ("nv12_scaled", "nv12_masked"):
            runtimes[base + suffix(fname, filt)].set_source_size(sw, sh, filt)
            inputs[base + suffix(fname, filt)] = big_frames
        runtimes["nv12_masked" + suffix(fname, filt)].set_source_mask(mask)
    rb = runtimes["bgrx_model"]
    pairs = [(rb.device_image(t.data_ptr(), w, h), rb.device_image(out_bgrx.data_ptr(), 4 * w, 4 * h)) for t in d_small]
    for a, b in pairs:
        rb.prepare_frames(a, b)
    torch.cuda.synchronize()

    def run(name, count):
        rt = runtimes[name]
        if name == "bgrx_model":
            for i in range(count):
                rt.process(*pairs[i % len(pairs)])
            return
        frames = inputs[name]
        for i in range(count):
            rt.process_frame(frames[i % len(frames)], out_nv12)

    if args.profile:
        masked = ["nv12_masked" + suffix(*f) for f in filters]
        for name in masked:
            run(name, args.profile)
        print(json.dumps({"profiled": masked, "frames": args.profile, "source": args.source}))
        return
    names = list(runtimes)
    for name in names:
        run(name, 50)
    rates = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            t0 = time.perf_counter()
            run(name, args.frames_per_round)
            rates[name].append(args.frames_per_round / (time.perf_counter() - t0))
    result = {"tool": "source_bench", "preset": args.preset, "dtype": "bf16", "source": args.source,
              "frames_per_round": args.frames_per_round, "filters": [f for f, _ in filters],
              "frames_per_s": {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                               for k, v in rates.items()},
              "source_stage_frames": {k: runtimes[k].stat("source_stage_frames") for k in names}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
