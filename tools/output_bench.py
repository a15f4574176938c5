"""Frames/s of ju_process_frame with the output stage (docs/output_stage.md) against the same call at the model's own
output size, psp-quality (480x270 -> 1920x1080), device NV12 in, device NV12 or P010 out.

Variants, interleaved in rounds of --frames-per-round synchronous calls on runtimes of one process, so that the clock
and the other work on the machine are shared alike:

  nv12_1920x1080 / p010_1920x1080   runtimes without the stage (the staged path as it was; P010 from the f16 state)
  nv12_1280x720  / p010_1280x720    ju_set_output_size(1280, 720): scale_bgrx on the 8-bit frame / scale_state + the
  nv12_3840x2160 / p010_3840x2160   encode from the 16-bit frame; and the same at 3840x2160

--filter NAME[,NAME...] (triangle, catmull-rom, mitchell; default triangle) chooses the filter of the scaled variants;
with several names every scaled variant exists once per filter, its name ending in the filter's (the triangle's has no
suffix), all in the same process and the same rounds -- the triangle is the comparison point of the cubic filters.
--sizes WxH[,WxH...] replaces the two output sizes.

Prints one JSON line.  --profile N instead runs N frames of each scaled variant only, for a
`rocprofv3 --kernel-trace --stats -- python tools/output_bench.py --profile N` run."""

import argparse
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
import yuv_reference as Y  # noqa: E402

CS = R.CS_BT709_LIMITED
SIZES = ((1280, 720), (3840, 2160))
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


def out_frame(fmt, w, h, dev, keep):
    dt = torch.uint8 if fmt == R.FMT_NV12 else torch.int16          # (16-bit words; the bench never reads them)
    planes = [torch.zeros((h, w), dtype=dt, device=dev), torch.zeros((h // 2, w), dtype=dt, device=dev)]
    keep.append(planes)
    return R.device_frame(fmt, w, h, planes, colorspace=CS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames-per-round", type=int, default=300)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--filter", default="triangle")
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES))
    args = ap.parse_args()
    filters = [(name, FILTERS[name]) for name in args.filter.split(",")]
    sizes = tuple(tuple(int(x) for x in s.split("x")) for s in args.sizes.split(","))
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    keep = []
    inputs = nv12_device(M.synthetic_frames(4, h, w, seed=1234, kind="smooth"), dev, keep)
    runtimes, outputs = {}, {}
    for fmt, tag in ((R.FMT_NV12, "nv12"), (R.FMT_P010, "p010")):
        name = f"{tag}_{4 * w}x{4 * h}"
        runtimes[name], outputs[name] = R.Runtime(blob, 0, R.DTYPE_BF16, hooks=False), out_frame(fmt, 4 * w, 4 * h, dev, keep)
        for (ow, oh) in sizes:
            for fname, filt in filters:
                name = f"{tag}_{ow}x{oh}" + ("" if filt == R.SCALE_TRIANGLE else "_" + fname)
                rt = R.Runtime(blob, 0, R.DTYPE_BF16, hooks=False)
                rt.set_output_size(ow, oh, filt)
                runtimes[name], outputs[name] = rt, out_frame(fmt, ow, oh, dev, keep)
    torch.cuda.synchronize()

    def run(name, count):
        rt, out = runtimes[name], outputs[name]
        for i in range(count):
            rt.process_frame(inputs[i % len(inputs)], out)

    names = list(runtimes)
    scaled = [n for n in names if runtimes[n].stat("output_scaled")]
    if args.profile:
        for name in scaled:
            run(name, args.profile)
        print(json.dumps({"profiled": scaled, "frames_each": args.profile}))
        return
    for name in names:
        run(name, 50)
    rates = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            t0 = time.perf_counter()
            run(name, args.frames_per_round)
            rates[name].append(args.frames_per_round / (time.perf_counter() - t0))
    result = {"tool": "output_bench", "preset": args.preset, "dtype": "bf16", "input": f"nv12 {w}x{h}",
              "frames_per_round": args.frames_per_round, "filters": [f for f, _ in filters],
              "frames_per_s": {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                               for k, v in rates.items()},
              "source_stage_frames": {k: runtimes[k].stat("source_stage_frames") for k in names}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
