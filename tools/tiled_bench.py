"""Frames/s of tiled upscaling (ju_tiled_process; docs/tiled.md) on one GPU, seeded weights, device BGRX frames.

Per source size in --sizes (default 960x540 1280x720; psp-quality bf16, overlap 16), two ju_tiled objects of the same model:
  tiled:   as created by default -- the tiles advance as group passes (ju_process_group inside the object);
  serial:  created under JU_LOOKAHEAD=1 (the documented switch, read when a runtime is created: no passes) -- the same
           tiles through ju_process one by one, between the same two kernels.
The difference between the two is what the group pass gives.  The variants run alternately, round after round, in one
process (the clock and the machine's other work are shared alike), after a warm-up of each.  Prints one JSON line: per
size and variant the median, min and max frames/s over the rounds and tiled / serial; the "group_frames" stat shows that
each variant took its route.

--out-format names the output frames' format (default bgrx; nv12, p010, i410, bgrx64, rgbph: device planes through
ju_tiled_process_frame).  --compare deep runs, instead of tiled / serial, two objects that both advance as group passes:
  deep_off:  ju_tiled_set_deep_from_state 0 -- a deep format encoded from the blended 8-bit frame (the yardstick);
  deep_on:   the setting at 1 -- from the blend of the tiles' f16 states (docs/tiled.md "Deep outputs");
"deep_state_frames" shows that each took its route.  --compare scene runs three objects that all advance as group passes:
  scene_off / scene_report / scene_reset:  ju_tiled_set_scene_detect off (the yardstick), JU_SCENE_REPORT and JU_SCENE_RESET
  (docs/tiled.md "Scene cuts"; --threshold, default 10000);
"scene_cuts" shows what each saw.  --clip cuts replaces the four noise frames (no cut: S_t is large and constant) by four
smooth scenes of four frames each, a cut every fourth frame.

--trace WxH runs one variant alone (--deep-from-state 0 | 1, --scene off | report | reset, --out-format, --clip) for a `rocprofv3 --kernel-trace --stats` run;
--summarize <kernel_stats.csv> WxH prints the tile kernels' and the 10-bit 4:2:0 encodes' time per call from such a run,
and the least time the bytes they must move would take at the copy bandwidth measured for the MI355X (6.29 TB/s, a
float4 copy): their share of it."""

import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BYTES_PER_S = 6.29e12
TILE_KERNELS = ("tile_split_kernel", "tile_split_scene_kernel", "scene_clear_tiles_kernel", "tile_stitch_kernel", "tile_stitch_state_kernel", "frame16_to_yuv420p10_kernel",
                "bgrx_to_yuv420p10_kernel")
# what a variant is: created under JU_LOOKAHEAD=1 (no passes), its ju_tiled_set_deep_from_state, its scene mode
VARIANTS = {"tiled": (False, 0, 0), "serial": (True, 0, 0), "deep_off": (False, 0, 0), "deep_on": (False, 1, 0),
            "scene_off": (False, 0, 0), "scene_report": (False, 0, 1), "scene_reset": (False, 0, 2)}
SCENE_NAMES = {"off": "scene_off", "report": "scene_report", "reset": "scene_reset"}
# output formats: (the runtime's FMT_ name, per plane (rows per output row, bytes per output pixel of a row))
OUT_FORMATS = {"bgrx": ("FMT_BGRX", [(1, 4)]), "nv12": ("FMT_NV12", [(1, 1), (0.5, 1)]), "p010": ("FMT_P010", [(1, 2), (0.5, 2)]),
               "i410": ("FMT_I410", [(1, 2)] * 3), "bgrx64": ("FMT_BGRX64", [(1, 8)]), "rgbph": ("FMT_RGBPH", [(1, 2)] * 3)}


def size(text):
    w, h = (int(v) for v in text.lower().split("x"))
    return w, h


def kernel_bytes(sw, sh, w, h, ov):
    """The bytes each kernel must move: the split reads the source once and writes every tile; the stitch reads every
    output pixel once where one tile covers it -- and the seams' pixels from two or four -- and writes the frame; the
    stitch of the states the same at 8 bytes per pixel; a P010 encode reads its frame (8 or 4 bytes per pixel) and writes
    3 bytes per pixel.  The split with the detector also reads and rewrites the kept source-size frame; the conditional
    clear reads one flag word per workgroup while no cut is flagged (its bytes at a cut depend on the model: not listed)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tiled_reference as T
    nx, ny = len(T.origins(sw, w, ov)), len(T.origins(sh, h, ov))

    def reads(S, t):                                                # tile reads per output coordinate, summed over the axis
        _, _, q = T.layout(S, t, ov)
        return int((1 + (q != 0)).sum())
    split = 4 * sw * sh + 4 * w * h * nx * ny
    stitch = 4 * reads(sw, w) * reads(sh, h) + 64 * sw * sh
    return {"tiles": [nx, ny], "tile_split_kernel": split, "tile_split_scene_kernel": split + 8 * sw * sh, "tile_stitch_kernel": stitch, "tile_stitch_state_kernel": 2 * stitch,
            "frame16_to_yuv420p10_kernel": (8 + 3) * 16 * sw * sh, "bgrx_to_yuv420p10_kernel": (4 + 3) * 16 * sw * sh}


def summarize(path, sw, sh, w, h, ov):
    need = kernel_bytes(sw, sh, w, h, ov)
    out = {"stats": path, "source": f"{sw}x{sh}", "tiles": need["tiles"], "copy_bandwidth_TBps": COPY_BYTES_PER_S / 1e12}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in TILE_KERNELS:
                if k in r["Name"]:                                 # (no name of the list is part of another)
                    us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"])
                    if k not in need:
                        out[k] = {"calls": int(r["Calls"]), "us_per_call": round(us, 2)}
                        continue
                    least = need[k] / COPY_BYTES_PER_S * 1e6
                    out[k] = {"calls": int(r["Calls"]), "us_per_call": round(us, 2), "bytes": need[k],
                              "least_us_at_copy_bandwidth": round(least, 2), "share_of_copy_bandwidth": round(least / us, 3)}
    print(json.dumps(out))


class Pair:
    """The variants for one source size, with their device frames."""

    def __init__(self, sw, sh, preset, dtype, ov, names=("tiled", "serial"), out_format="bgrx", clip="noise", threshold=10000):
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[dtype]
        self.obj = {}
        for name in names:
            serial, deep, scene = VARIANTS[name]
            if serial:
                os.environ["JU_LOOKAHEAD"] = "1"
            try:
                self.obj[name] = R.TiledRuntime(blob, 0, dt, sw, sh, ov, hooks=False)
            finally:
                os.environ.pop("JU_LOOKAHEAD", None)
            self.obj[name].set_deep_from_state(deep)
            if scene:
                self.obj[name].set_scene_detect(scene, threshold)
        if clip == "cuts":
            import numpy as np
            clip = np.ascontiguousarray(np.concatenate([M.synthetic_frames(4, sh, sw, seed=seed, kind="smooth")
                                                        for seed in (1, 2, 3, 4)], axis=0))
        else:
            clip = M.synthetic_frames(4, sh, sw, seed=1234, kind="noise")
        self.count = len(clip)
        self.d_in = torch.from_numpy(clip).to(dev)
        fmt_name, planes = OUT_FORMATS[out_format]
        self.d_out = [torch.zeros((int(4 * sh * rows), 4 * sw * width), dtype=torch.uint8, device=dev) for rows, width in planes]
        torch.cuda.synchronize()
        self.frames = out_format != "bgrx"       # (ju_tiled_process_frame; else ju_tiled_process on two images)
        if self.frames:
            self.ins = [R.device_frame(R.FMT_BGRX, sw, sh, [self.d_in[t].data_ptr()]) for t in range(self.count)]
            self.out = R.device_frame(getattr(R, fmt_name), 4 * sw, 4 * sh, self.d_out)
        else:
            self.ins = [R.JuImage(self.d_in[t].data_ptr(), R.LOC_DEVICE, 4 * sw, sw, sh) for t in range(self.count)]
            self.out = R.JuImage(self.d_out[0].data_ptr(), R.LOC_DEVICE, 16 * sw, 4 * sw, 4 * sh)
        self.lib = next(iter(self.obj.values()))._lib

    def run(self, name, frames):
        h = self.obj[name]._h
        call = self.lib.ju_tiled_process_frame if self.frames else self.lib.ju_tiled_process
        t0 = time.perf_counter()
        for t in range(frames):
            if call(h, C.byref(self.ins[t % self.count]), C.byref(self.out)) != 0:
                raise RuntimeError(self.lib.ju_last_error().decode())
        return time.perf_counter() - t0          # (every call is synchronous)

    def close(self):
        for o in self.obj.values():
            o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp8"])
    ap.add_argument("--sizes", nargs="+", default=["960x540", "1280x720"])
    ap.add_argument("--overlap", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=240, help="frames per variant and round")
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--out-format", default="bgrx", choices=sorted(OUT_FORMATS))
    ap.add_argument("--compare", default="passes", choices=["passes", "deep", "scene"],
                    help="passes: tiled against serial; deep: ju_tiled_set_deep_from_state 0 against 1; scene: the scene "
                         "detector off, JU_SCENE_REPORT and JU_SCENE_RESET")
    ap.add_argument("--scene", default="off", choices=sorted(SCENE_NAMES), help="--trace: the scene mode of the one variant")
    ap.add_argument("--clip", default="noise", choices=["noise", "cuts"])
    ap.add_argument("--threshold", type=int, default=10000, help="threshold_milli of the scene detector")
    ap.add_argument("--deep-from-state", type=int, default=0, choices=[0, 1], help="--trace: the setting of the one variant")
    ap.add_argument("--trace", default=None, metavar="WxH")
    ap.add_argument("--summarize", nargs=2, metavar=("CSV", "WxH"), default=None)
    args = ap.parse_args()
    from joshupscale_amd import model_file as M
    cfg = M.PRESETS[args.preset]
    if args.summarize:
        summarize(args.summarize[0], *size(args.summarize[1]), cfg.frame_width, cfg.frame_height, args.overlap)
        return
    import torch
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first, as bench.py does)
    if args.trace:
        name = "deep_on" if args.deep_from_state else SCENE_NAMES[args.scene] if args.scene != "off" else "tiled"
        p = Pair(*size(args.trace), args.preset, args.dtype, args.overlap, (name,), args.out_format, args.clip, args.threshold)
        p.run(name, args.warmup)
        p.run(name, args.frames)
        print(json.dumps({"trace": args.trace, "variant": name, "out_format": args.out_format, "frames": args.warmup + args.frames,
                          "group_frames": p.obj[name].stat("group_frames"),
                          "deep_state_frames": p.obj[name].stat("deep_state_frames"), "clip": args.clip,
                          "scene_cuts": p.obj[name].stat("scene_cuts")}))
        p.close()
        return
    res = {}
    names = {"deep": ("deep_off", "deep_on"), "scene": ("scene_off", "scene_report", "scene_reset")}.get(args.compare, ("tiled", "serial"))
    for text in args.sizes:
        sw, sh = size(text)
        p = Pair(sw, sh, args.preset, args.dtype, args.overlap, names, args.out_format, args.clip, args.threshold)
        for name in p.obj:
            p.run(name, args.warmup)
        fps = {name: [] for name in p.obj}
        for _ in range(args.rounds):
            for name in p.obj:
                fps[name].append(args.frames / p.run(name, args.frames))
        row = {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
               for name, v in fps.items()}
        for other in names[1:]:
            key = names[0] + "_over_" + other if len(names) == 2 else other + "_over_" + names[0]
            a, b = (names[0], other) if len(names) == 2 else (other, names[0])
            row[key] = round(row[a]["median"] / row[b]["median"], 4 if len(names) > 2 else 3)
        row["tiles"] = p.obj[names[0]].info()["tiles_x"] * p.obj[names[0]].info()["tiles_y"]
        row["group_frames"] = {name: o.stat("group_frames") for name, o in p.obj.items()}
        row["deep_state_frames"] = {name: o.stat("deep_state_frames") for name, o in p.obj.items()}
        row["frames"] = {name: o.stat("frames") for name, o in p.obj.items()}
        if args.compare == "scene":
            row["scene_cuts"] = {name: o.stat("scene_cuts") for name, o in p.obj.items()}
        res[text] = row
        p.close()
    what = {"tiled": "the tiles as group passes", "serial": "the same object created under JU_LOOKAHEAD=1: every tile "
            "through ju_process, the same two kernels", "deep_off": "ju_tiled_set_deep_from_state 0: a deep format from the "
            "blended 8-bit frame", "deep_on": "ju_tiled_set_deep_from_state 1: from the blend of the tiles' f16 states",
            "scene_off": "the scene detector off: the split alone", "scene_report": "JU_SCENE_REPORT: the split and the "
            "detector in one launch", "scene_reset": "JU_SCENE_RESET: that launch and the conditional clear of all tiles"}
    print(json.dumps({"metric": "frames/s of ju_tiled_process, device BGRX in, device " + args.out_format.upper() + " out",
                      "preset": args.preset, "dtype": args.dtype, "overlap": args.overlap, "frames_per_round": args.frames,
                      "rounds": args.rounds, "clip": args.clip, "variants": {name: what[name] for name in names}, "fps": res}))


if __name__ == "__main__":
    main()
