"""Frames/s of tiled upscaling (ju_tiled_process; docs/tiled.md) on one GPU, seeded weights, device BGRX frames.

Per source size in --sizes (default 960x540 1280x720; psp-quality bf16, overlap 16), two ju_tiled objects of the same model:
  tiled:   as created by default -- the tiles advance as group passes (ju_process_group inside the object);
  serial:  created under JU_LOOKAHEAD=1 (the documented switch, read when a runtime is created: no passes) -- the same
           tiles through ju_process one by one, between the same two kernels.
The difference between the two is what the group pass gives.  The variants run alternately, round after round, in one
process (the clock and the machine's other work are shared alike), after a warm-up of each.  Prints one JSON line: per
size and variant the median, min and max frames/s over the rounds and tiled / serial; the "group_frames" stat shows that
each variant took its route.

--trace WxH runs the tiled variant alone for a `rocprofv3 --kernel-trace --stats` run; --summarize <kernel_stats.csv> WxH
prints the two tile kernels' time per call from such a run, and the least time the bytes they must move would take at
the copy bandwidth measured for the MI355X (6.29 TB/s, a float4 copy): their share of it."""

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
TILE_KERNELS = ("tile_split_kernel", "tile_stitch_kernel")


def size(text):
    w, h = (int(v) for v in text.lower().split("x"))
    return w, h


def kernel_bytes(sw, sh, w, h, ov):
    """The bytes each kernel must move: the split reads the source once and writes every tile; the stitch reads every
    output pixel once where one tile covers it -- and the seams' pixels from two or four -- and writes the frame."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tiled_reference as T
    nx, ny = len(T.origins(sw, w, ov)), len(T.origins(sh, h, ov))

    def reads(S, t):                                                # tile reads per output coordinate, summed over the axis
        _, _, q = T.layout(S, t, ov)
        return int((1 + (q != 0)).sum())
    split = 4 * sw * sh + 4 * w * h * nx * ny
    stitch = 4 * reads(sw, w) * reads(sh, h) + 64 * sw * sh
    return {"tiles": [nx, ny], "tile_split_kernel": split, "tile_stitch_kernel": stitch}


def summarize(path, sw, sh, w, h, ov):
    need = kernel_bytes(sw, sh, w, h, ov)
    out = {"stats": path, "source": f"{sw}x{sh}", "tiles": need["tiles"], "copy_bandwidth_TBps": COPY_BYTES_PER_S / 1e12}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in TILE_KERNELS:
                if k in r["Name"]:
                    us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"])
                    least = need[k] / COPY_BYTES_PER_S * 1e6
                    out[k] = {"calls": int(r["Calls"]), "us_per_call": round(us, 2), "bytes": need[k],
                              "least_us_at_copy_bandwidth": round(least, 2), "share_of_copy_bandwidth": round(least / us, 3)}
    print(json.dumps(out))


class Pair:
    """The two variants for one source size, with their device frames."""

    def __init__(self, sw, sh, preset, dtype, ov, only=None):
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[dtype]
        self.obj = {}
        for name in ("tiled", "serial"):
            if only and name != only:
                continue
            if name == "serial":
                os.environ["JU_LOOKAHEAD"] = "1"
            try:
                self.obj[name] = R.TiledRuntime(blob, 0, dt, sw, sh, ov, hooks=False)
            finally:
                os.environ.pop("JU_LOOKAHEAD", None)
        clip = M.synthetic_frames(4, sh, sw, seed=1234, kind="noise")
        self.d_in = torch.from_numpy(clip).to(dev)
        self.d_out = torch.zeros((4 * sh, 4 * sw, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.ins = [R.JuImage(self.d_in[t].data_ptr(), R.LOC_DEVICE, 4 * sw, sw, sh) for t in range(4)]
        self.out = R.JuImage(self.d_out.data_ptr(), R.LOC_DEVICE, 16 * sw, 4 * sw, 4 * sh)
        self.lib = next(iter(self.obj.values()))._lib

    def run(self, name, frames):
        h = self.obj[name]._h
        t0 = time.perf_counter()
        for t in range(frames):
            if self.lib.ju_tiled_process(h, C.byref(self.ins[t % 4]), C.byref(self.out)) != 0:
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
        p = Pair(*size(args.trace), args.preset, args.dtype, args.overlap, only="tiled")
        p.run("tiled", args.warmup)
        p.run("tiled", args.frames)
        print(json.dumps({"trace": args.trace, "frames": args.warmup + args.frames,
                          "group_frames": p.obj["tiled"].stat("group_frames")}))
        p.close()
        return
    res = {}
    for text in args.sizes:
        sw, sh = size(text)
        p = Pair(sw, sh, args.preset, args.dtype, args.overlap)
        for name in p.obj:
            p.run(name, args.warmup)
        fps = {name: [] for name in p.obj}
        for _ in range(args.rounds):
            for name in p.obj:
                fps[name].append(args.frames / p.run(name, args.frames))
        row = {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
               for name, v in fps.items()}
        row["tiled_over_serial"] = round(row["tiled"]["median"] / row["serial"]["median"], 3)
        row["tiles"] = p.obj["tiled"].info()["tiles_x"] * p.obj["tiled"].info()["tiles_y"]
        row["group_frames"] = {name: o.stat("group_frames") for name, o in p.obj.items()}
        row["frames"] = {name: o.stat("frames") for name, o in p.obj.items()}
        res[text] = row
        p.close()
    print(json.dumps({"metric": "frames/s of ju_tiled_process, device BGRX in and out", "preset": args.preset,
                      "dtype": args.dtype, "overlap": args.overlap, "frames_per_round": args.frames, "rounds": args.rounds,
                      "variants": {"tiled": "the tiles as group passes", "serial": "the same object created under "
                                   "JU_LOOKAHEAD=1: every tile through ju_process, the same two kernels"},
                      "fps": res}))


if __name__ == "__main__":
    main()
