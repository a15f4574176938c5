"""What ju_set_alpha costs (docs/alpha.md "Measurements") on one GPU, seeded weights, device frames.

Default: frames/s, psp-quality bf16, one process, the variants alternating round after round after a warm-up of each; the
yardstick of every workload is mode 0 in the same process:
  frame_rgbx:    ju_process_frame, RGBX device frames in and out, JU_ALPHA_ZERO / OPAQUE / SOURCE.  Both sides take the
                 staged route already, so the difference is the alpha launch.
  process_bgrx:  ju_process, device BGRX, the three modes -- here a mode other than 0 also costs the direct device path --
                 and `staged`: mode 0 of a runtime created under JU_DIRECT=0 (a developer switch of the test flavour:
                 every frame through the staging buffers), which is the route without the kernel.
  pass_bgrx / pass_rgbx: look-ahead passes of 8 device frames (ju_process_batch on BGRX, ju_process_frames on RGBX):
                 mode 0 in passes, and OPAQUE and SOURCE with ju_set_alpha_lookahead 1 (`_on`: alpha inside the pass) and 0
                 (`_off`: every frame on its own through the staged route).
  group:         8 streams of device BGRX frames through ju_process_group: mode 0, and SOURCE and OPAQUE members with
                 ju_set_alpha_group 1 (`_on`: they ride) and 0 (`_off`: each runs alone behind the pass).
  tiled_540 / tiled_720: a ju_tiled of 960x540 / 1280x720 on device BGRX frames, ju_tiled_set_alpha ZERO / OPAQUE / SOURCE.
                 (--workloads names them; profiles/alpha_pass_bench.json holds a run of them)
Prints one JSON line: per workload and variant the median, min and max frames/s over the rounds, each variant over
mode 0, and the "alpha_frames" stat that shows each took its route.

--trace KERNEL runs one alpha kernel alone through its hook (scale | fill; --sink byte | word; --size small | large:
480x270 -> 1920x1080 or 1280x720 -> 3840x2160; --filter) --calls times, for a `rocprofv3 --kernel-trace --stats` run.
--summarize <kernel_stats.csv> with the same --sink / --size prints the kernel's time per call, the bytes it must move
(the source's alpha reads -- one byte or one word per source pixel -- and the sink's writes; both sinks are plain stores,
nothing is read back) and their share of the copy bandwidth measured for the MI355X (6.29 TB/s, a float4 copy)."""

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
SIZES = {"small": ((480, 270), (1920, 1080)), "large": ((1280, 720), (3840, 2160))}
FILTERS = {"triangle": 0, "catmull-rom": 2, "mitchell": 3}
SINKS = {"byte": (0, 4, 1), "word": (1, 8, 2)}                      # kind, bytes per pixel, bytes per slot


def kernel_bytes(kernel, sink, size):
    (sw, sh), (ow, oh) = SIZES[size]
    slot = SINKS[sink][2]
    return (sw * sh * slot if kernel == "scale" else 0) + ow * oh * slot


def trace(kernel, sink, size, filt, calls):
    import torch
    from joshupscale_amd import runtime as R
    lib = R.load_library(True)
    dev = torch.device("cuda", 0)
    (sw, sh), (ow, oh) = SIZES[size]
    kind, px, _ = SINKS[sink]
    src = torch.randint(0, 256, (sh, sw * px), dtype=torch.uint8, device=dev)
    dst = torch.zeros((oh, ow * px), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for _ in range(calls):
        if kernel == "scale":
            rc = lib.ju_debug_alpha_scale(kind, kind, filt, dst.data_ptr(), ow * px, ow, oh, src.data_ptr(), sw * px, sw, sh)
        else:
            rc = lib.ju_debug_alpha_fill(kind, dst.data_ptr(), ow * px, ow, oh)
        if rc != 0:
            raise RuntimeError(lib.ju_last_error().decode())
    print(json.dumps({"traced": kernel, "sink": sink, "size": size, "filter": filt, "calls": calls}))


def summarize(path, sink, size):
    out = {"stats": os.path.basename(path), "sink": sink, "source": "%dx%d" % SIZES[size][0], "output": "%dx%d" % SIZES[size][1],
           "copy_bandwidth_TBps": COPY_BYTES_PER_S / 1e12}
    with open(path) as f:
        for r in csv.DictReader(f):
            for kernel, name in (("scale", "alpha_scale_kernel"), ("fill", "alpha_fill_kernel")):
                if name in r["Name"]:
                    us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"])
                    need = kernel_bytes(kernel, sink, size)
                    least = need / COPY_BYTES_PER_S * 1e6
                    out[name] = {"calls": int(r["Calls"]), "us_per_call": round(us, 2), "bytes": need,
                                 "least_us_at_copy_bandwidth": round(least, 2), "share_of_copy_bandwidth": round(least / us, 3)}
    print(json.dumps(out))


class Workload:
    """The variants of one workload over the same device frames."""

    def __init__(self, kind, preset, dtype, filt):
        import numpy as np
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16}[dtype]
        h, w = cfg.frame_height, cfg.frame_width
        self.kind, self.rt = kind, {}
        names = ["mode0", "opaque", "source"] + (["staged"] if kind == "process_bgrx" else [])
        for name in names:
            if name == "staged":
                os.environ["JU_DIRECT"] = "0"
            try:
                self.rt[name] = R.Runtime(blob, 0, dt, hooks=True)
            finally:
                os.environ.pop("JU_DIRECT", None)
            self.rt[name].set_alpha({"opaque": R.ALPHA_OPAQUE, "source": R.ALPHA_SOURCE}.get(name, R.ALPHA_ZERO), filt)
        clip = M.synthetic_frames(4, h, w, seed=1234, kind="noise").copy()
        clip[..., 3] = np.random.default_rng(5).integers(0, 256, clip.shape[:3], dtype=np.uint8)
        self.count = len(clip)
        self.d_in = torch.from_numpy(clip).to(dev)
        self.d_out = {n: torch.zeros((4 * h, 4 * w * 4), dtype=torch.uint8, device=dev) for n in names}
        self.lib = self.rt["mode0"]._lib
        if kind == "frame_rgbx":
            self.call = self.lib.ju_process_frame
            self.ins = [R.device_frame(R.FMT_RGBX, w, h, [self.d_in[t].data_ptr()]) for t in range(self.count)]
            self.outs = {n: R.device_frame(R.FMT_RGBX, 4 * w, 4 * h, [self.d_out[n]]) for n in names}
        else:
            self.call = self.lib.ju_process
            self.ins = [R.JuImage(self.d_in[t].data_ptr(), R.LOC_DEVICE, 4 * w, w, h) for t in range(self.count)]
            self.outs = {n: R.JuImage(self.d_out[n].data_ptr(), R.LOC_DEVICE, 16 * w, 4 * w, 4 * h) for n in names}
        torch.cuda.synchronize()

    def run(self, name, frames):
        h = self.rt[name]._h
        t0 = time.perf_counter()
        for t in range(frames):
            if self.call(h, C.byref(self.ins[t % self.count]), C.byref(self.outs[name])) != 0:
                raise RuntimeError(self.lib.ju_last_error().decode())
        return time.perf_counter() - t0                              # (every call is synchronous)

    def close(self):
        for rt in self.rt.values():
            rt.close()


class PassWorkload:
    """Passes of 8 device frames, a group of 8 streams, or a tiled object: the variants over the same device frames.
    run() counts frames: a pass call advances 8, a group call 8 (one per stream), a tiled call 1."""

    def __init__(self, kind, preset, dtype, filt):
        import numpy as np
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        self.R, self.kind, self.rt = R, kind, {}
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16}[dtype]
        h, w = cfg.frame_height, cfg.frame_width
        modes = {"mode0": R.ALPHA_ZERO, "opaque": R.ALPHA_OPAQUE, "source": R.ALPHA_SOURCE}
        self.per_call = 8
        if kind.startswith("tiled"):
            sw, sh = {"tiled_540": (960, 540), "tiled_720": (1280, 720)}[kind]
            self.per_call = 1
            for name, mode in modes.items():
                self.rt[name] = R.TiledRuntime(blob, 0, dt, sw, sh, 16, hooks=True)
                self.rt[name].set_alpha(mode, filt)
            h, w = sh, sw
            names = list(modes)
        else:
            names = ["mode0", "opaque_on", "opaque_off", "source_on", "source_off"]
        clip = M.synthetic_frames(8, h, w, seed=1234, kind="noise").copy()
        clip[..., 3] = np.random.default_rng(5).integers(0, 256, clip.shape[:3], dtype=np.uint8)
        self.d_in = torch.from_numpy(clip).to(dev)
        frames_out = 1 if kind.startswith("tiled") else 8            # (a tiled call writes one frame)
        self.d_out = {n: torch.zeros((frames_out, 4 * h, 4 * w * 4), dtype=torch.uint8, device=dev) for n in names}
        self.calls = {}
        for name in names:
            if kind.startswith("tiled"):
                tr = self.rt[name]
                pair = (R.JuImage(self.d_in[0].data_ptr(), R.LOC_DEVICE, 4 * w, w, h),
                        R.JuImage(self.d_out[name][0].data_ptr(), R.LOC_DEVICE, 16 * w, 4 * w, 4 * h))
                self.calls[name] = (lambda tr=tr, pair=pair: tr.process(*pair))
                continue
            mode = modes[name.split("_")[0]]
            on = 0 if name.endswith("_off") else 1
            if kind == "group":
                rts = [R.Runtime(blob, 0, dt, hooks=True) for _ in range(8)]
                for rt in rts:
                    rt.set_alpha(mode, filt)
                    rt.set_alpha_group(on)
                self.rt[name] = rts
                ins = [rts[k].device_image(self.d_in[k].data_ptr(), w, h) for k in range(8)]
                outs = [rts[k].device_image(self.d_out[name][k].data_ptr(), 4 * w, 4 * h) for k in range(8)]
                self.calls[name] = (lambda rts=rts, ins=ins, outs=outs: R.process_group(rts, ins, outs))
                continue
            rt = R.Runtime(blob, 0, dt, hooks=True)
            rt.set_alpha(mode, filt)
            rt.set_alpha_lookahead(on)
            self.rt[name] = rt
            if kind == "pass_bgrx":
                ins = [rt.device_image(self.d_in[k].data_ptr(), w, h) for k in range(8)]
                outs = [rt.device_image(self.d_out[name][k].data_ptr(), 4 * w, 4 * h) for k in range(8)]
                self.calls[name] = (lambda rt=rt, ins=ins, outs=outs: rt.process_batch(ins, outs))
            else:
                ins = [R.device_frame(R.FMT_RGBX, w, h, [self.d_in[k].data_ptr()]) for k in range(8)]
                outs = [R.device_frame(R.FMT_RGBX, 4 * w, 4 * h, [self.d_out[name][k].data_ptr()]) for k in range(8)]
                self.calls[name] = (lambda rt=rt, ins=ins, outs=outs: rt.process_frames(ins, outs))
        torch.cuda.synchronize()

    def run(self, name, frames):
        call = self.calls[name]
        t0 = time.perf_counter()
        for _ in range(max(1, frames // self.per_call)):
            call()                                                   # (every call is synchronous)
        return (time.perf_counter() - t0) * frames / (max(1, frames // self.per_call) * self.per_call)

    def stats(self, name):
        rt = self.rt[name]
        one = rt[0] if isinstance(rt, list) else rt
        keys = ("alpha_frames",) if self.kind.startswith("tiled") else ("alpha_frames", "lookahead_frames", "lookahead_alpha_frames",
                                                                        "group_frames", "group_alpha_frames", "graph_replays")
        return {k: one.stat(k) for k in keys}

    def close(self):
        for rt in self.rt.values():
            for one in (rt if isinstance(rt, list) else [rt]):
                one.close()


PASS_WORKLOADS = ("pass_bgrx", "pass_rgbx", "group", "tiled_540", "tiled_720")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--filter", default="triangle", choices=sorted(FILTERS))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["frame_rgbx", "process_bgrx"])
    ap.add_argument("--trace", choices=["scale", "fill"])
    ap.add_argument("--summarize", metavar="CSV")
    ap.add_argument("--sink", default="byte", choices=sorted(SINKS))
    ap.add_argument("--size", default="small", choices=sorted(SIZES))
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    filt = FILTERS[args.filter]
    if args.summarize:
        return summarize(args.summarize, args.sink, args.size)
    import torch
    torch.zeros(1, device="cuda:0")                                  # (torch's HIP runtime first, as bench.py does)
    if args.trace:
        return trace(args.trace, args.sink, args.size, filt, args.calls)
    result = {"preset": args.preset, "dtype": args.dtype, "filter": args.filter, "frames": args.frames, "rounds": args.rounds,
              "workloads": {}}
    for kind in args.workloads:
        wl = (PassWorkload if kind in PASS_WORKLOADS else Workload)(kind, args.preset, args.dtype, filt)
        try:
            names = list(wl.rt)
            for name in names:
                wl.run(name, args.warmup)
            fps = {name: [] for name in names}
            for r in range(args.rounds):
                for name in (names if r % 2 == 0 else names[::-1]):  # (no variant always first in a round)
                    fps[name].append(args.frames / wl.run(name, args.frames))
            rows = {}
            for name in names:
                rows[name] = {"median_fps": round(statistics.median(fps[name]), 1), "min_fps": round(min(fps[name]), 1),
                              "max_fps": round(max(fps[name]), 1)}
                if kind in PASS_WORKLOADS:
                    rows[name].update(wl.stats(name))
                else:
                    rows[name].update({"alpha_frames": wl.rt[name].stat("alpha_frames"),
                                       "graph_replays": wl.rt[name].stat("graph_replays")})
            for name in names:
                rows[name]["over_mode0"] = round(rows[name]["median_fps"] / rows["mode0"]["median_fps"], 4)
            result["workloads"][kind] = rows
        finally:
            wl.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
