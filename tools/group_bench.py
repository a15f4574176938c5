"""Aggregate frames/s of N live streams on one GPU, psp-quality at full size, seeded weights, device frames.

For N in --sizes (default 1 2 4 8), N runtimes of the same model each take one frame per tick, three ways:
  (a) group:    ju_process_group over the N runtimes (one call per tick);
  (b) serial:   ju_process on each runtime in turn, from one thread;
  (c) threads:  N threads, each running ju_process on its own runtime.
The methods and sizes run alternately, round after round, in one process (the clock and the machine's other work are
shared alike), after a warm-up of every (method, N).  Prints one JSON line: per (N, method) the median, min and max
over the rounds, and (a) / (b) per N.  Every device pair is registered with ju_prepare_frames first, as bench.py does,
so (b) and (c) replay their graphs; group passes launch eagerly.

--scene report|reset turns every runtime's scene detector on (threshold_milli 22000) and times
  group: ju_process_group with ju_set_scene_group(rt, 1) (the detector rides in the passes: two launches per pass),
  group_off: the same call with the setting at 0 (every member on its own, two detector launches per frame),
  serial: ju_process per runtime.
--format nv12 hands over device NV12 frames on both sides and times
  group: ju_process_group_frames, serial: ju_process_frame per runtime.
Both may be combined; neither runs the threads method.
--source WxH / --output WxH / --mask put every stream under ju_set_source_size / ju_set_output_size / ju_set_source_mask
(frames are then handed over at those sizes through ju_process_group_frames, in --format's format) and time
  group: ju_set_stage_group(rt, 1) (the members ride, the pass carries their stages),
  group_off: the same call with the setting at 0 (every member on its own, on the staged single-frame route),
  serial: ju_process_frame per runtime.

--trace group|single runs one method alone for a `rocprofv3 --kernel-trace --stats` run: N = 8 group calls, or the
same number of frames through ju_process on one runtime.  --summarize <kernel_stats.csv> <frames> prints the flow
net's kernel time per frame of such a run."""

import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the flow net's kernels in psp-quality's plan (the generator's tower, warp and tail are other kernels)
FLOW_KERNELS = ("flow_block_kernel", "conv_splitk_kernel", "upsample2_kernel")


def summarize(path, frames):
    total = flow = 0.0
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            total += ns
            if any(k in r["Name"] for k in FLOW_KERNELS):
                flow += ns
            rows.append((r["Name"][:90], int(r["Calls"]), round(ns / 1e3 / frames, 2)))
    print(json.dumps({"stats": path, "frames": frames, "flow_us_per_frame": round(flow / 1e3 / frames, 2),
                      "all_kernels_us_per_frame": round(total / 1e3 / frames, 2),
                      "kernels_us_per_frame": sorted(rows, key=lambda x: -x[2])}))


class Streams:
    def __init__(self, n, preset, dtype, inputs_per_stream=4, scene="off", fmt="bgrx", source=None, output=None, mask=False):
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        self.R = R
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        h, w = cfg.frame_height, cfg.frame_width
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[dtype]
        self.rts = [R.Runtime(blob, 0, dt, hooks=False) for _ in range(n)]
        clip = M.synthetic_frames(n * inputs_per_stream, h, w, seed=1234, kind="noise")
        self.d_in = torch.from_numpy(clip).to(dev).view(n, inputs_per_stream, h, w, 4)
        self.d_out = torch.zeros((n, 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        self.k = inputs_per_stream
        # images[i][t]: stream i's pair at tick t % k
        self.ins = [[R.JuImage(self.d_in[i][t].data_ptr(), R.LOC_DEVICE, 4 * w, w, h) for t in range(self.k)]
                    for i in range(n)]
        self.outs = [R.JuImage(self.d_out[i].data_ptr(), R.LOC_DEVICE, 16 * w, 4 * w, 4 * h) for i in range(n)]
        for i, rt in enumerate(self.rts):
            for t in range(self.k):
                rt.prepare_frames(self.ins[i][t], self.outs[i])
        self.lib = self.rts[0]._lib
        self.group_args = {}
        self.scene, self.fmt = scene, fmt
        self.staged = bool(source or output or mask)
        self.frames_api = fmt == "nv12" or self.staged
        sw, sh = source or (w, h)                                  # what the frames measure on either side
        ow, oh = output or (4 * w, 4 * h)
        if self.staged:
            import numpy as np
            for rt in self.rts:
                if source:
                    rt.set_source_size(sw, sh)
                if mask:                                           # a HUD strip along the bottom and a corner box stay the source
                    m = np.full((90, 160, 4), 255, np.uint8)
                    m[78:, :, :3] = 0
                    m[4:20, 4:44, :3] = 0
                    rt.set_source_mask(m)
                if output:
                    rt.set_output_size(ow, oh)
        if scene != "off":
            for rt in self.rts:
                rt.set_scene_detect({"report": R.SCENE_REPORT, "reset": R.SCENE_RESET}[scene], 22000)
        if fmt == "nv12":
            # device NV12 on both sides: any bytes are a frame (noise, as the BGRX clip is)
            gen = torch.Generator(device="cpu").manual_seed(1234)
            self.d_y = torch.randint(16, 236, (n, self.k, sh, sw), dtype=torch.uint8, generator=gen).to(dev)
            self.d_uv = torch.randint(16, 241, (n, self.k, sh // 2, sw), dtype=torch.uint8, generator=gen).to(dev)
            self.d_oy = torch.zeros((n, oh, ow), dtype=torch.uint8, device=dev)
            self.d_ouv = torch.zeros((n, oh // 2, ow), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            self.fins = [[R.device_frame(R.FMT_NV12, sw, sh, [self.d_y[i][t], self.d_uv[i][t]]) for t in range(self.k)]
                         for i in range(n)]
            self.fouts = [R.device_frame(R.FMT_NV12, ow, oh, [self.d_oy[i], self.d_ouv[i]]) for i in range(n)]
        elif self.staged:
            # device BGRX at the sizes set, through the frames entry points
            gen = torch.Generator(device="cpu").manual_seed(1234)
            self.d_src = torch.randint(0, 256, (n, self.k, sh, sw, 4), dtype=torch.uint8, generator=gen).to(dev)
            self.d_dst = torch.zeros((n, oh, ow, 4), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            self.fins = [[R.device_frame(R.FMT_BGRX, sw, sh, [self.d_src[i][t]]) for t in range(self.k)] for i in range(n)]
            self.fouts = [R.device_frame(R.FMT_BGRX, ow, oh, [self.d_dst[i]]) for i in range(n)]

    def set_scene_group(self, on):
        """The settings that decide whether the members ride: ju_set_scene_group and, under a stage, ju_set_stage_group."""
        for rt in self.rts:
            if self.scene != "off":
                rt.set_scene_group(on)
            if self.staged:
                rt.set_stage_group(on)

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.ju_last_error().decode())

    def group(self, n, ticks, start=0):
        R = self.R
        key = n
        nv12 = self.frames_api
        if key not in self.group_args:
            hs = (C.c_void_p * n)(*[rt._h.value for rt in self.rts[:n]])
            if nv12:
                per_t = [((R.JuFrame * n)(*[self.fins[i][t] for i in range(n)]), (R.JuFrame * n)(*self.fouts[:n]))
                         for t in range(self.k)]
            else:
                per_t = [((R.JuImage * n)(*[self.ins[i][t] for i in range(n)]), (R.JuImage * n)(*self.outs[:n]))
                         for t in range(self.k)]
            self.group_args[key] = (hs, per_t)
        hs, per_t = self.group_args[key]
        call = self.lib.ju_process_group_frames if nv12 else self.lib.ju_process_group
        for t in range(start, start + ticks):
            a, b = per_t[t % self.k]
            self.check(call(hs, a, b, n))

    group_off = group  # (the same call; timed() leaves ju_set_scene_group at 0 for it)

    def serial(self, n, ticks, start=0):
        nv12 = self.frames_api
        call = self.lib.ju_process_frame if nv12 else self.lib.ju_process
        ins, outs = (self.fins, self.fouts) if nv12 else (self.ins, self.outs)
        refs = [[(self.rts[i]._h, C.byref(ins[i][t]), C.byref(outs[i])) for t in range(self.k)] for i in range(n)]
        for t in range(start, start + ticks):
            for i in range(n):
                self.check(call(*refs[i][t % self.k]))

    def threads(self, n, ticks, start=0):
        call = self.lib.ju_process
        barrier = threading.Barrier(n + 1)
        errors = []

        def run(i):
            refs = [(self.rts[i]._h, C.byref(self.ins[i][t]), C.byref(self.outs[i])) for t in range(self.k)]
            barrier.wait()
            for t in range(start, start + ticks):
                if call(*refs[t % self.k]) != 0:
                    errors.append(self.lib.ju_last_error().decode())
                    return

        ths = [threading.Thread(target=run, args=(i,)) for i in range(n)]
        for th in ths:
            th.start()
        barrier.wait()
        t0 = time.perf_counter()
        for th in ths:
            th.join()
        dt = time.perf_counter() - t0
        if errors:
            raise RuntimeError(errors[0])
        return dt

    def close(self):
        for rt in self.rts:
            rt.close()


def timed(streams, method, n, ticks):
    if method == "threads":
        return streams.threads(n, ticks)
    streams.set_scene_group(1 if method == "group" else 0)  # (waits for the stream: outside the timed region)
    t0 = time.perf_counter()
    getattr(streams, method)(n, ticks)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp8"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=256, help="frames per (method, N) and round, all streams together")
    ap.add_argument("--warmup", type=int, default=16, help="ticks of every (method, N) before the first round")
    ap.add_argument("--trace", choices=["group", "single"], default=None)
    ap.add_argument("--ticks", type=int, default=64, help="--trace: timed ticks after a warm-up of as many")
    ap.add_argument("--scene", choices=["off", "report", "reset"], default="off")
    ap.add_argument("--format", choices=["bgrx", "nv12"], default="bgrx")
    ap.add_argument("--source", default=None, metavar="WxH", help="ju_set_source_size on every stream")
    ap.add_argument("--output", default=None, metavar="WxH", help="ju_set_output_size on every stream")
    ap.add_argument("--mask", action="store_true", help="ju_set_source_mask on every stream")
    ap.add_argument("--summarize", nargs=2, metavar=("CSV", "FRAMES"), default=None)
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize[0], int(args.summarize[1]))
        return
    size = lambda text: tuple(int(v) for v in text.lower().split("x")) if text else None  # noqa: E731
    stage = dict(source=size(args.source), output=size(args.output), mask=args.mask)
    staged = bool(args.source or args.output or args.mask)
    import torch
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first, as bench.py does)
    if args.trace:
        s = Streams(8 if args.trace == "group" else 1, args.preset, args.dtype, scene=args.scene, fmt=args.format, **stage)
        s.set_scene_group(1)
        if args.trace == "group":
            s.group(8, args.ticks)
            s.group(8, args.ticks)
            frames = 8 * args.ticks
        else:
            s.serial(1, 8 * args.ticks)
            s.serial(1, 8 * args.ticks)
            frames = 8 * args.ticks
        print(json.dumps({"trace": args.trace, "frames_per_half": frames,
                          "group_frames": s.rts[0].stat("group_frames"),
                          "group_staged_frames": s.rts[0].stat("group_staged_frames")}))
        s.close()
        return
    s = Streams(max(args.sizes), args.preset, args.dtype, scene=args.scene, fmt=args.format, **stage)
    methods = ("group", "serial", "threads")
    if args.scene != "off" or staged:
        methods = ("group", "group_off", "serial")
    elif args.format != "bgrx":
        methods = ("group", "serial")
    for n in args.sizes:
        for m in methods:
            timed(s, m, n, args.warmup)
    fps = {(n, m): [] for n in args.sizes for m in methods}
    for _ in range(args.rounds):
        for n in args.sizes:
            ticks = max(args.frames // n, 8)
            for m in methods:
                fps[(n, m)].append(n * ticks / timed(s, m, n, ticks))
    res = {}
    for n in args.sizes:
        row = {}
        for m in methods:
            v = fps[(n, m)]
            row[m] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
        row["group_over_serial"] = round(row["group"]["median"] / row["serial"]["median"], 3)
        if "threads" in row:
            row["group_over_threads"] = round(row["group"]["median"] / row["threads"]["median"], 3)
        if "group_off" in row:
            row["group_over_group_off"] = round(row["group"]["median"] / row["group_off"]["median"], 3)
        res[str(n)] = row
    group_frames = [rt.stat("group_frames") for rt in s.rts]
    extra = {"scene": args.scene, "format": args.format, "source": args.source, "output": args.output, "mask": args.mask,
             "group_staged_frames": [rt.stat("group_staged_frames") for rt in s.rts],
             "scene_group_frames": [rt.stat("scene_group_frames") for rt in s.rts],
             "group_yuv_frames": [rt.stat("group_yuv_frames") for rt in s.rts],
             "scene_cuts": [rt.stat("scene_cuts") for rt in s.rts]}
    s.close()
    print(json.dumps({"metric": "aggregate frames/s of N streams on one GPU", "preset": args.preset, "dtype": args.dtype,
                      "frames_per_round": args.frames, "rounds": args.rounds,
                      "methods": {"group": "ju_process_group (ju_process_group_frames for --format nv12 or under a stage; "
                                           "ju_set_scene_group / ju_set_stage_group 1)",
                                  "group_off": "the same call with ju_set_scene_group / ju_set_stage_group 0: detecting or "
                                               "staged members on their own",
                                  "serial": "ju_process (ju_process_frame) per runtime, one thread",
                                  "threads": "one thread per runtime, ju_process"},
                      "fps": res, "group_frames": group_frames, **extra}))


if __name__ == "__main__":
    main()
