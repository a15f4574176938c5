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

--compare output --output WxH --filter triangle | catmull-rom | mitchell runs two objects that both advance as group passes:
  output_off:  no output size -- the blended frame of four times the source (the yardstick);
  output_on:   ju_tiled_set_output_size(W, H, filter) -- blend and scale in one launch (docs/tiled.md "An output size");
both with --deep-from-state (with --out-format p010 and 1: the 16-bit route); "output_scaled_frames" shows each one's route.

--compare mask [--mask obs black ...] [--output WxH --filter NAME] runs objects that all advance as group passes, all under
the output size where one is named:
  mask_off:    no mask (the yardstick: today's route);
  mask_obs:    ju_tiled_set_source_mask with tests/golden/obs_mask.png -- a HUD: the box is a few per cent of the frame;
  mask_black:  a black mask -- every pixel is rewritten with the source;
  mask_grey:   random grey levels at the source size -- every pixel blended;
  mask_none:   no mask again, a second yardstick at another place in the round (what the place alone costs);
"source_mask_frames" and "mask_box" show each one's route (docs/tiled.md "A mask").

--compare pass [--place host | device] [--in-format bgrx | nv12] [--out-format ...] [--pass-frames N] [--output WxH] runs
three objects of one model (docs/tiled.md "Look-ahead passes"), over N input and N output buffers each, host (pageable numpy
memory) or device:
  frame:  ju_tiled_process_frame, frame by frame (the yardstick);
  pass:   ju_tiled_process_frames in calls of N frames (default 8);
  frame_last:  frame by frame again, a second yardstick at the END of the round (what the place in the round alone costs:
          docs/tiled.md "A mask" met 1.5 % between the first and the last place);
"pass_frames", "pass_split_launches" and "pass_overlapped_copies" show each one's route.  With --pass-frames N, --trace runs
the `pass` variant alone.

--trace WxH runs one variant alone (--deep-from-state 0 | 1, --scene off | report | reset, --mask KIND, --out-format, --clip,
--output and --filter: the output size set) for a `rocprofv3 --kernel-trace --stats` run; with --two-launch and --mask no
mask is set and every frame is followed by mask_blend_kernel alone, through its hook, over the blended BGRX frame the object
wrote (and with --output by the scaler below: the route of three launches); with --two-launch the output size is NOT
set and every frame is followed by the existing scaler alone, through its hook, at the sizes --output names: scale_bgrx_kernel
over the blended BGRX frame, or (an --out-format other than bgrx) scale_state_kernel over a state of the blended size --
what a route of two launches would add to the blend;
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
TILE_KERNELS = ("tile_split_kernel", "tile_split_frames_kernel", "tile_split_scene_kernel", "scene_clear_tiles_kernel", "tile_stitch_kernel", "tile_stitch_state_kernel", "frame16_to_yuv420p10_kernel",
                "bgrx_to_yuv420p10_kernel", "tile_stitch_scale_kernel", "tile_stitch_scale_state_kernel", "scale_bgrx_kernel", "scale_state_kernel",
                "tile_stitch_mask_kernel", "tile_stitch_mask_scale_kernel", "mask_blend_kernel")
# what a variant is: created under JU_LOOKAHEAD=1 (no passes), its ju_tiled_set_deep_from_state, its scene mode
VARIANTS = {"tiled": (False, 0, 0), "serial": (True, 0, 0), "deep_off": (False, 0, 0), "deep_on": (False, 1, 0),
            "scene_off": (False, 0, 0), "scene_report": (False, 0, 1), "scene_reset": (False, 0, 2),
            "output_off": (False, 0, 0), "output_on": (False, 0, 0),
            "mask_off": (False, 0, 0), "mask_obs": (False, 0, 0), "mask_black": (False, 0, 0), "mask_grey": (False, 0, 0), "mask_none": (False, 0, 0)}
MASKS = ("obs", "black", "grey", "none")
FILTERS = {"triangle": 0, "catmull-rom": 2, "mitchell": 3}
SCENE_NAMES = {"off": "scene_off", "report": "scene_report", "reset": "scene_reset"}
# output formats: (the runtime's FMT_ name, per plane (rows per output row, bytes per output pixel of a row))
OUT_FORMATS = {"bgrx": ("FMT_BGRX", [(1, 4)]), "nv12": ("FMT_NV12", [(1, 1), (0.5, 1)]), "p010": ("FMT_P010", [(1, 2), (0.5, 2)]),
               "i410": ("FMT_I410", [(1, 2)] * 3), "bgrx64": ("FMT_BGRX64", [(1, 8)]), "rgbph": ("FMT_RGBPH", [(1, 2)] * 3)}


def size(text):
    w, h = (int(v) for v in text.lower().split("x"))
    return w, h


def kernel_bytes(sw, sh, w, h, ov, output=None, frames=8):
    """The bytes each kernel must move (output: (OW, OH) for the kernels of an output size -- a fused kernel reads what
    the stitch reads and writes the scaled frame, the scaler alone reads the blended frame and writes the scaled one; 4
    bytes per pixel for the 8-bit kernels, 8 for the 16-bit ones): the split reads the source once and writes every tile; the stitch reads every
    output pixel once where one tile covers it -- and the seams' pixels from two or four -- and writes the frame; the
    stitch of the states the same at 8 bytes per pixel; a P010 encode reads its frame (8 or 4 bytes per pixel) and writes
    3 bytes per pixel.  The split with the detector also reads and rewrites the kept source-size frame; the conditional
    clear reads one flag word per workgroup while no cut is flagged (its bytes at a cut depend on the model: not listed).
    The split of a look-ahead pass moves the split's bytes once per frame of the pass (`frames`)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tiled_reference as T
    nx, ny = len(T.origins(sw, w, ov)), len(T.origins(sh, h, ov))

    def reads(S, t):                                                # tile reads per output coordinate, summed over the axis
        _, _, q = T.layout(S, t, ov)
        return int((1 + (q != 0)).sum())
    split = 4 * sw * sh + 4 * w * h * nx * ny
    stitch = 4 * reads(sw, w) * reads(sh, h) + 64 * sw * sh
    scaled = {}
    if output:
        out_px, read = output[0] * output[1], reads(sw, w) * reads(sh, h)
        scaled = {"tile_stitch_scale_kernel": 4 * read + 4 * out_px, "tile_stitch_scale_state_kernel": 8 * read + 8 * out_px,
                  "scale_bgrx_kernel": 64 * sw * sh + 4 * out_px, "scale_state_kernel": 128 * sw * sh + 8 * out_px}
        # (the encode then runs at one of two sizes, which a stats file does not tell: its time alone)
        return {**scaled, "tiles": [nx, ny], "tile_split_kernel": split, "tile_split_frames_kernel": frames * split, "tile_split_scene_kernel": split + 8 * sw * sh,
                "tile_stitch_kernel": stitch, "tile_stitch_state_kernel": 2 * stitch}
    return {"tiles": [nx, ny], "tile_split_kernel": split, "tile_split_frames_kernel": frames * split, "tile_split_scene_kernel": split + 8 * sw * sh, "tile_stitch_kernel": stitch, "tile_stitch_state_kernel": 2 * stitch,
            "frame16_to_yuv420p10_kernel": (8 + 3) * 16 * sw * sh, "bgrx_to_yuv420p10_kernel": (4 + 3) * 16 * sw * sh}


def summarize(path, sw, sh, w, h, ov, output=None, frames=8):
    import re
    need = kernel_bytes(sw, sh, w, h, ov, output, frames)
    out = {"stats": path, "source": f"{sw}x{sh}", "tiles": need["tiles"], "copy_bandwidth_TBps": COPY_BYTES_PER_S / 1e12}
    if output:
        out["output"] = f"{output[0]}x{output[1]}"
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in TILE_KERNELS:
                # (the whole name: some end in another's; a name left mangled carries it behind its length)
                if re.search(r"(^|[^A-Za-z0-9_])" + k + r"($|[^A-Za-z0-9_])", r["Name"]) or \
                        (r["Name"].startswith("_Z") and f"{len(k)}{k}" in r["Name"]):
                    us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"])
                    if k not in need:
                        out[k] = {"calls": int(r["Calls"]), "us_per_call": round(us, 2)}
                        continue
                    least = need[k] / COPY_BYTES_PER_S * 1e6
                    out[k] = {"calls": int(r["Calls"]), "us_per_call": round(us, 2), "bytes": need[k],
                              "least_us_at_copy_bandwidth": round(least, 2), "share_of_copy_bandwidth": round(least / us, 3)}
    print(json.dumps(out))


def make_mask(kind, sw, sh):
    """The BGRX mask of a variant: the reference's HUD mask, all black, or random grey levels at the source size."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if kind == "obs":
        import source_reference as S
        return S.read_png_palette_1bit(os.path.join(ROOT, "tests", "golden", "obs_mask.png"))
    if kind == "black":
        return np.zeros((2, 2, 4), np.uint8)
    return np.random.default_rng(77).integers(0, 256, (sh, sw, 4), dtype=np.uint8)


class Pair:
    """The variants for one source size, with their device frames."""

    def __init__(self, sw, sh, preset, dtype, ov, names=("tiled", "serial"), out_format="bgrx", clip="noise", threshold=10000,
                 output=None, deep=None, two_launch=None, two_mask=None):
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[dtype]
        self.obj = {}
        deep_all = deep
        for name in names:
            serial, deep, scene = VARIANTS[name]
            if serial:
                os.environ["JU_LOOKAHEAD"] = "1"
            try:
                self.obj[name] = R.TiledRuntime(blob, 0, dt, sw, sh, ov, hooks=two_launch is not None or two_mask is not None)
            finally:
                os.environ.pop("JU_LOOKAHEAD", None)
            self.obj[name].set_deep_from_state(deep_all if deep_all is not None else deep)
            if output and name != "output_off":
                self.obj[name].set_output_size(*output)
            if scene:
                self.obj[name].set_scene_detect(scene, threshold)
            if name.startswith("mask_") and name not in ("mask_off", "mask_none"):
                self.obj[name].set_source_mask(make_mask(name[len("mask_"):], sw, sh))
        if clip == "cuts":
            import numpy as np
            clip = np.ascontiguousarray(np.concatenate([M.synthetic_frames(4, sh, sw, seed=seed, kind="smooth")
                                                        for seed in (1, 2, 3, 4)], axis=0))
        else:
            clip = M.synthetic_frames(4, sh, sw, seed=1234, kind="noise")
        self.count = len(clip)
        self.d_in = torch.from_numpy(clip).to(dev)
        fmt_name, planes = OUT_FORMATS[out_format]
        self.frames = out_format != "bgrx"       # (ju_tiled_process_frame; else ju_tiled_process on two images)
        self.d_out, self.out = {}, {}
        for name, o in self.obj.items():         # (each variant's frames at the size it hands out)
            fw, fh = o.frame_output_size()
            self.d_out[name] = [torch.zeros((int(fh * rows), fw * width), dtype=torch.uint8, device=dev) for rows, width in planes]
            if self.frames:
                self.out[name] = R.device_frame(getattr(R, fmt_name), fw, fh, self.d_out[name])
            else:
                self.out[name] = R.JuImage(self.d_out[name][0].data_ptr(), R.LOC_DEVICE, 4 * fw, fw, fh)
        if self.frames:
            self.ins = [R.device_frame(R.FMT_BGRX, sw, sh, [self.d_in[t].data_ptr()]) for t in range(self.count)]
        else:
            self.ins = [R.JuImage(self.d_in[t].data_ptr(), R.LOC_DEVICE, 4 * sw, sw, sh) for t in range(self.count)]
        self.lib = next(iter(self.obj.values()))._lib
        # --two-launch: the existing scaler alone behind every frame (its hook), blended size -> (OW, OH, filter)
        self.two = None
        if two_launch is not None:
            ow, oh, filt = two_launch
            op = 1 if self.frames else 0
            src = torch.zeros((4 * sh, 4 * sw * 8), dtype=torch.uint8, device=dev) if op else self.d_out[names[0]][0]
            dst = torch.zeros((oh, ow * (8 if op else 4)), dtype=torch.uint8, device=dev)
            self.two = (op, filt, dst, 4 * ow, ow, oh, src, 16 * sw, 4 * sw, 4 * sh)
        # --two-launch --mask: mask_blend_kernel alone behind every frame (its hook), over the blended frame just written
        self.two_mask = None
        if two_mask is not None:
            m = make_mask(two_mask, sw, sh)
            self.two_mask = (torch.from_numpy(m.copy()).to(dev), m.shape[1], m.shape[0], self.d_out[names[0]][0], sw, sh)
        torch.cuda.synchronize()

    def run(self, name, frames):
        h = self.obj[name]._h
        call = self.lib.ju_tiled_process_frame if self.frames else self.lib.ju_tiled_process
        t0 = time.perf_counter()
        for t in range(frames):
            if call(h, C.byref(self.ins[t % self.count]), C.byref(self.out[name])) != 0:
                raise RuntimeError(self.lib.ju_last_error().decode())
            if self.two_mask:
                d_mask, mw, mh, gen, sw, sh = self.two_mask
                if self.lib.ju_debug_source(1, gen.data_ptr(), 16 * sw, 4 * sw, 4 * sh, self.d_in[t % self.count].data_ptr(), 4 * sw, sw, sh,
                                            d_mask.data_ptr(), 4 * mw, mw, mh) != 0:
                    raise RuntimeError(self.lib.ju_last_error().decode())
            if self.two:
                op, filt, dst, stride, ow, oh, src, src_stride, bw, bh = self.two
                if self.lib.ju_debug_scale(op, filt, dst.data_ptr(), stride, ow, oh, src.data_ptr(), src_stride, bw, bh, None, None, None) != 0:
                    raise RuntimeError(self.lib.ju_last_error().decode())
        return time.perf_counter() - t0          # (every call is synchronous)

    def close(self):
        for o in self.obj.values():
            o.close()


class PassPair:
    """--compare pass: `frame` (ju_tiled_process_frame) and `pass` (ju_tiled_process_frames in calls of n frames), each over
    n input and n output buffers of its own, host or device."""

    def __init__(self, sw, sh, preset, dtype, ov, place, in_format, out_format, output, n, names=("frame", "pass", "frame_last")):
        import numpy as np
        import torch
        from joshupscale_amd import model_file as M
        from joshupscale_amd import runtime as R
        dev = torch.device("cuda", 0)
        cfg = M.PRESETS[preset]
        blob = M.serialize(cfg, M.make_seeded_weights(cfg))
        dt = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[dtype]
        self.n, self.obj, self.keep, self.ins, self.outs = n, {}, [], {}, {}
        rng = np.random.default_rng(1234)
        in_name, in_planes = OUT_FORMATS[in_format]
        out_name, out_planes = OUT_FORMATS[out_format]

        def frames_of(fmt_name, planes, w, h, fill):
            out = []
            for _ in range(n):
                arrays = [fill((int(h * rows), w * width)) for rows, width in planes]
                if fmt_name == "FMT_BGRX":
                    arrays = [arrays[0].reshape(h, w, 4)]
                elif planes[0][1] == 2:                            # (the 10-bit formats: 16-bit samples)
                    arrays = [a.view(np.uint16) for a in arrays]
                if place == "host":
                    self.keep.append(arrays)
                    out.append(R.host_frame(getattr(R, fmt_name), arrays))
                else:
                    tensors = [torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1)).to(dev) for a in arrays]
                    self.keep.append(tensors)
                    out.append(R.device_frame(getattr(R, fmt_name), w, h, tensors))
            return (R.JuFrame * n)(*out)
        for name in names:
            o = self.obj[name] = R.TiledRuntime(blob, 0, dt, sw, sh, ov)
            if output:
                o.set_output_size(*output)
            fw, fh = o.frame_output_size()
            self.ins[name] = frames_of(in_name, in_planes, sw, sh, lambda shape: rng.integers(0, 256, shape, dtype=np.uint8))
            self.outs[name] = frames_of(out_name, out_planes, fw, fh, lambda shape: np.zeros(shape, np.uint8))
        self.lib = next(iter(self.obj.values()))._lib
        torch.cuda.synchronize()

    def run(self, name, frames):
        h, ins, outs, n = self.obj[name]._h, self.ins[name], self.outs[name], self.n
        assert frames % n == 0
        t0 = time.perf_counter()
        if name == "pass":
            for _ in range(frames // n):
                if self.lib.ju_tiled_process_frames(h, ins, outs, n) != 0:
                    raise RuntimeError(self.lib.ju_last_error().decode())
        else:
            for t in range(frames):
                if self.lib.ju_tiled_process_frame(h, C.byref(ins[t % n]), C.byref(outs[t % n])) != 0:
                    raise RuntimeError(self.lib.ju_last_error().decode())
        return time.perf_counter() - t0          # (every call is synchronous)

    def stats(self, name):
        keys = ("frames", "group_frames", "lookahead", "pass_calls", "pass_frames", "pass_split_launches", "pass_overlapped_copies",
                "output_scaled_frames")
        return {k: self.obj[name].stat(k) for k in keys}

    def close(self):
        for o in self.obj.values():
            o.close()


def compare_pass(args, output):
    res = {}
    for text in args.sizes:
        sw, sh = size(text)
        p = PassPair(sw, sh, args.preset, args.dtype, args.overlap, args.place, args.in_format, args.out_format, output, args.pass_frames)
        for name in p.obj:
            p.run(name, args.warmup)
        fps = {name: [] for name in p.obj}
        for _ in range(args.rounds):
            for name in p.obj:
                fps[name].append(args.frames / p.run(name, args.frames))
        row = {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for name, v in fps.items()}
        row["pass_over_frame"] = round(row["pass"]["median"] / row["frame"]["median"], 4)
        row["pass_over_frame_last"] = round(row["pass"]["median"] / row["frame_last"]["median"], 4)
        row["stats"] = {name: p.stats(name) for name in p.obj}
        res[text] = row
        p.close()
    print(json.dumps({"metric": "frames/s of a tiled object, " + args.place + " " + args.in_format.upper() + " in, " + args.place + " " +
                      args.out_format.upper() + " out", "preset": args.preset, "dtype": args.dtype, "overlap": args.overlap,
                      "frames_per_round": args.frames, "rounds": args.rounds, "pass_frames": args.pass_frames, "output": args.output,
                      "filter": args.filter if args.output else None,
                      "variants": {"frame": "ju_tiled_process_frame, frame by frame, first in the round",
                                   "pass": "ju_tiled_process_frames in calls of " + str(args.pass_frames) + " frames",
                                   "frame_last": "frame by frame again, last in the round"}, "fps": res}))


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
    ap.add_argument("--place", default="device", choices=["host", "device"], help="--compare pass, --trace --pass-frames: where the frames lie")
    ap.add_argument("--in-format", default="bgrx", choices=["bgrx", "nv12"], help="--compare pass, --trace --pass-frames: the input frames' format")
    ap.add_argument("--pass-frames", type=int, default=None, metavar="N",
                    help="--compare pass: frames per ju_tiled_process_frames call (default 8); --trace: run the pass variant alone")
    ap.add_argument("--compare", default="passes", choices=["passes", "deep", "scene", "output", "mask", "pass"],
                    help="passes: tiled against serial; deep: ju_tiled_set_deep_from_state 0 against 1; scene: the scene "
                         "detector off, JU_SCENE_REPORT and JU_SCENE_RESET; output: no output size against --output; "
                         "mask: no mask against the masks of --mask (all under --output where given)")
    ap.add_argument("--mask", nargs="+", default=None, choices=MASKS,
                    help="--compare mask: the masks to run beside no mask (default obs black); --trace: the one mask set")
    ap.add_argument("--output", default=None, metavar="WxH", help="--compare output, --trace, --summarize: the output size")
    ap.add_argument("--filter", default="triangle", choices=sorted(FILTERS), help="the output size's filter")
    ap.add_argument("--two-launch", action="store_true", help="--trace: the existing scaler alone behind every frame")
    ap.add_argument("--scene", default="off", choices=sorted(SCENE_NAMES), help="--trace: the scene mode of the one variant")
    ap.add_argument("--clip", default="noise", choices=["noise", "cuts"])
    ap.add_argument("--threshold", type=int, default=10000, help="threshold_milli of the scene detector")
    ap.add_argument("--deep-from-state", type=int, default=0, choices=[0, 1],
                    help="--trace: the setting of the one variant; --compare output: of both")
    ap.add_argument("--trace", default=None, metavar="WxH")
    ap.add_argument("--summarize", nargs=2, metavar=("CSV", "WxH"), default=None)
    args = ap.parse_args()
    from joshupscale_amd import model_file as M
    cfg = M.PRESETS[args.preset]
    if args.summarize:
        summarize(args.summarize[0], *size(args.summarize[1]), cfg.frame_width, cfg.frame_height, args.overlap,
                  size(args.output) if args.output else None, args.pass_frames or 8)
        return
    output = (*size(args.output), FILTERS[args.filter]) if args.output else None
    if (args.compare == "output" or (args.two_launch and not args.mask)) and not output:
        ap.error("--compare output and --two-launch without --mask need --output WxH")
    import torch
    torch.zeros(1, device="cuda:0")  # (torch's HIP runtime first, as bench.py does)
    if args.compare == "pass" or (args.trace and args.pass_frames):
        args.pass_frames = args.pass_frames or 8
        if args.pass_frames < 1 or args.frames % args.pass_frames or args.warmup % args.pass_frames:
            ap.error("--frames and --warmup must be multiples of --pass-frames")
    if args.trace and args.pass_frames:
        p = PassPair(*size(args.trace), args.preset, args.dtype, args.overlap, args.place, args.in_format, args.out_format, output,
                     args.pass_frames, names=("pass",))
        p.run("pass", args.warmup)
        p.run("pass", args.frames)
        print(json.dumps({"trace": args.trace, "variant": "pass", "place": args.place, "in_format": args.in_format,
                          "out_format": args.out_format, "frames": args.warmup + args.frames, "output": args.output, **p.stats("pass")}))
        p.close()
        return
    if args.compare == "pass":
        return compare_pass(args, output)
    if args.trace:
        name = "deep_on" if args.deep_from_state else SCENE_NAMES[args.scene] if args.scene != "off" else "tiled"
        if args.mask and not args.two_launch:
            name = "mask_" + args.mask[0]
        p = Pair(*size(args.trace), args.preset, args.dtype, args.overlap, (name,), args.out_format, args.clip, args.threshold,
                 output=None if args.two_launch else output, two_launch=output if args.two_launch else None,
                 two_mask=args.mask[0] if args.mask and args.two_launch else None)
        p.run(name, args.warmup)
        p.run(name, args.frames)
        print(json.dumps({"trace": args.trace, "variant": name, "out_format": args.out_format, "frames": args.warmup + args.frames,
                          "output": args.output, "filter": args.filter, "two_launch": args.two_launch, "mask": args.mask,
                          "source_mask_frames": p.obj[name].stat("source_mask_frames"),
                          "output_scaled_frames": p.obj[name].stat("output_scaled_frames"),
                          "group_frames": p.obj[name].stat("group_frames"),
                          "deep_state_frames": p.obj[name].stat("deep_state_frames"), "clip": args.clip,
                          "scene_cuts": p.obj[name].stat("scene_cuts")}))
        p.close()
        return
    res = {}
    names = {"deep": ("deep_off", "deep_on"), "scene": ("scene_off", "scene_report", "scene_reset"),
             "output": ("output_off", "output_on"),
             "mask": ("mask_off",) + tuple("mask_" + m for m in (args.mask or ("obs", "black")))}.get(args.compare, ("tiled", "serial"))
    for text in args.sizes:
        sw, sh = size(text)
        p = Pair(sw, sh, args.preset, args.dtype, args.overlap, names, args.out_format, args.clip, args.threshold,
                 output=output if args.compare in ("output", "mask") else None,
                 deep=args.deep_from_state if args.compare == "output" else None)
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
        if args.compare == "output":
            row["output_scaled_frames"] = {name: o.stat("output_scaled_frames") for name, o in p.obj.items()}
            row["output"], row["filter"], row["deep_from_state"] = args.output, args.filter, args.deep_from_state
        if args.compare == "mask":
            row["source_mask_frames"] = {name: o.stat("source_mask_frames") for name, o in p.obj.items()}
            row["mask_box"] = {name: [int(o.stat("mask_box_" + k)) for k in ("x0", "y0", "x1", "y1")] for name, o in p.obj.items()}
            row["output_scaled_frames"] = {name: o.stat("output_scaled_frames") for name, o in p.obj.items()}
            row["output"], row["filter"] = args.output, args.filter
        res[text] = row
        p.close()
    what = {"tiled": "the tiles as group passes", "serial": "the same object created under JU_LOOKAHEAD=1: every tile "
            "through ju_process, the same two kernels", "deep_off": "ju_tiled_set_deep_from_state 0: a deep format from the "
            "blended 8-bit frame", "deep_on": "ju_tiled_set_deep_from_state 1: from the blend of the tiles' f16 states",
            "scene_off": "the scene detector off: the split alone", "scene_report": "JU_SCENE_REPORT: the split and the "
            "detector in one launch", "scene_reset": "JU_SCENE_RESET: that launch and the conditional clear of all tiles",
            "output_off": "no output size: the blended frame of four times the source",
            "output_on": "ju_tiled_set_output_size: blend and scale in one launch",
            "mask_off": "no mask: the unmasked launches", "mask_obs": "ju_tiled_set_source_mask, the reference's HUD mask: the "
            "box is a few per cent of the frame", "mask_black": "a black mask: every pixel rewritten with the source",
            "mask_grey": "random grey levels at the source size: every pixel blended",
            "mask_none": "no mask, as mask_off: a second yardstick at another place in the round"}
    print(json.dumps({"metric": "frames/s of ju_tiled_process, device BGRX in, device " + args.out_format.upper() + " out",
                      "preset": args.preset, "dtype": args.dtype, "overlap": args.overlap, "frames_per_round": args.frames,
                      "rounds": args.rounds, "clip": args.clip, "variants": {name: what[name] for name in names}, "fps": res}))


if __name__ == "__main__":
    main()
