"""Per-call frames/s of ju_process_frame on BGRX, NV12 and I420 frames, host and device, psp-quality at 480x270.

Every variant goes through the same runtime in turn (interleaved rounds of --frames-per-round frames), each call
synchronous (ju_process_frame / ju_process), so that the clock and the other work on the machine are shared alike.
Prints one JSON line.  --kernels instead runs the two conversion kernels alone at --kernel-size (default 1920x1080)
through ju_debug_yuv, for a `rocprofv3 --kernel-trace --stats` run (the test flavour of the library is needed)."""

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
import yuv_reference as Y  # noqa: E402

FORMATS = {"bgrx": R.FMT_BGRX, "nv12": R.FMT_NV12, "i420": R.FMT_I420}


def planes_for(fmt, h, w, bgrx, cs):
    if fmt == R.FMT_BGRX:
        return [bgrx]
    y, u, v = Y.encode(bgrx, cs)
    return [y, Y.to_nv12(u, v)] if fmt == R.FMT_NV12 else [y, u, v]


def empty_planes(fmt, h, w):
    if fmt == R.FMT_BGRX:
        return [np.zeros((h, w, 4), np.uint8)]
    if fmt == R.FMT_NV12:
        return [np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)]
    return [np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)]


def frame_bench(args):
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = R.CS_BT709_LIMITED
    clip = M.synthetic_frames(8, h, w, seed=1234, kind="smooth")
    variants = {}
    keep = []
    rt = R.Runtime(blob, 0, {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[args.dtype], hooks=False)
    for name, fmt in FORMATS.items():
        for loc in ("host", "device"):
            pairs = []
            for f in clip:
                pin = planes_for(fmt, h, w, f, cs)
                pout = empty_planes(fmt, 4 * h, 4 * w)
                if loc == "host":
                    keep.append((pin, pout))
                    pairs.append((R.host_frame(fmt, pin, cs), R.host_frame(fmt, pout, cs)))
                else:
                    din = [torch.from_numpy(p).to(dev) for p in pin]
                    dout = [torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in pout]
                    keep.append((din, dout))
                    pairs.append((R.device_frame(fmt, w, h, din, colorspace=cs),
                                  R.device_frame(fmt, 4 * w, 4 * h, dout, colorspace=cs)))
            if fmt == R.FMT_BGRX and loc == "device":
                for a, b in pairs:   # the direct device path's graphs, as bench.py registers its buffers
                    rt.prepare_frames(R.JuImage(a.planes[0], R.LOC_DEVICE, a.strides[0], w, h),
                                      R.JuImage(b.planes[0], R.LOC_DEVICE, b.strides[0], 4 * w, 4 * h))
            variants[f"{name}_{loc}"] = [(C.byref(a), C.byref(b)) for a, b in pairs]
    torch.cuda.synchronize()
    lib, handle = rt._lib, rt._h
    call = lib.ju_process_frame
    for name, refs in variants.items():         # warm-up: every variant, every buffer
        for _ in range(args.warmup):
            for a, b in refs:
                if call(handle, a, b) != 0:
                    raise RuntimeError(lib.ju_last_error().decode())
    times = {k: 0.0 for k in variants}
    frames = {k: 0 for k in variants}
    for _ in range(args.rounds):
        for name, refs in variants.items():
            n = args.frames_per_round
            t0 = time.perf_counter()
            for i in range(n):
                a, b = refs[i % len(refs)]
                call(handle, a, b)
            times[name] += time.perf_counter() - t0
            frames[name] += n
    err = lib.ju_last_error().decode()
    rt.close()
    fps = {k: round(frames[k] / times[k], 1) for k in variants}
    bytes_per_frame = {name: int(sum(p.nbytes for p in planes_for(fmt, h, w, clip[0], cs)) +
                                 sum(p.nbytes for p in empty_planes(fmt, 4 * h, 4 * w)))
                       for name, fmt in FORMATS.items()}
    print(json.dumps({"metric": "ju_process_frame per-call frames/s", "preset": args.preset, "dtype": args.dtype,
                      "size": f"{w}x{h}", "frames_per_variant": frames[next(iter(frames))], "fps": fps,
                      "host_bytes_per_frame": bytes_per_frame, "last_error": err}))


def kernel_bench(args):
    """The two conversion kernels alone (ju_debug_yuv) at args.kernel_size, NV12 and I420, args.iters times each."""
    dev = torch.device("cuda", 0)
    w, h = (int(x) for x in args.kernel_size.split("x"))
    lib = R.load_library(True)
    rng = np.random.default_rng(0)
    bgrx = torch.from_numpy(rng.integers(0, 256, (h, w, 4), dtype=np.uint8)).to(dev)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    res = {}
    for name, fmt in (("nv12", R.FMT_NV12), ("i420", R.FMT_I420)):
        planes = [torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in empty_planes(fmt, h, w)]
        ptrs = (C.c_void_p * 3)(*([p.data_ptr() for p in planes] + [None] * (3 - len(planes))))
        strides = (C.c_ssize_t * 3)(*([p.stride(0) for p in planes] + [0] * (3 - len(planes))))
        torch.cuda.synchronize()
        for direction, src in ((1, bgrx), (0, out)):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                rc = lib.ju_debug_yuv(direction, fmt, R.CS_BT709_LIMITED, w, h, src.data_ptr(), 4 * w, ptrs, strides)
                if rc != 0:
                    raise RuntimeError(lib.ju_last_error().decode())
            res[f"{name}_{'encode' if direction else 'decode'}_ms_per_call"] = \
                round((time.perf_counter() - t0) * 1e3 / args.iters, 4)
    print(json.dumps({"metric": "ju_debug_yuv host time per synchronous call (kernel time: the trace)",
                      "size": f"{w}x{h}", "iters": args.iters, **res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality", choices=sorted(M.PRESETS))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp8"])
    ap.add_argument("--warmup", type=int, default=4, help="passes over each variant's 8 buffers before timing")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=64)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-size", default="1920x1080")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if args.kernels:
        kernel_bench(args)
    else:
        frame_bench(args)


if __name__ == "__main__":
    main()
