"""Per-call frames/s of ju_process_frame on BGRX, NV12, I420, P010, YUY2, I444, P210, BGR24, RGBP16, RGBPS and BGR96F
frames, host and device, psp-quality at 480x270.

Every variant goes through the same runtime in turn (interleaved rounds of --frames-per-round frames), each call
synchronous (ju_process_frame / ju_process), so that the clock and the other work on the machine are shared alike.
Prints one JSON line.  --kernels instead runs the two conversion kernels alone at --kernel-size (default 1920x1080)
through ju_debug_yuv, for a `rocprofv3 --kernel-trace --stats` run (the test flavour of the library is needed), and in
the same run the three 10-bit kernels (ju_debug_yuv10: decode, encode from a u8 frame, encode from an f16 tensor; P010
and I010) at that size plus their decode at --small-size (default 480x270, the LR frame of the flagship workload), and
the 4:2:2 / 4:4:4 kernels (ju_debug_yuv_sampled: every format's decode and encodes at that size, its decode at
--small-size), and the RGB kernels alike (ju_debug_rgb: all ten formats).  --chroma center | topleft runs the YUV kernels'
instantiations of that siting (docs/yuv_io.md, "Chroma siting and BT.2020").

--passes N adds the look-ahead variants, N frames per call: nv12_host_pass, i420_host_pass, nv12_device_pass
(ju_process_frames), p010_*_pass, yuy2_*_pass, i444_*_pass, p210_*_pass alike, and bgrx_host_pass, bgrx_device_pass (ju_process_batch), interleaved with the per-call variants in
the same process; --runs repeats the whole measurement, and the result also goes to --out
(profiles/yuv_pass_bench.json); --only limits the variants (a `rocprofv3 --kernel-trace --memory-copy-trace` run).  --kernels --items K: K frames at --kernel-size through ONE launch of the pass's decode
kernel (ju_debug_yuv_items) and through K launches of the single-frame kernel, for the same kind of trace."""

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
import yuv10_reference as T  # noqa: E402
import yuv_sampled_reference as S  # noqa: E402
import rgb_reference as G  # noqa: E402

FORMATS = {"bgrx": R.FMT_BGRX, "nv12": R.FMT_NV12, "i420": R.FMT_I420, "p010": R.FMT_P010, "yuy2": R.FMT_YUY2,
           "i444": R.FMT_I444, "p210": R.FMT_P210, "bgr24": R.FMT_BGR24, "rgbp16": R.FMT_RGBP16, "rgbps": R.FMT_RGBPS,
           "bgr96f": R.FMT_BGR96F}
TEN = (R.FMT_P010, R.FMT_I010)
CHROMA = {"left": R.CHROMA_LEFT, "center": R.CHROMA_CENTER, "topleft": R.CHROMA_TOPLEFT}


def planes_for(fmt, h, w, bgrx, cs):
    if fmt == R.FMT_BGRX:
        return [bgrx]
    if fmt in G.NEW_FORMATS:
        return G.encode_planes(fmt, frame=bgrx)
    if fmt in S.NEW_FORMATS:
        return S.encode_planes(fmt, cs, frame=bgrx)
    if fmt in TEN:
        return T.to_words(fmt, *T.encode10(T.p_from_u8(bgrx), cs))
    y, u, v = Y.encode(bgrx, cs)
    return [y, Y.to_nv12(u, v)] if fmt == R.FMT_NV12 else [y, u, v]


def empty_planes(fmt, h, w):
    if fmt == R.FMT_BGRX:
        return [np.zeros((h, w, 4), np.uint8)]
    if fmt in G.NEW_FORMATS:
        return G.blank_planes(fmt, h, w)
    if fmt in S.NEW_FORMATS:
        return S.blank_planes(fmt, h, w)
    dt = np.uint16 if fmt in TEN else np.uint8
    if fmt in (R.FMT_NV12, R.FMT_P010):
        return [np.zeros((h, w), dt), np.zeros((h // 2, w), dt)]
    return [np.zeros((h, w), dt), np.zeros((h // 2, w // 2), dt), np.zeros((h // 2, w // 2), dt)]


def to_device(plane, dev):
    """A device copy of a host plane (uint16 planes travel as int16: the bytes are what counts)."""
    return torch.from_numpy(plane.view(np.int16) if plane.dtype == np.uint16 else plane).to(dev)


def frame_bench(args):
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    blob = M.serialize(cfg, M.make_seeded_weights(cfg))
    h, w = cfg.frame_height, cfg.frame_width
    cs = R.CS_BT709_LIMITED
    clip = M.synthetic_frames(8, h, w, seed=1234, kind="smooth")
    variants, passes = {}, {}
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
                    din = [to_device(p, dev) for p in pin]
                    dout = [to_device(p, dev) for p in pout]
                    keep.append((din, dout))
                    pairs.append((R.device_frame(fmt, w, h, din, colorspace=cs),
                                  R.device_frame(fmt, 4 * w, 4 * h, dout, colorspace=cs)))
            if fmt == R.FMT_BGRX and loc == "device":
                for a, b in pairs:   # the direct device path's graphs, as bench.py registers its buffers
                    rt.prepare_frames(R.JuImage(a.planes[0], R.LOC_DEVICE, a.strides[0], w, h),
                                      R.JuImage(b.planes[0], R.LOC_DEVICE, b.strides[0], 4 * w, 4 * h))
            variants[f"{name}_{loc}"] = [(C.byref(a), C.byref(b)) for a, b in pairs]
            n = args.passes
            if n > 1 and (name, loc) != ("i420", "device"):
                # the same buffers, n consecutive ones per call (the clip's 8 buffers as a ring)
                ring = [pairs[i % len(pairs)] for i in range(max(n, len(pairs)))]
                calls = []
                for at in range(0, len(ring) - n + 1, n):
                    chunk = ring[at:at + n]
                    if fmt == R.FMT_BGRX:
                        img = lambda f: R.JuImage(f.planes[0], f.location, f.strides[0], f.width, f.height)
                        calls.append(((R.JuImage * n)(*[img(a) for a, _ in chunk]), (R.JuImage * n)(*[img(b) for _, b in chunk])))
                    else:
                        calls.append(((R.JuFrame * n)(*[a for a, _ in chunk]), (R.JuFrame * n)(*[b for _, b in chunk])))
                passes[f"{name}_{loc}_pass"] = (rt._lib.ju_process_batch if fmt == R.FMT_BGRX else rt._lib.ju_process_frames, calls)
    torch.cuda.synchronize()
    lib, handle = rt._lib, rt._h
    call = lib.ju_process_frame

    def run(name, count):
        """`count` frames of a variant; returns the frames actually run (whole calls)"""
        if name in variants:
            refs = variants[name]
            for i in range(count):
                a, b = refs[i % len(refs)]
                if call(handle, a, b) != 0:
                    raise RuntimeError(lib.ju_last_error().decode())
            return count
        fn, calls = passes[name]
        done = 0
        for i in range(max(1, count // args.passes)):
            a, b = calls[i % len(calls)]
            if fn(handle, a, b, args.passes) != 0:
                raise RuntimeError(lib.ju_last_error().decode())
            done += args.passes
        return done

    names = list(variants) + list(passes)
    if args.only:
        names = [k for k in names if k in args.only.split(",")]
    for name in names:                          # warm-up: every variant, every buffer
        run(name, args.warmup * len(clip))
    runs = []
    for _ in range(args.runs):
        times = {k: 0.0 for k in names}
        frames = {k: 0 for k in names}
        for _ in range(args.rounds):
            for name in names:
                t0 = time.perf_counter()
                frames[name] += run(name, args.frames_per_round)
                times[name] += time.perf_counter() - t0
        runs.append({k: round(frames[k] / times[k], 1) for k in names})
    stats = {k: rt.stat(k) for k in ("lookahead_frames", "lookahead_host_frames", "lookahead_yuv_frames", "graph_captures",
                                     "fallbacks")}
    err = lib.ju_last_error().decode()
    rt.close()
    fps = runs[0]
    bytes_per_frame = {name: int(sum(p.nbytes for p in planes_for(fmt, h, w, clip[0], cs)) +
                                 sum(p.nbytes for p in empty_planes(fmt, 4 * h, 4 * w)))
                       for name, fmt in FORMATS.items()}
    res = {"metric": "ju_process_frame per-call frames/s", "preset": args.preset, "dtype": args.dtype,
           "size": f"{w}x{h}", "frames_per_variant": frames[next(iter(frames))], "fps": fps,
           "host_bytes_per_frame": bytes_per_frame, "last_error": err}
    if passes:
        res.update({"metric": "frames/s per call (ju_process_frame) and per look-ahead pass (*_pass)",
                    "frames_per_pass": args.passes, "runs": runs, "stats": stats})
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


def kernel_bench(args):
    """The two conversion kernels alone (ju_debug_yuv) at args.kernel_size, NV12 and I420, args.iters times each."""
    dev = torch.device("cuda", 0)
    w, h = (int(x) for x in args.kernel_size.split("x"))
    lib = R.load_library(True)
    cs = R.CS_BT709_LIMITED | CHROMA[args.chroma]             # (the RGB kernels have no colour space)
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
                rc = lib.ju_debug_yuv(direction, fmt, cs, w, h, src.data_ptr(), 4 * w, ptrs, strides)
                if rc != 0:
                    raise RuntimeError(lib.ju_last_error().decode())
            res[f"{name}_{'encode' if direction else 'decode'}_ms_per_call"] = \
                round((time.perf_counter() - t0) * 1e3 / args.iters, 4)
    # the 10-bit kernels in the same run: decode, encode from a u8 frame, encode from an f16 tensor
    sw, sh = (int(x) for x in args.small_size.split("x"))
    state = torch.from_numpy(rng.uniform(-0.5, 0.5, (h, w, 4)).astype(np.float16)).to(dev)
    small_out = torch.zeros((sh, sw, 4), dtype=torch.uint8, device=dev)
    for name, fmt in (("p010", R.FMT_P010), ("i010", R.FMT_I010)):
        for (pw, ph), ops in (((w, h), ((1, "encode8", bgrx, 4 * w), (2, "encode_state", state, 0), (0, "decode", out, 4 * w))),
                              ((sw, sh), ((0, "decode_small", small_out, 4 * sw),))):
            planes = [to_device(rng.integers(0, 1024, p.shape, dtype=np.uint16) << (6 if fmt == R.FMT_P010 else 0), dev)
                      for p in empty_planes(fmt, ph, pw)]
            ptrs = (C.c_void_p * 3)(*([p.data_ptr() for p in planes] + [None] * (3 - len(planes))))
            strides = (C.c_ssize_t * 3)(*([2 * p.stride(0) for p in planes] + [0] * (3 - len(planes))))
            torch.cuda.synchronize()
            for op, what, image, image_stride in ops:
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    rc = lib.ju_debug_yuv10(op, fmt, cs, pw, ph, image.data_ptr(), image_stride, ptrs, strides)
                    if rc != 0:
                        raise RuntimeError(lib.ju_last_error().decode())
                res[f"{name}_{what}_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 / args.iters, 4)
    # the 4:2:2 / 4:4:4 kernels in the same run
    for fmt in S.NEW_FORMATS:
        name, deep = S.FORMAT_NAMES[fmt], fmt in S.DEEP
        full_ops = ((1, "encode8", bgrx, 4 * w),) + (((2, "encode_state", state, 0),) if deep else ()) + ((0, "decode", out, 4 * w),)
        for (pw, ph), ops in (((w, h), full_ops), ((sw, sh), ((0, "decode_small", small_out, 4 * sw),))):
            top = 1024 if deep else 256
            held = [p + rng.integers(0, top, p.shape).astype(p.dtype) << (6 if fmt == R.FMT_P210 else 0)
                    for p in S.blank_planes(fmt, ph, pw)]
            planes = [to_device(p, dev) for p in held]
            ptrs = (C.c_void_p * 3)(*([p.data_ptr() for p in planes] + [None] * (3 - len(planes))))
            strides = (C.c_ssize_t * 3)(*([p.nbytes // p.shape[0] for p in held] + [0] * (3 - len(planes))))
            torch.cuda.synchronize()
            for op, what, image, image_stride in ops:
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    rc = lib.ju_debug_yuv_sampled(op, fmt, cs, pw, ph, image.data_ptr(), image_stride, ptrs, strides)
                    if rc != 0:
                        raise RuntimeError(lib.ju_last_error().decode())
                res[f"{name}_{what}_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 / args.iters, 4)
    # the RGB kernels in the same run: every format's encode from a u8 frame, the deep formats' encode from an f16 tensor,
    # the decode at both sizes
    for fmt in G.NEW_FORMATS:
        name, deep = G.FORMAT_NAMES[fmt], fmt in G.DEEP
        full_ops = ((1, "encode8", bgrx, 4 * w),) + (((2, "encode_state", state, 0),) if deep else ()) + ((0, "decode", out, 4 * w),)
        for (pw, ph), ops in (((w, h), full_ops), ((sw, sh), ((0, "decode_small", small_out, 4 * sw),))):
            held = G.encode_planes(fmt, frame=rng.integers(0, 256, (ph, pw, 4), dtype=np.uint8))
            planes = [to_device(p, dev) for p in held]
            ptrs = (C.c_void_p * 3)(*([p.data_ptr() for p in planes] + [None] * (3 - len(planes))))
            strides = (C.c_ssize_t * 3)(*([p.nbytes // p.shape[0] for p in held] + [0] * (3 - len(planes))))
            torch.cuda.synchronize()
            for op, what, image, image_stride in ops:
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    rc = lib.ju_debug_rgb(op, fmt, pw, ph, image.data_ptr(), image_stride, ptrs, strides)
                    if rc != 0:
                        raise RuntimeError(lib.ju_last_error().decode())
                res[f"{name}_{what}_ms_per_call"] = round((time.perf_counter() - t0) * 1e3 / args.iters, 4)
    print(json.dumps({"metric": "ju_debug_yuv / ju_debug_yuv10 / ju_debug_yuv_sampled / ju_debug_rgb host time per synchronous call (kernel time: the trace)",
                      "chroma": args.chroma, "size": f"{w}x{h}", "small_size": f"{sw}x{sh}", "iters": args.iters, **res}))


def items_bench(args):
    """K frames at args.kernel_size: one launch of the pass's decode kernel, then K launches of the single-frame one."""
    dev = torch.device("cuda", 0)
    w, h = (int(x) for x in args.kernel_size.split("x"))
    k = args.items
    lib = R.load_library(True)
    rng = np.random.default_rng(0)
    outs = [torch.zeros((h, w, 4), dtype=torch.uint8, device=dev) for _ in range(k)]
    planes = [[torch.from_numpy(rng.integers(0, 256, p.shape, dtype=np.uint8)).to(dev) for p in empty_planes(R.FMT_NV12, h, w)]
              for _ in range(k)]
    ptrs = (C.c_void_p * (3 * k))(*[q for pl in planes for q in (pl[0].data_ptr(), pl[1].data_ptr(), None)])
    strides = (C.c_ssize_t * (3 * k))(*[q for _ in planes for q in (w, w, 0)])
    fmts, css = (C.c_int * k)(*[R.FMT_NV12] * k), (C.c_int * k)(*[R.CS_BT709_LIMITED] * k)
    dst, dst_strides = (C.c_void_p * k)(*[o.data_ptr() for o in outs]), (C.c_ssize_t * k)(*[4 * w] * k)
    torch.cuda.synchronize()
    for _ in range(args.iters):
        if lib.ju_debug_yuv_items(k, fmts, css, w, h, dst, dst_strides, ptrs, strides) != 0:
            raise RuntimeError(lib.ju_last_error().decode())
        for i in range(k):
            one = (C.c_void_p * 3)(planes[i][0].data_ptr(), planes[i][1].data_ptr(), None)
            one_strides = (C.c_ssize_t * 3)(w, w, 0)
            if lib.ju_debug_yuv(0, R.FMT_NV12, R.CS_BT709_LIMITED, w, h, outs[i].data_ptr(), 4 * w, one, one_strides) != 0:
                raise RuntimeError(lib.ju_last_error().decode())
    print(json.dumps({"metric": "decode launches for a kernel trace", "size": f"{w}x{h}", "items": k, "iters": args.iters,
                      "launches": {"yuv420_to_bgrx_items_kernel": args.iters, "yuv420_to_bgrx_kernel": args.iters * k}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality", choices=sorted(M.PRESETS))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp8"])
    ap.add_argument("--warmup", type=int, default=4, help="passes over each variant's 8 buffers before timing")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=64)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-size", default="1920x1080")
    ap.add_argument("--small-size", default="480x270", help="with --kernels: the second size of the 10-bit decode")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--passes", type=int, default=0, help="frames per look-ahead call (2..8) of the *_pass variants; 0: none")
    ap.add_argument("--runs", type=int, default=1, help="repeat the whole interleaved measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_pass_bench.json"))
    ap.add_argument("--only", default="", help="comma-separated variants to run (for a trace), e.g. nv12_host_pass")
    ap.add_argument("--chroma", default="left", choices=sorted(CHROMA),
                    help="with --kernels: the chroma siting of the YUV kernels (left: the default's instantiations)")
    ap.add_argument("--items", type=int, default=0, help="with --kernels: the pass's decode kernel over this many frames")
    args = ap.parse_args()
    if args.kernels and args.items:
        items_bench(args)
    elif args.kernels:
        kernel_bench(args)
    else:
        frame_bench(args)


if __name__ == "__main__":
    main()
