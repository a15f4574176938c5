"""Frames/s of a preset against its output_flow variant (model_file.output_flow: the frames are pre_warp, written by
the warp launch; the generator's own frame goes to a scratch buffer), through ju_process on device BGRX frames.

Both runtimes live in one process and take turns (interleaved rounds of --frames-per-round frames, each call
synchronous), so that the clock and the other work on the machine are shared alike; --runs repeats the whole
measurement.  Prints one JSON line and writes it to --out (profiles/output_flow_bench.json).
--trace N: N frames through each runtime and nothing else, for a `rocprofv3 --kernel-trace --stats` run (the two
instantiations of warp_pack_kernel side by side)."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch's HIP runtime first, as bench.py does)

from joshupscale_amd import model_file as M  # noqa: E402
from joshupscale_amd import runtime as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="psp-quality", choices=sorted(M.PRESETS))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp8"])
    ap.add_argument("--warmup", type=int, default=4, help="passes over each runtime's 8 buffer pairs before timing")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3, help="repeat the whole interleaved measurement")
    ap.add_argument("--trace", type=int, default=0, help="only this many frames per runtime (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_flow_bench.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    cfg = M.PRESETS[args.preset]
    wts = M.make_seeded_weights(cfg)
    blobs = {"frame": M.serialize(cfg, wts), "pre_warp": M.serialize(*M.output_flow(cfg, wts))}
    h, w = cfg.frame_height, cfg.frame_width
    clip = M.synthetic_frames(8, h, w, seed=1234, kind="smooth")
    dtype = {"bf16": R.DTYPE_BF16, "fp16": R.DTYPE_F16, "fp8": R.DTYPE_FP8}[args.dtype]
    d_in = torch.from_numpy(clip).to(dev)
    rts, pairs, keep = {}, {}, []
    for name, blob in blobs.items():
        rt = R.Runtime(blob, 0, dtype, hooks=False)
        assert rt.output == name
        d_out = torch.zeros((len(clip), 4 * h, 4 * w, 4), dtype=torch.uint8, device=dev)
        keep.append(d_out)
        torch.cuda.synchronize()
        pairs[name] = [(rt.device_image(d_in[k].data_ptr(), w, h), rt.device_image(d_out[k].data_ptr(), 4 * w, 4 * h))
                       for k in range(len(clip))]
        for a, b in pairs[name]:               # the direct device path's graphs, as bench.py registers its buffers
            rt.prepare_frames(a, b)
        rts[name] = rt

    def run(name, count):
        rt, ps = rts[name], pairs[name]
        for i in range(count):
            rt.process(*ps[i % len(ps)])

    if args.trace:
        for name in rts:
            run(name, args.trace)
        print(json.dumps({"metric": "frames for a kernel trace", "frames_per_runtime": args.trace}))
        return
    for name in rts:
        run(name, args.warmup * len(clip))
    runs = []
    for _ in range(args.runs):
        times = {k: 0.0 for k in rts}
        for _ in range(args.rounds):
            for name in rts:
                t0 = time.perf_counter()
                run(name, args.frames_per_round)
                times[name] += time.perf_counter() - t0
        n = args.rounds * args.frames_per_round
        runs.append({k: round(n / times[k], 1) for k in rts})
    stats = {name: {k: rt.stat(k) for k in ("launches_per_frame", "resident_tower", "graph_replays", "fallbacks")}
             for name, rt in rts.items()}
    for rt in rts.values():
        rt.close()
    res = {"metric": "ju_process frames/s on device BGRX frames: the plain model (frame) and its output_flow variant (pre_warp)",
           "preset": args.preset, "dtype": args.dtype, "size": f"{w}x{h}",
           "frames_per_run": args.rounds * args.frames_per_round, "runs": runs,
           "pre_warp_over_frame": [round(r["pre_warp"] / r["frame"], 4) for r in runs], "stats": stats}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
