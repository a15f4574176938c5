#!/usr/bin/env python3
"""Make a .jupw model output the warped previous frame: the counterpart of the reference's
scripts/inference/onnx/output_flow.py (same positional arguments) for this engine's container.

The result runs exactly as the input model does -- same flow net, same generator, same recurrent
state and frame history -- but every frame the caller gets is pre_warp, the previous output warped
by the flow field, as u8((pre_warp + 0.5) * 255): what the flow net and the warp do, made visible.
The weights are untouched; header word 140 of the container selects the output.  A flow-free model
is refused -- it has no flow net and no previous frame to warp.

usage:
  output_flow.py IN.jupw OUT.jupw
"""

import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from joshupscale_amd import model_file as M  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("model_path", help="recurrent model (.jupw)")
    ap.add_argument("output_path", help="the same model with pre_warp as its output (.jupw)")
    args = ap.parse_args()
    try:
        cfg, weights = M.output_flow(*M.load(args.model_path))
    except ValueError as e:
        print(f"output_flow: {e}", file=sys.stderr)
        return 1
    M.save(args.output_path, cfg, weights)
    print(f"{args.output_path}: {cfg.frame_width}x{cfg.frame_height} model, output {cfg.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
