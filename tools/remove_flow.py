#!/usr/bin/env python3
"""Remove the flow net from a .jupw model: the counterpart of the reference's
scripts/inference/onnx/remove_flow.py (same positional arguments) for this engine's container.

The result is a stateless single-image 4x upscaler made from the same trained weights: no flow
net, no warp, no recurrent state; the generator sees the current LR frame only
(generator/conv_1 keeps input channels 0..2).  A model with the temporal output filter on is
refused -- the filter blends the warped previous output, which needs the flow net.

usage:
  remove_flow.py IN.jupw OUT.jupw
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
    ap.add_argument("output_path", help="flow-free model (.jupw)")
    args = ap.parse_args()
    try:
        cfg, weights = M.remove_flow(*M.load(args.model_path))
    except ValueError as e:
        print(f"remove_flow: {e}", file=sys.stderr)
        return 1
    M.save(args.output_path, cfg, weights)
    print(f"{args.output_path}: flow-free {cfg.frame_width}x{cfg.frame_height} model, "
          f"{cfg.gen_blocks} blocks x {cfg.gen_filters} filters")
    return 0


if __name__ == "__main__":
    sys.exit(main())
