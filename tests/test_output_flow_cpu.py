"""The output_flow model variant (output "pre_warp", the reference's scripts/inference/onnx/output_flow.py) without a
GPU: the container word, both loaders' checks, the CLI, and the oracle side the GPU tests rest on."""
import dataclasses
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from flowfree_common import flow_free
from helpers import M, ROOT, small_config
from joshupscale_amd import runtime as R
from output_flow_common import expected_frame, oracle_frames

# SHA-256 of serialize(cfg, make_seeded_weights(cfg, seed=42)), computed on the commit before header word 140 had a
# meaning: small_config() (128-byte header), small_config(temporal_strength=0.5, temporal_window=3) (160-byte header)
# and the default-mode filter (128-byte header)
PLAIN_SHA256 = [
    (dict(), 128, "ad49009d10b5d4a8e9ce26fadfd0948cffb4089e9667374eeafb99620164476b"),
    (dict(temporal_strength=0.5, temporal_window=3), 160, "20228b467912612a9cd26113580cbbcf864e9b3f3a265702b47e4387588217fb"),
    (dict(temporal_strength=0.5), 128, "8429a6da8a20ec8129acff1f11a5a52bbb6989e95d93ba820b0fbb02ec36f5bc"),
]

VARIANTS = {
    "autoencoder": small_config(),
    "resnet": small_config(flow_arch="resnet", flow_pad_factor=0, flow_res_blocks=2),
    "brightness": small_config(normalize_brightness=True),
    "temporal": small_config(temporal_strength=0.25),
    "temporal-extended": small_config(temporal_strength=0.5, temporal_window=16, temporal_gain=4.0, temporal_norm="L2",
                                      temporal_limit=True, temporal_luma=True),
    "lrelu": small_config(flow_activation="lrelu", gen_activation="lrelu", gen_negative_slope=0.2),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_round_trip(name):
    cfg = VARIANTS[name]
    wts = M.make_seeded_weights(cfg)
    assert cfg.output == "frame"
    cfg_v, wts_v = M.output_flow(cfg, wts)
    assert cfg_v.output == "pre_warp" and cfg_v == dataclasses.replace(cfg, output="pre_warp")
    assert list(wts_v) == list(wts) and all(wts_v[k].tobytes() == wts[k].tobytes() for k in wts)
    blob = M.serialize(cfg_v, wts_v)
    version, header_bytes = struct.unpack_from("<2I", blob, 8)
    assert version == 1 and header_bytes == 160
    assert struct.unpack_from("<I", blob, 140)[0] == 1
    assert struct.unpack_from("<4I", blob, 144) == (0, 0, 0, 0)        # still reserved
    if not cfg.temporal_extended:                                      # the three temporal words at their defaults
        assert blob[128:140] == bytes(12)
    cfg2, wts2 = M.deserialize(blob)
    assert cfg2.output == "pre_warp" and list(wts2) == list(wts)
    assert all(wts2[k].tobytes() == wts[k].tobytes() for k in wts)
    assert M.serialize(cfg2, wts2) == blob
    # the plain container of the same model: the same tensors, a header that says nothing of the variant
    plain = M.serialize(cfg, wts)
    assert M.deserialize(plain)[0].output == "frame"
    assert blob[16:128] == plain[16:128]


@pytest.mark.parametrize("kw,header_bytes,sha", PLAIN_SHA256, ids=["plain", "temporal-extended", "temporal-default"])
def test_plain_containers_are_byte_identical_to_the_parents(kw, header_bytes, sha):
    cfg = small_config(**kw)
    assert cfg.output == "frame"
    blob = M.serialize(cfg, M.make_seeded_weights(cfg, seed=42))
    assert struct.unpack_from("<I", blob, 12)[0] == header_bytes
    assert hashlib.sha256(blob).hexdigest() == sha
    # ... and so is the round trip through the variant and back
    cfg_v, wts_v = M.output_flow(*M.deserialize(blob))
    back = dataclasses.replace(M.deserialize(M.serialize(cfg_v, wts_v))[0], output="frame")
    assert hashlib.sha256(M.serialize(back, wts_v)).hexdigest() == sha


def variant_blob(cfg=None):
    cfg = cfg or small_config(gen_blocks=1)
    return M.serialize(*M.output_flow(cfg, M.make_seeded_weights(cfg)))


def test_python_loader_refusals():
    blob = bytearray(variant_blob())
    struct.pack_into("<I", blob, 140, 2)
    with pytest.raises(ValueError) as e:
        M.deserialize(bytes(blob))
    assert str(e.value) == "Invalid model: unknown output selection"
    with pytest.raises(ValueError) as e:
        M.validate_config(small_config(output="both"))
    assert str(e.value) == "Invalid model: unknown output selection"
    # a flow-free model has no flow net and nothing to warp
    cfg_f, wts_f = flow_free(small_config(gen_blocks=1))
    assert M.NO_FLOW_PRE_WARP == "output pre_warp needs a flow net"
    for refuse in (lambda: M.validate_config(dataclasses.replace(cfg_f, output="pre_warp")),
                   lambda: M.serialize(dataclasses.replace(cfg_f, output="pre_warp"), wts_f),
                   lambda: M.output_flow(cfg_f, wts_f),
                   lambda: M.deserialize(M.serialize(dataclasses.replace(cfg_f, output="pre_warp"), wts_f, validate=False))):
        with pytest.raises(ValueError) as e:
            refuse()
        assert str(e.value) == "Invalid model: " + M.NO_FLOW_PRE_WARP
    # a 128-byte header has no such word: nothing to refuse, the plain model
    assert M.deserialize(M.serialize(small_config(gen_blocks=1), M.make_seeded_weights(small_config(gen_blocks=1))))[0].output == "frame"


def test_cxx_loader_refusals_and_acceptance(hip_library):
    for name, cfg in VARIANTS.items():
        R.validate_model(variant_blob(cfg))
    blob = bytearray(variant_blob())
    struct.pack_into("<I", blob, 140, 2)
    with pytest.raises(R.JoshUpscaleError) as e:
        R.validate_model(bytes(blob))
    assert e.value.code == 1 and "Invalid model: unknown output selection" in str(e.value)
    struct.pack_into("<I", blob, 140, 0xFFFFFFFF)
    with pytest.raises(R.JoshUpscaleError, match="unknown output selection"):
        R.validate_model(bytes(blob))
    struct.pack_into("<I", blob, 140, 0)                       # an extended header that selects the frame: the plain model
    R.validate_model(bytes(blob))
    cfg_f, wts_f = flow_free(small_config(gen_blocks=1))
    bad = M.serialize(dataclasses.replace(cfg_f, output="pre_warp"), wts_f, validate=False)
    with pytest.raises(R.JoshUpscaleError) as e:
        R.validate_model(bad)
    assert e.value.code == 1 and "Invalid model: " + M.NO_FLOW_PRE_WARP in str(e.value)


def test_cli_writes_the_same_bytes(tmp_path):
    cfg = small_config(gen_blocks=2, normalize_brightness=True)
    src, dst = tmp_path / "in.jupw", tmp_path / "out.jupw"
    M.save(str(src), cfg, M.make_seeded_weights(cfg))
    tool = os.path.join(ROOT, "tools", "output_flow.py")
    subprocess.run([sys.executable, tool, str(src), str(dst)], check=True, capture_output=True)
    assert dst.read_bytes() == M.serialize(*M.output_flow(*M.load(str(src))))
    assert M.load(str(dst))[0].output == "pre_warp"
    # a flow-free input: exit status 1, the message, no file
    M.save(str(src), *flow_free(cfg))
    r = subprocess.run([sys.executable, tool, str(src), str(tmp_path / "no.jupw")], capture_output=True, text=True)
    assert r.returncode == 1 and M.NO_FLOW_PRE_WARP in r.stderr and not (tmp_path / "no.jupw").exists()


def test_there_is_no_preset_of_the_variant():
    assert all(cfg.output == "frame" for cfg in M.PRESETS.values())


def test_oracle_frame_zero_is_mid_grey_and_later_frames_are_not_the_generators():
    """pre_warp of frame 0 is the warp of a zero state: every byte is trunc(0.5 * 255) = 127 (no brightness
    normalisation).  On later frames the expected variant frame differs from the plain model's frame in most bytes,
    so a GPU test that compared against the wrong tensor could not pass by accident."""
    cfg = small_config()
    frames = M.synthetic_frames(4, cfg.frame_height, cfg.frame_width, seed=5, kind="smooth")
    plain, variant, _ = oracle_frames(cfg, M.make_seeded_weights(cfg), frames)
    assert (variant[0][..., :3] == 127).all() and (variant[0][..., 3] == 0).all()
    for t in range(1, 4):
        assert variant[t].shape == plain[t].shape and (variant[t][..., 3] == 0).all()
        differ = float(np.mean(variant[t][..., :3] != plain[t][..., :3]))
        assert differ > 0.9, (t, differ)
    # the byte function: truncation, and a clamp where O.postprocess alone would wrap
    v = np.array([-0.75, -0.5, -0.4999, 0.0, 0.4999, 0.5, 0.51, 1.33])
    assert expected_frame(v.reshape(1, 8, 1).repeat(3, 2))[0, :, 0].tolist() == [0, 0, 0, 127, 254, 255, 255, 255]
