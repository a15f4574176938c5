"""Flow-free single-image models (flow_arch "none", the reference's scripts/inference/onnx/remove_flow.py) without a
GPU: the transformation, the container, both loaders' checks, the CLI and the Keras import."""
import dataclasses
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from flowfree_common import flow_free, recurrent_twin
from helpers import M, ROOT, small_config
from joshupscale_amd import keras_import as K
from joshupscale_amd import runtime as R


def test_remove_flow_is_the_reference_scripts_slice():
    for cfg in [M.PRESETS["psp-quality"], M.PRESETS["psp-quality-flowres"], small_config(gen_filters=32)]:
        wts = M.make_seeded_weights(cfg)
        cfg_f, wts_f = M.remove_flow(cfg, wts)
        assert cfg_f.flow_arch == "none" and cfg_f.temporal_strength == 0
        assert not any(k.startswith("flow/") for k in wts_f)
        gen = [k for k in wts if k.startswith("generator/")]
        assert list(wts_f) == gen
        for k in gen:
            want = wts[k][:, :, :3, :] if k == "generator/conv_1/kernel" else wts[k]
            assert wts_f[k].shape == want.shape and wts_f[k].tobytes() == want.tobytes(), k
        assert wts_f["generator/conv_1/kernel"].shape == (3, 3, 3, cfg.gen_filters)
        # what the weights cannot tell stays: geometry, generator activation, eps, dtype hint, brightness flag
        for f in ("frame_height", "frame_width", "gen_filters", "gen_blocks", "gen_activation", "bn_eps",
                  "compute_dtype", "normalize_brightness"):
            assert getattr(cfg_f, f) == getattr(cfg, f), f
        blob = M.serialize(cfg_f, wts_f)
        cfg2, wts2 = M.deserialize(blob)
        assert cfg2.flow_arch == "none" and list(wts2) == list(wts_f)
        assert M.serialize(cfg2, wts2) == blob


def test_flow_free_container_header():
    cfg, wts = flow_free(small_config(flow_pad_factor=4, num_flow_inputs=2, flow_arch="resnet", flow_res_blocks=2))
    blob = M.serialize(cfg, wts)
    assert struct.unpack_from("<I", blob, 8)[0] == 1                  # the container version stays 1
    assert struct.unpack_from("<I", blob, 32)[0] == 2                 # flow_arch "none"
    d = M.ModelConfig()                                               # flow fields at their defaults
    assert struct.unpack_from("<2I", blob, 28) == (d.num_flow_inputs, 2)
    assert struct.unpack_from("<I", blob, 36)[0] == d.flow_pad_factor
    assert struct.unpack_from("<3I", blob, 52) == (d.flow_res_filters, d.flow_res_blocks, len(d.flow_filters))


def test_preset_is_remove_flow_of_psp_quality_and_old_presets_are_unchanged():
    cfg = M.PRESETS["psp-quality-noflow"]
    want_cfg, want = M.remove_flow(M.PRESETS["psp-quality"], M.make_seeded_weights(M.PRESETS["psp-quality"]))
    got = M.make_seeded_weights(cfg)
    assert cfg == want_cfg and list(got) == list(want)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    # the seeded recurrent presets do not depend on the new one (tests/test_golden.py pins their SHA-256)
    psp = M.serialize(M.PRESETS["psp-quality"], M.make_seeded_weights(M.PRESETS["psp-quality"]))
    assert hashlib.sha256(psp).hexdigest() == hashlib.sha256(
        M.serialize(M.ModelConfig(), M.make_seeded_weights(M.ModelConfig()))).hexdigest()


def refused_by_both(cfg, wts, message):
    with pytest.raises(ValueError) as py:
        M.serialize(cfg, wts)
    assert str(py.value) == "Invalid model: " + message
    with pytest.raises(R.JoshUpscaleError) as cc:
        R.validate_model(M.serialize(cfg, wts, validate=False))
    assert cc.value.code == 1 and str(py.value) in str(cc.value), str(cc.value)


def test_flow_free_checks_of_both_loaders(hip_library):
    cfg, wts = flow_free(small_config(gen_blocks=1))
    R.validate_model(M.serialize(cfg, wts))
    # conv_1 of the recurrent model (51 input channels), or a wrong width
    full = M.make_seeded_weights(small_config(gen_blocks=1))
    refused_by_both(cfg, {**wts, "generator/conv_1/kernel": full["generator/conv_1/kernel"]},
                    M.NO_FLOW_CONV_1)
    refused_by_both(cfg, {**wts, "generator/conv_1/kernel": wts["generator/conv_1/kernel"][..., :32]},
                    M.NO_FLOW_CONV_1)
    # stray flow tensors
    refused_by_both(cfg, {**wts, "flow/conv_2/bias": full["flow/conv_2/bias"]}, M.NO_FLOW_TENSORS)
    # the temporal filter blends pre_warp: it needs the flow net
    refused_by_both(dataclasses.replace(cfg, temporal_strength=0.25), wts, M.NO_FLOW_TEMPORAL)
    with pytest.raises(ValueError, match=M.NO_FLOW_TEMPORAL):
        M.remove_flow(small_config(temporal_strength=0.25), M.make_seeded_weights(small_config()))


def test_flow_fields_of_a_flow_free_model_are_ignored(hip_library):
    cfg, wts = flow_free(small_config(gen_blocks=1))
    weird = dataclasses.replace(cfg, num_flow_inputs=9, flow_pad_factor=7, flow_filters=(33,), flow_res_filters=48,
                                flow_res_blocks=1000, flow_activation="lrelu", flow_negative_slope=-3.0)
    M.validate_config(weird)
    blob = bytearray(M.serialize(cfg, wts))
    struct.pack_into("<2I", blob, 28, 9, 2)                 # num_flow_inputs, (flow_arch)
    struct.pack_into("<I", blob, 36, 7)                     # flow_pad_factor
    struct.pack_into("<3I", blob, 52, 48, 1000, 1)          # flow_res_filters, flow_res_blocks, n_flow_filters
    struct.pack_into("<I", blob, 64, 33)                    # flow_filters[0]
    struct.pack_into("<If", blob, 116, 1, -3.0)             # flow activation lrelu, slope -3
    R.validate_model(bytes(blob))
    # the 4 GiB rule counts the generator's widths only: a flow net this wide would not fit
    big = dataclasses.replace(cfg, frame_height=8192, frame_width=4064)
    M.validate_config(big)
    with pytest.raises(ValueError, match="4 GiB"):
        M.validate_config(dataclasses.replace(big, flow_arch="resnet", flow_pad_factor=0, flow_res_filters=256))
    # the brightness flag is accepted (it has no effect without the flow net)
    R.validate_model(M.serialize(dataclasses.replace(cfg, normalize_brightness=True), wts))


def test_loader_accepts_the_flow_free_preset_and_its_twin(hip_library):
    cfg = M.PRESETS["psp-quality-noflow"]
    wts = M.make_seeded_weights(cfg)
    R.validate_model(M.serialize(cfg, wts))
    R.validate_model(M.serialize(*recurrent_twin(cfg, wts)))


def test_remove_flow_cli_writes_the_same_bytes(tmp_path):
    cfg = small_config(gen_blocks=2)
    src = tmp_path / "in.jupw"
    M.save(str(src), cfg, M.make_seeded_weights(cfg))
    dst = tmp_path / "out.jupw"
    tool = os.path.join(ROOT, "tools", "remove_flow.py")
    subprocess.run([sys.executable, tool, str(src), str(dst)], check=True, capture_output=True)
    assert dst.read_bytes() == M.serialize(*M.remove_flow(*M.load(str(src))))
    # a model with the temporal filter on is refused
    M.save(str(src), dataclasses.replace(cfg, temporal_strength=0.5), M.make_seeded_weights(cfg))
    r = subprocess.run([sys.executable, tool, str(src), str(tmp_path / "no.jupw")], capture_output=True, text=True)
    assert r.returncode != 0 and M.NO_FLOW_TEMPORAL in r.stderr and not (tmp_path / "no.jupw").exists()


def test_keras_import_with_remove_flow():
    cfg = small_config(gen_blocks=2)
    wts = M.make_seeded_weights(cfg, seed=5)
    gen, flow = K.layers_from_container(wts)
    base = M.ModelConfig(frame_height=30, frame_width=48, flow_pad_factor=cfg.flow_pad_factor)
    cfg_f, wts_f = M.remove_flow(cfg, wts)
    cfg2, w2 = K.container_weights(gen, flow, base, remove_flow=True)
    assert cfg2 == cfg_f and set(w2) == set(wts_f)
    assert M.serialize(cfg2, {k: w2[k] for k in wts_f}) == M.serialize(cfg_f, wts_f)
    # a generator-only layer set with a 3-channel conv_1: an already flow-free model
    gen_f, flow_f = K.layers_from_container(wts_f)
    assert flow_f == {}
    cfg3, w3 = K.container_weights(gen_f, flow_f, base)
    assert cfg3 == cfg_f
    assert M.serialize(cfg3, {k: w3[k] for k in wts_f}) == M.serialize(cfg_f, wts_f)
    # a 51-channel conv_1 without a flow net is still an error
    with pytest.raises(KeyError, match="flow model has no layer"):
        K.container_weights(gen, {}, base)
