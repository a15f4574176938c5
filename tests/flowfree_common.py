"""Shared pieces of the flow-free model tests (test infrastructure).

A flow-free model F (flow_arch "none", model_file.remove_flow) is checked against its RECURRENT TWIN R(F): a normal
recurrent container with seeded flow weights, F's generator tensors, and generator/conv_1 = concat(F's conv_1,
zeros[3, 3, 48, F]) -- temporal filter and brightness flag off.  In real arithmetic R(F)'s output at every frame equals
F(frame) for any history (the pre-warp channels meet zero weights), so the unchanged oracles of the recurrent model are
F's reference, and on the GPU F's bytes equal R(F)'s (same tower, same packed weights, the generator input differs only
in slots whose weights are zero)."""

from dataclasses import replace

import numpy as np

from helpers import M


def flow_free(cfg: M.ModelConfig, seed: int = 42):
    """(cfg, weights) of the flow-free model with the generator of `cfg`'s seeded recurrent model."""
    return M.remove_flow(cfg, M.make_seeded_weights(cfg, seed=seed))


def recurrent_twin(cfg_f: M.ModelConfig, wts_f, flow_seed: int = 7):
    """R(F): seeded auto-encoder flow weights + F's generator, conv_1 zero-padded over the 48 pre-warp channels."""
    cfg_r = replace(cfg_f, flow_arch="autoencoder", normalize_brightness=False, temporal_strength=0.0)
    seeded = M.make_seeded_weights(cfg_r, seed=flow_seed)
    wts = {k: v for k, v in seeded.items() if k.startswith("flow/")}
    for k, v in wts_f.items():
        if k == "generator/conv_1/kernel":
            v = np.concatenate([v, np.zeros(v.shape[:2] + (48, v.shape[3]), np.float32)], axis=2)
        wts[k] = v
    return cfg_r, wts
