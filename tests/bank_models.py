"""Standard-topology WaveNets (16 -> 8 channels, ten dilations 1 .. 512 each, Tanh) with seeded random weights, written where a
test asks (tmp_path): members for model banks. The recipe is tests/golden/make_synthetic_models.py: build — same shapes, scales
and draw order — with the model's head_scale a parameter, so that the members of a bank differ in the per-member scalar too."""
import json

import numpy as np

DILATIONS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
ARRAYS = [(16, DILATIONS, "Tanh", False), (8, DILATIONS, "Tanh", True)]


def head_scale_of(seed):
    """distinct per seed, 0.03 .. 0.079"""
    return round(0.03 + 0.007 * (seed % 8), 4)


def write_standard(path, seed, head_scale=None):
    """Writes the model to `path`; returns its head_scale."""
    head_scale = head_scale_of(seed) if head_scale is None else head_scale
    rng = np.random.default_rng(seed)
    layers, weights = [], []
    n = len(ARRAYS)
    for i, (C, dil, act, hb) in enumerate(ARRAYS):
        in_size = 1 if i == 0 else ARRAYS[i - 1][0]
        head = 1 if i == n - 1 else ARRAYS[i + 1][0]
        K = 3
        layers.append(dict(input_size=in_size, condition_size=1, head_size=head, channels=C, kernel_size=K, dilations=dil,
                           activation=act, gated=False, head_bias=hb))

        def w(shape, fan_in):
            v = rng.standard_normal(shape).astype(np.float32) * np.float32(0.9 / np.sqrt(fan_in))
            weights.extend(v.reshape(-1).tolist())

        w((C, in_size), in_size)
        for _ in dil:
            w((C, C, K), C * K)
            w((C,), 4.0)
            w((C, 1), 1.0)
            w((C, C), C)
            w((C,), 4.0)
        w((head, C), C * len(dil))
        if hb:
            w((head,), 4.0)
    weights.append(head_scale)
    model = dict(version="0.5.4", architecture="WaveNet", config=dict(layers=layers, head=None, head_scale=head_scale),
                 metadata=dict(name=f"bank_member_{seed}", note="synthetic test model (seeded random weights)"), weights=weights,
                 sample_rate=48000)
    with open(path, "w") as f:
        json.dump(model, f)
    return head_scale
