"""A2-topology WaveNets (one layer array of 8 channels, 23 layers with kernel sizes 6 / 15, a 16-tap head rechannel with bias: the
topology nam_kq_kernel is compiled for, csrc/kp_table.h) with seeded random weights, written where a test asks (tmp_path): members
for model banks of the A2 family. The recipe is tests/golden/make_synthetic_models.py: build_ktap — same shapes, scales and draw
order — with the model's head_scale and the LeakyReLU slope parameters, so that the members of a bank differ in both per-member
scalars too."""
import json

import numpy as np

CHANNELS = 8
KERNEL_SIZES = [6] * 14 + [15, 15] + [6] * 7
DILATIONS = [1, 3, 7, 17, 41, 101, 239] * 2 + [1, 13] + [1, 3, 7, 17, 41, 101, 239]
HEAD_K = 16


def head_scale_of(seed):
    """distinct per seed (mod 8), 0.03 .. 0.079"""
    return round(0.03 + 0.007 * (seed % 8), 4)


def slope_of(seed):
    """LeakyReLU negative slope, distinct per seed (mod 10), in (0, 0.3]"""
    return round(0.03 * (seed % 10 + 1), 4)


def write_a2(path, seed, head_scale=None, slope=None, act="LeakyReLU"):
    """Writes the model to `path`; returns (head_scale, slope). `act`: "LeakyReLU" (with `slope`, default slope_of(seed)) or the
    name of a parameter-free activation ("Tanh", "ReLU", "Sigmoid" ...), for which slope is None."""
    head_scale = head_scale_of(seed) if head_scale is None else head_scale
    if act == "LeakyReLU":
        slope = slope_of(seed) if slope is None else slope
        activation = dict(type="LeakyReLU", negative_slope=slope)
    else:
        slope, activation = None, act
    rng = np.random.default_rng(seed)
    weights = []
    C = CHANNELS

    def w(shape, fan_in):
        v = rng.standard_normal(shape).astype(np.float32) * np.float32(0.9 / np.sqrt(fan_in))
        weights.extend(v.reshape(-1).tolist())

    layer = dict(input_size=1, condition_size=1, head=dict(out_channels=1, kernel_size=HEAD_K, bias=True), channels=C,
                 kernel_sizes=KERNEL_SIZES, dilations=DILATIONS, activation=activation, gated=False)
    w((C, 1), 1.0)
    for K in KERNEL_SIZES:
        w((C, C, K), C * K)
        w((C,), 4.0)
        w((C, 1), 1.0)
        w((C, C), C)
        w((C,), 4.0)
    w((1, C, HEAD_K), C * HEAD_K * len(KERNEL_SIZES))
    w((1,), 4.0)
    weights.append(head_scale)
    model = dict(version="0.5.4", architecture="WaveNet", config=dict(layers=[layer], head=None, head_scale=head_scale),
                 metadata=dict(name=f"a2_bank_member_{seed}", note="synthetic test model (seeded random weights)"), weights=weights,
                 sample_rate=48000)
    with open(path, "w") as f:
        json.dump(model, f)
    return head_scale, slope
