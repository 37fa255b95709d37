"""Models with seeded random weights, written where a test asks (tmp_path): members for model banks, one writer per bank family.
The recipes are tests/golden/make_synthetic_models.py's — same shapes, scales and draw order — with what a bank keeps per member
(head_scale, the LeakyReLU slope, an LSTM's initial state) as parameters, so that the members of a bank differ in those too.
  write_standard  the official topology (16 -> 8 channels, ten dilations 1 .. 512 each, Tanh): recipe `build`
  write_a2        the A2 topology (one array of 8 channels, 23 layers with kernel sizes 6 / 15, a 16-tap head rechannel with bias:
                  what nam_kq_kernel is compiled for, csrc/kp_table.h): recipe `build_ktap`
  write_lstm      LSTMs (nam_lstm_row_kernel: hidden <= 4, nam_lstm_wide_kernel: 5 .. 32 units): recipe `build_lstm`"""
import json

import numpy as np

DILATIONS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
ARRAYS = [(16, DILATIONS, "Tanh", False), (8, DILATIONS, "Tanh", True)]

A2_CHANNELS = 8
A2_KERNEL_SIZES = [6] * 14 + [15, 15] + [6] * 7
A2_DILATIONS = [1, 3, 7, 17, 41, 101, 239] * 2 + [1, 13] + [1, 3, 7, 17, 41, 101, 239]
A2_HEAD_K = 16


def head_scale_of(seed):
    """distinct per seed (mod 8), 0.03 .. 0.079"""
    return round(0.03 + 0.007 * (seed % 8), 4)


def slope_of(seed):
    """LeakyReLU negative slope, distinct per seed (mod 10), in (0, 0.3]"""
    return round(0.03 * (seed % 10 + 1), 4)


def _draw(rng, weights, shape, scale):
    """the next `shape` normal draws of `rng`, as float32 times float32(scale), behind `weights`"""
    weights.extend((rng.standard_normal(shape).astype(np.float32) * np.float32(scale)).reshape(-1).tolist())


def _draw_layer(rng, weights, C, K):
    """one WaveNet layer: conv [C][C][K] + bias, input mixin [C][1], 1x1 [C][C] + bias"""
    _draw(rng, weights, (C, C, K), 0.9 / np.sqrt(C * K))
    _draw(rng, weights, (C,), 0.9 / np.sqrt(4.0))
    _draw(rng, weights, (C, 1), 0.9 / np.sqrt(1.0))
    _draw(rng, weights, (C, C), 0.9 / np.sqrt(C))
    _draw(rng, weights, (C,), 0.9 / np.sqrt(4.0))


def _write(path, architecture, config, name, weights, sample_rate=48000):
    model = dict(version="0.5.4", architecture=architecture, config=config,
                 metadata=dict(name=name, note="synthetic test model (seeded random weights)"), weights=weights, sample_rate=sample_rate)
    with open(path, "w") as f:
        json.dump(model, f)


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
        _draw(rng, weights, (C, in_size), 0.9 / np.sqrt(in_size))
        for _ in dil:
            _draw_layer(rng, weights, C, K)
        _draw(rng, weights, (head, C), 0.9 / np.sqrt(C * len(dil)))
        if hb:
            _draw(rng, weights, (head,), 0.9 / np.sqrt(4.0))
    weights.append(head_scale)
    _write(path, "WaveNet", dict(layers=layers, head=None, head_scale=head_scale), f"bank_member_{seed}", weights)
    return head_scale


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
    C = A2_CHANNELS
    layer = dict(input_size=1, condition_size=1, head=dict(out_channels=1, kernel_size=A2_HEAD_K, bias=True), channels=C,
                 kernel_sizes=A2_KERNEL_SIZES, dilations=A2_DILATIONS, activation=activation, gated=False)
    _draw(rng, weights, (C, 1), 0.9 / np.sqrt(1.0))
    for K in A2_KERNEL_SIZES:
        _draw_layer(rng, weights, C, K)
    _draw(rng, weights, (1, C, A2_HEAD_K), 0.9 / np.sqrt(C * A2_HEAD_K * len(A2_KERNEL_SIZES)))
    _draw(rng, weights, (1,), 0.9 / np.sqrt(4.0))
    weights.append(head_scale)
    _write(path, "WaveNet", dict(layers=[layer], head=None, head_scale=head_scale), f"a2_bank_member_{seed}", weights)
    return head_scale, slope


def lstm_weights(seed, num_layers, input_size, hidden, out_channels, state_seed=None):
    """The weight stream as a list of floats (per layer W [4H][I + H], b [4H], h0 [H], c0 [H]; then the head's W [out][H], b [out]),
    and the positions of h0 / c0 in it ([(start, stop)] per layer, h0 and c0 together). A seed gives weights AND an initial state
    (h0 / c0 are part of an LSTM's weight stream) of its own; `state_seed` redraws h0 / c0 alone: two members with one `seed` and
    different `state_seed`s have equal weights and different initial states."""
    rng = np.random.default_rng(seed)
    srng = None if state_seed is None else np.random.default_rng(state_seed)
    weights, state_at = [], []
    for l in range(num_layers):
        I = input_size if l == 0 else hidden
        _draw(rng, weights, (4 * hidden, I + hidden), 0.6 / np.sqrt(I + hidden))
        _draw(rng, weights, (4 * hidden,), 0.2)
        start = len(weights)
        _draw(rng, weights, (hidden,), 0.1)  # h0 (drawn from `rng` in any case: the draws behind it stay where build_lstm has them)
        _draw(rng, weights, (hidden,), 0.1)  # c0
        if srng is not None:
            del weights[start:]
            _draw(srng, weights, (hidden,), 0.1)
            _draw(srng, weights, (hidden,), 0.1)
        state_at.append((start, len(weights)))
    _draw(rng, weights, (out_channels, hidden), 1.0 / np.sqrt(hidden))
    _draw(rng, weights, (out_channels,), 0.1)
    return weights, state_at


def write_lstm(path, seed, num_layers=1, input_size=1, hidden=3, out_channels=1, state_seed=None, sample_rate=48000):
    """Writes the model to `path`; returns its weights (list of floats)."""
    weights, _ = lstm_weights(seed, num_layers, input_size, hidden, out_channels, state_seed)
    config = dict(input_size=input_size, hidden_size=hidden, num_layers=num_layers)
    if input_size != 1:
        config["in_channels"] = input_size
    if out_channels != 1:
        config["out_channels"] = out_channels
    _write(path, "LSTM", config, f"lstm_bank_member_{seed}", weights, sample_rate)
    return weights
