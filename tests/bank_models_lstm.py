"""LSTMs with seeded random weights, written where a test asks (tmp_path): members for model banks of the LSTM family
(nam_lstm_row_kernel: hidden <= 4, nam_lstm_wide_kernel: 5 .. 32 units). The recipe is tests/golden/make_synthetic_models.py:
build_lstm — same scales and draw order (per layer W [4H][I + H], b [4H], h0 [H], c0 [H]; then the head's W [out][H], b [out]) —
so a seed gives weights AND an initial state (h0 / c0 are part of an LSTM's weight stream) of its own. `state_seed` redraws h0 /
c0 alone: two members with one `seed` and different `state_seed`s have equal weights and different initial states."""
import json

import numpy as np


def lstm_weights(seed, num_layers, input_size, hidden, out_channels, state_seed=None):
    """The weight stream as a list of floats, and the positions of h0 / c0 in it ([(start, stop)] per layer, h0 and c0 together)."""
    rng = np.random.default_rng(seed)
    srng = None if state_seed is None else np.random.default_rng(state_seed)
    weights, state_at = [], []

    def w(shape, scale, r=rng):
        weights.extend((r.standard_normal(shape).astype(np.float32) * np.float32(scale)).reshape(-1).tolist())

    for l in range(num_layers):
        I = input_size if l == 0 else hidden
        w((4 * hidden, I + hidden), 0.6 / np.sqrt(I + hidden))
        w((4 * hidden,), 0.2)
        start = len(weights)
        w((hidden,), 0.1)  # h0 (drawn from `rng` in any case: the draws behind it stay where build_lstm has them)
        w((hidden,), 0.1)  # c0
        if srng is not None:
            del weights[start:]
            w((hidden,), 0.1, srng)
            w((hidden,), 0.1, srng)
        state_at.append((start, len(weights)))
    w((out_channels, hidden), 1.0 / np.sqrt(hidden))
    w((out_channels,), 0.1)
    return weights, state_at


def write_lstm(path, seed, num_layers=1, input_size=1, hidden=3, out_channels=1, state_seed=None, sample_rate=48000):
    """Writes the model to `path`; returns its weights (list of floats)."""
    weights, _ = lstm_weights(seed, num_layers, input_size, hidden, out_channels, state_seed)
    config = dict(input_size=input_size, hidden_size=hidden, num_layers=num_layers)
    if input_size != 1:
        config["in_channels"] = input_size
    if out_channels != 1:
        config["out_channels"] = out_channels
    model = dict(version="0.5.4", architecture="LSTM", config=config,
                 metadata=dict(name=f"lstm_bank_member_{seed}", note="synthetic test model (seeded random weights)"), weights=weights,
                 sample_rate=sample_rate)
    with open(path, "w") as f:
        json.dump(model, f)
    return weights
