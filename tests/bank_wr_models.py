"""Members for model banks of the nam_wn_reg_kernel family (tests/test_bank_wr_abi.py, tests/test_gpu_bank_wr.py), written where a
test asks, and the list of every file those tests write (`write_all`): tools/warm_jit_cache.py writes the same files with the same
seeds, so that the per-model code objects — keyed on the generated header's text, not on the path — are compiled by build().
  write_nano  the official nano size (4 -> 2 channels, ten dilations 1 .. 512 each, Tanh, head bias on the second array):
              bank_models.write_standard's recipe and draw order on those arrays
  redraw      a fixture's JSON with every weight list — a nested condition_dsp's too — multiplied by 1 + 0.25 xi, xi seeded
              normal, in float32: the topology and the counts are the fixture's, every weight (the head scales too) its own"""
import json
import os

import numpy as np

from bank_models import DILATIONS, _draw, _draw_layer, _write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")

NANO_ARRAYS = [(4, DILATIONS, "Tanh", False), (2, DILATIONS, "Tanh", True)]
NANO_HEAD_SCALE = 0.05  # tests/golden/models/synth_a1_nano.nam's: such a member's generated header is the fixture's

NANO_SEEDS = (601, 602, 603, 604, 605, 606, 607, 608)
NANO_OTHER_SCALE = (5, 0.08)  # (member, head_scale): the one nano member of the GPU tests with another head_scale
COND_SEEDS = (621, 622, 623)
HEAD_SEEDS = (641, 642, 643)


def write_nano(path, seed, head_scale=None, dilations=None, head_bias=True):
    """Writes the model to `path`; returns its head_scale. `dilations`: the second array's, when not the official ones (a member
    of another geometry, for refusals); `head_bias`: the second array's (off: the same geometry, another program)."""
    head_scale = NANO_HEAD_SCALE if head_scale is None else head_scale
    arrays = list(NANO_ARRAYS)
    if dilations is not None:
        arrays[1] = (arrays[1][0], list(dilations)) + arrays[1][2:]
    arrays[1] = arrays[1][:3] + (bool(head_bias),)
    rng = np.random.default_rng(seed)
    layers, weights = [], []
    n = len(arrays)
    for i, (C, dil, act, hb) in enumerate(arrays):
        in_size = 1 if i == 0 else arrays[i - 1][0]
        head = 1 if i == n - 1 else arrays[i + 1][0]
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
    _write(path, "WaveNet", dict(layers=layers, head=None, head_scale=head_scale), f"nano_bank_member_{seed}", weights)
    return head_scale


def redraw(fixture_name, path, seed):
    """Writes tests/golden/models/<fixture_name>.nam with redrawn weights to `path`."""
    with open(os.path.join(MODELS, fixture_name + ".nam")) as f:
        model = json.load(f)
    rng = np.random.default_rng(seed)

    def walk(node):
        if isinstance(node, dict):
            for key in sorted(node):
                if key == "weights" and isinstance(node[key], list):
                    w = np.asarray(node[key], dtype=np.float32)
                    xi = rng.standard_normal(w.shape).astype(np.float32)
                    node[key] = (w * (np.float32(1.0) + np.float32(0.25) * xi)).astype(np.float32).tolist()
                else:
                    walk(node[key])
        elif isinstance(node, list):
            for v in node:
                walk(v)

    walk(model)
    with open(path, "w") as f:
        json.dump(model, f)


def write_all(directory):
    """Every model file the new bank tests use, under `directory`: {"nano": [eight paths], "cond": [three], "head": [three],
    "nano_dil": path, "nano_nobias": path}.
      nano      write_nano(seed) for NANO_SEEDS; member NANO_OTHER_SCALE[0] with head_scale NANO_OTHER_SCALE[1]
      cond      redraw("wavenet_condition_dsp", seed) for COND_SEEDS
      head      redraw("synth_posthead", seed) for HEAD_SEEDS: a post-stack head (two output channels); head_scale, redrawn like every
                weight, sits on the head's first layer
      nano_dil  a nano whose second array's last dilation is 256 instead of 512 (another geometry: refused next to a nano)
      nano_nobias  a nano without the second array's head bias (the same rings and prewarm, another op program: refused too)"""
    directory = str(directory)
    out = dict(nano=[], cond=[], head=[])
    for i, seed in enumerate(NANO_SEEDS):
        p = os.path.join(directory, f"nano_{seed}.nam")
        write_nano(p, seed, head_scale=NANO_OTHER_SCALE[1] if i == NANO_OTHER_SCALE[0] else None)
        out["nano"].append(p)
    for seed in COND_SEEDS:
        p = os.path.join(directory, f"cond_{seed}.nam")
        redraw("wavenet_condition_dsp", p, seed)
        out["cond"].append(p)
    for seed in HEAD_SEEDS:
        p = os.path.join(directory, f"head_{seed}.nam")
        redraw("synth_posthead", p, seed)
        out["head"].append(p)
    out["nano_dil"] = os.path.join(directory, "nano_dil.nam")
    write_nano(out["nano_dil"], 631, dilations=DILATIONS[:-1] + [256])
    out["nano_nobias"] = os.path.join(directory, "nano_nobias.nam")
    write_nano(out["nano_nobias"], 632, head_bias=False)
    return out


def check_members(oracle, paths, signal, fast_tanh=True):
    """On the CPU oracle: every member finite and audible (|y|max > 1e-3) on `signal` [in_channels, T], every two members different.
    Returns |y|max per member."""
    ys = []
    for p in paths:
        ref = oracle.get_dsp(p, fast_tanh=fast_tanh)
        ref.Reset(48000.0, 64)
        ys.append(np.asarray(ref.process_stream(signal, 64)))
    peaks = [float(np.max(np.abs(y))) for y in ys]
    for p, y, peak in zip(paths, ys, peaks):
        assert np.isfinite(y).all(), p
        assert peak > 1e-3, (p, peak)
    for i in range(len(ys)):
        for j in range(i + 1, len(ys)):
            assert not np.array_equal(ys[i], ys[j]), (paths[i], paths[j])
    return peaks
