"""Shared by the tests of a SlimmableContainer whose submodels are all Linear (one impulse response at several sizes): the
document, the ratio that selects each submodel, and one-model renderings to compare against. tests/linear_oracle.py supplies the
impulse responses (linear_doc(R, True, seed=R)) and the float64 yardstick."""
import json
import os

import numpy as np

import linear_oracle as lo

SIZES = (33, 65, 257, 1025)  # split plans 1 x 64, 1 x 128, 3 x 128, 9 x 128: two split_taps values, three split counts
MAX_VALUES = (0.25, 0.5, 0.75, 1.0)
# ModelSpec::container_index (NAM/container.cpp:85-97): the first submodel whose max_value exceeds the ratio, else the last
RATIOS = (0.1, 0.3, 0.6, 1.0)
RING_FRAMES = 9 * 128 + 512  # at max_frames <= 512: the longest submodel's splits + one launch piece
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear", "linear_container_33_65_257_1025.nam")


def sub_doc(R):
    return lo.linear_doc(R, True, seed=R)


def container_doc(sizes=SIZES, max_values=MAX_VALUES, subs=None):
    """The container of sub_doc(R) for R in sizes; `subs`: {index: document} replaces single submodels."""
    models = [sub_doc(R) for R in sizes]
    for i, d in (subs or {}).items():
        models[i] = d
    return {"version": "0.5.4", "architecture": "SlimmableContainer", "weights": [], "sample_rate": 48000,
            "config": {"submodels": [{"max_value": float(v), "model": m} for v, m in zip(max_values, models)]}}


def load(nam, doc):
    return nam.get_dsp_json(json.dumps(doc))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assign(batch, sizes):
    """Stream s of a fresh batch (every stream on the last submodel) to submodel sizes[s]."""
    for w in range(len(SIZES)):
        ids = [s for s, v in enumerate(sizes) if v == w]
        if ids and w != len(SIZES) - 1:
            batch.SetSlimmableSize(RATIOS[w], ids)


def blocks_of(x, lengths):
    """x [streams, N] cut along time into the given call lengths (which must add up to N)."""
    assert sum(lengths) == x.shape[1]
    at, out = 0, []
    for k in lengths:
        out.append(x[:, at:at + k])
        at += k
    return out


def one_model_outputs(nam, sizes, x, lengths, docs=None):
    """What the streams must equal bit for bit: for every submodel in use, ONE one-model Linear batch of it fed the rows of the
    streams on it, in the same calls. Returns [streams, N] float32."""
    y = np.zeros(x.shape, dtype=np.float32)
    for w in sorted(set(sizes)):
        ids = [s for s, v in enumerate(sizes) if v == w]
        b = load(nam, (docs or {}).get(w) or sub_doc(SIZES[w])).batch(len(ids), 64)
        assert b.kernel_name() == "nam_linear_kernel"
        rows = np.ascontiguousarray(x[ids])
        y[ids] = np.concatenate([b.process(blk) for blk in blocks_of(rows, lengths)], axis=-1)[:, 0, :]
        b.close()
    return y
