"""The yardstick of the Linear tests: nam::Linear (NAM/linear.cpp:168-196) restated in numpy.

The reference build under oracle/_ref leaves linear.cpp out (it needs Eigen's FFT), so the function is restated here:

    y[ch][n] = bias + sum_{k < R} weights[k] * x[ch][n - k]        ch < min(in, out), history zero at the start
    y[ch][n] = 0                                                    ch >= min(in, out)

    truth(h, b, x)             float64 arithmetic on the float32-rounded values
    f32_strict(h, b, x, order) float32, separate multiply and add (what the reference's build flags compile), taps
                               accumulated "oldest" first (lag R - 1 down to 0) or "newest" first (lag 0 up), the bias last
    e32                        max(error oldest-first, error newest-first) against truth

Both orders, because Eigen's dot has no defined order and on a decaying impulse response they differ by up to 4x: a kernel
may legitimately sum in either. A GPU result passes when max |gpu - truth| <= FACTOR * e32, FACTOR = 4 (tests/accuracy.py's
reasoning: two bits for association and FMA contraction). It is a condition on the kernel, not a fit to it.

linear_doc: the models of the tests. With rng = default_rng(seed): h = rng.standard_normal(R) * exp(-k / max(R / 6, 1)), scaled so
that sum |h| = 0.9 * min(4, sqrt(R)), rounded to float32; the bias is 0.0123.
"""
import copy
import functools

import numpy as np

from signals import stream_bank

FACTOR = 4.0
N_STREAMS, SEED = 8, 3
AMPLITUDES = (1.0, 2.7)
BIAS = 0.0123
# the GPU accuracy table (tests/test_gpu_linear.py): (R, bias) -> frames; the longest impulse responses see > 1,000 frames with full history
ACCURACY_CASES = [(1, True), (2, True), (63, True), (64, True), (64, False), (65, True), (257, True), (1025, True), (4099, True)]
# the teeth cases: R -> k, the largest tap scaled by 1 + 2^-k must FAIL the bound
TEETH = {65: 11, 4099: 9}


def n_frames_for(R):
    return 768 if R <= 257 else 5120


def impulse_response(R, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(R, dtype=np.float64)
    h = rng.standard_normal(R) * np.exp(-k / max(R / 6.0, 1.0))
    h *= 0.9 * min(4.0, np.sqrt(R)) / np.sum(np.abs(h))
    return h.astype(np.float32)


def linear_doc(R, bias, in_ch=1, out_ch=1, implementation=None, seed=0):
    """A .nam document of a Linear model."""
    h = impulse_response(R, seed)
    config = {"receptive_field": int(R), "bias": bool(bias)}
    if in_ch != 1:
        config["in_channels"] = int(in_ch)
    if out_ch != 1:
        config["out_channels"] = int(out_ch)
    if implementation is not None:
        config["implementation"] = implementation
    weights = [float(v) for v in h] + ([float(np.float32(BIAS))] if bias else [])
    return {"version": "0.5.4", "architecture": "Linear", "config": config, "weights": weights, "sample_rate": 48000}


def taps_and_bias(doc):
    """(h float32 [R], b float32) of a document."""
    R = doc["config"]["receptive_field"]
    w = np.asarray(doc["weights"], dtype=np.float32)
    return w[:R].copy(), (w[R] if doc["config"]["bias"] else np.float32(0.0))


def perturbed(doc, k):
    """The document with its largest-magnitude tap scaled by 1 + 2^-k, rounded to float32 like every weight."""
    j = copy.deepcopy(doc)
    h, _ = taps_and_bias(j)
    i = int(np.argmax(np.abs(h)))
    j["weights"][i] = float(np.float32(h[i] * np.float32(1.0 + 2.0 ** -k)))
    return j


def _lagged(x, k):
    """x delayed by k frames along the last axis, zeros in front."""
    if k == 0:
        return x
    out = np.zeros_like(x)
    out[..., k:] = x[..., :-k]
    return out


def truth(h, b, x):
    """float64 [..., N] for float32 taps, bias and input [..., N]."""
    x64 = np.asarray(x, dtype=np.float64)
    acc = np.zeros_like(x64)
    for k in range(len(h)):
        acc += np.float64(h[k]) * _lagged(x64, k)
    return acc + np.float64(b)


def f32_strict(h, b, x, order):
    """float32 [..., N]: one rounding per multiply and per add, taps in the given order, the bias last."""
    assert order in ("oldest", "newest")
    x32 = np.asarray(x, dtype=np.float32)
    acc = np.zeros_like(x32)
    ks = range(len(h) - 1, -1, -1) if order == "oldest" else range(len(h))
    for k in ks:
        acc = acc + np.float32(h[k]) * _lagged(x32, k)
        assert acc.dtype == np.float32
    return acc + np.float32(b)


def split_k_fma(h, b, x, chunk, order):
    """A CPU model of a split-K kernel: taps in chunks of `chunk`, inside a chunk one fused multiply-add per tap in the given
    order (the product exact in float64, one rounding to float32), the chunks' partial sums added in chunk order, the bias last."""
    x32 = np.asarray(x, dtype=np.float32)
    total = np.zeros_like(x32)
    for c0 in range(0, len(h), chunk):
        ks = list(range(c0, min(c0 + chunk, len(h))))
        if order == "oldest":
            ks.reverse()
        acc = np.zeros_like(x32)
        for k in ks:
            acc = (acc.astype(np.float64) + np.float64(h[k]) * _lagged(x32, k).astype(np.float64)).astype(np.float32)
        total = total + acc
    return total + np.float32(b)


def error(y, t):
    assert y.shape == t.shape, (y.shape, t.shape)
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - t)))


@functools.lru_cache(maxsize=None)
def inputs(n, amplitude):
    x = np.ascontiguousarray(stream_bank(N_STREAMS, n, seed=SEED) * np.float32(amplitude), dtype=np.float32)
    x.setflags(write=False)
    return x


class Yardstick:
    """One (h, b, x): the truth and e32, computed once and read-only."""

    def __init__(self, h, b, x):
        self.x = x
        self.truth = truth(h, b, x)
        self.truth.setflags(write=False)
        self.e_oldest = error(f32_strict(h, b, x, "oldest"), self.truth)
        self.e_newest = error(f32_strict(h, b, x, "newest"), self.truth)
        self.e32 = max(self.e_oldest, self.e_newest)

    def ratio(self, y):
        """max |y - truth| in units of e32."""
        return error(np.asarray(y), self.truth) / self.e32

    def passes(self, y):
        return error(np.asarray(y), self.truth) <= FACTOR * self.e32


@functools.lru_cache(maxsize=None)
def yardstick(R, bias, amplitude):
    """The accuracy table's yardstick for (R, bias, amplitude): model seed = R, stream_bank(8, N, seed=3) * amplitude."""
    h, b = taps_and_bias(linear_doc(R, bias, seed=R))
    return Yardstick(h, b, inputs(n_frames_for(R), float(amplitude)))
