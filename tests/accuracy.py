"""The accuracy yardstick: what float32 arithmetic on a model delivers, measured against a float64 evaluation of the
SAME function (oracle/nam_oracle.c built with ORC_REAL_DOUBLE: float32-rounded weights and constants, double arithmetic).

Per (model, fast_tanh, amplitude[, slimmable ratio]) this module computes once, and caches read-only:

    x      stream_bank(8, 768, seed=3) * amplitude                         float32 [8, 768]
    truth  the float64 oracle on x, Reset(prewarm=True), 64-frame calls    float64 [8, out_ch, 768]
    y32    the strict float32 oracle on the same                           float32 [8, out_ch, 768]
    e32    max |y32 - truth| over all streams and frames

A kernel passes when max |gpu - truth| <= FACTOR * e32 (tests/test_gpu_accuracy.py). FACTOR = 4: the legitimate
differences between a kernel and the float32 oracle are summation order and FMA contraction (an -Ofast -march=native
build of the oracle, which has both, lands within 0.7 .. 1.2 e32 of the truth) and rcp / exp2 at 1 ulp where the oracle
divides; four leaves two bits for those. It is a condition on the kernels, not a fit to them.

Eight streams by 768 frames is the smallest shape that runs every stage loop of the pipeline kernels in steady state and
wraps the short rings. Amplitude 2.7 puts the peak at about full scale; every other input of the suite peaks below 0.6.

EXP2_FORM_CASES: the one allowed change of yardstick (see profiles/accuracy/README.md).
"""
import copy
import functools

import numpy as np

import nam_oracle
from conftest import model_path
from signals import stream_bank

N_STREAMS, N_FRAMES, BLOCK, SEED = 8, 768, 64, 3
AMPLITUDES = (1.0, 2.7)
FACTOR = 4.0
SR = 48000.0

# models of the GPU cases: name -> (has a tanh / sigmoid that fast_tanh or libm mode changes, slimmable ratios)
MODELS = {
    "wavenet_a1_standard": (True, (None,)),
    "synth_a1_feather": (True, (None,)),
    "synth_a1_feather_relu": (False, (None,)),
    "synth_a1_nano": (True, (None,)),
    "A2": (False, (None,)),
    "wavenet_a2_max": (False, (None,)),
    "slimmable_wavenet": (False, (0.0, 1.0)),  # widths 1 and 3
    "lstm": (True, (None,)),
    "synth_lstm_h18x2": (True, (None,)),
}


def fast_tanh_values(name):
    """Both load modes where the model has a tanh at all; otherwise the mode changes nothing and one run says it all."""
    return (True, False) if MODELS[name][0] else (True,)


def yardstick_keys():
    """Every (name, fast_tanh, amplitude, ratio) a GPU case is measured with."""
    return [(name, ft, amp, ratio) for name, (_, ratios) in MODELS.items() for ft in fast_tanh_values(name)
            for amp in AMPLITUDES for ratio in ratios]


def old_bound(fast_tanh, peak):
    """What the parity tests (test_gpu_parity.py: _tol) allow: the reference's 5e-5 (1e-4 with libm tanh) times max(1, |y|)."""
    return (5e-5 if fast_tanh else 1e-4) * max(1.0, peak)


@functools.lru_cache(maxsize=None)
def inputs(amplitude):
    x = np.ascontiguousarray(stream_bank(N_STREAMS, N_FRAMES, seed=SEED) * np.float32(amplitude), dtype=np.float32)
    x.setflags(write=False)
    return x


def run_oracle(model, fast_tanh, x, real, ratio=None, luts=None):
    """`model`: a fixture's name or a parsed .nam document. Every stream (x[s]: [frames] or [in_channels, frames]) from
    Reset(prewarm=True), 64-frame calls. `luts`: lookup-table activations, as get_dsp takes them."""
    j = nam_oracle.validate_nam_file(model_path(model)) if isinstance(model, str) else model
    dt = np.float64 if real == "f64" else np.float32
    out = []
    for s in range(x.shape[0]):
        m = nam_oracle.load_nam_json(j, fast_tanh=nam_oracle.LoadMode(fast_tanh, luts) if luts else fast_tanh, real=real)
        if ratio is not None:
            m.SetSlimmableSize(ratio)
        m.Reset(SR, BLOCK, prewarm=True)
        y = m.process_stream(x[s].astype(dt), BLOCK)
        assert y.dtype == dt
        out.append(y)
    return np.stack(out)


class Yardstick:
    def __init__(self, name, fast_tanh, amplitude, ratio):
        self.key = (name, fast_tanh, amplitude, ratio)
        self.x = inputs(amplitude)
        self.truth = run_oracle(name, fast_tanh, self.x, "f64", ratio)
        self.y32 = run_oracle(name, fast_tanh, self.x, "f32", ratio)
        for a in (self.truth, self.y32):
            a.setflags(write=False)
        self.peak = float(np.max(np.abs(self.truth)))
        self.e32 = self.error(self.y32)
        self._e32_exp2 = None

    def error(self, y):
        """max |y - truth| over all streams and frames."""
        assert y.shape == self.truth.shape, (y.shape, self.truth.shape)
        return float(np.max(np.abs(y.astype(np.float64) - self.truth)))

    @property
    def e32_exp2(self):
        """e32 of the float32 oracle with tanh / sigmoid in the kernels' documented exp2 forms (ORC_EXP2_FORMS): a CPU
        number of the reference side, against the same truth."""
        if self._e32_exp2 is None:
            name, fast_tanh, _, ratio = self.key
            self._e32_exp2 = self.error(run_oracle(name, fast_tanh, self.x, "f32x2", ratio))
        return self._e32_exp2


@functools.lru_cache(maxsize=None)
def yardstick(name, fast_tanh, amplitude, ratio=None):
    nam_oracle.build()
    return Yardstick(name, bool(fast_tanh), float(amplitude), ratio)


# ---------------------------------------------------------------------------
# The teeth test's mutation: one weight of the model off by a factor 1 + 2^-k
# ---------------------------------------------------------------------------
def _active_document(j, ratio):
    """The document whose "weights" the run reads. A2 is a SlimmableContainer: its own weight list is empty and it evaluates its
    last submodel by default."""
    if j["architecture"] == "SlimmableContainer":
        assert ratio is None
        return j["config"]["submodels"][-1]["model"]
    return j


def perturbed(name, k, ratio=None):
    """The model's JSON with its largest-magnitude weight (of those the run uses: a slimmed width slices some away)
    scaled by 1 + 2^-k, rounded to float32 like every weight."""
    j = copy.deepcopy(nam_oracle.validate_nam_file(model_path(name)))
    doc = _active_document(j, ratio)
    w = np.asarray(doc["weights"], dtype=np.float32)
    used = np.arange(len(w))
    if ratio is not None:
        m = nam_oracle.load_nam_json(doc)
        ch = m.channels_for(ratio)
        if ch != [p.channels for p in m._wc.arrays]:
            # (indices below 2^24 are exact in the float32 the slicer works in)
            used = nam_oracle.extract_slimmed_weights(m._wc.arrays, np.arange(len(w), dtype=np.float32), ch).astype(np.int64)
    i = int(used[np.argmax(np.abs(w[used]))])
    w[i] = np.float32(w[i] * np.float32(1.0 + 2.0 ** -k))
    doc["weights"] = [float(v) for v in w]
    return j


# ---------------------------------------------------------------------------
# The formula-matched yardstick (the one per-case exception the accuracy tests allow)
# ---------------------------------------------------------------------------
# In libm mode (fast_tanh=False) four of the six kernels that run wavenet_a1_standard evaluate tanh as
# 1 - 2 / (exp2(x 2 log2 e) + 1): nam_a1_p4_kernel, nam_a1_p2_kernel and nam_a1_mfma_kernel through mf::act4 -> tanh_hw
# (neuralampmodelercore_amd/csrc/device_common.h), nam_a1_q_kernel through its own copy of the form (kernel_a1_q.hip: aq_act4).
# With every operation correctly rounded that form is off by up to 1.2e-7 ABSOLUTE for |x| < 0.01 (1 - a value next to 1) and
# 1.9e-7 up to |x| = 4, where tanhf is off by 7e-10 and 6e-8: the error is the form's, not the hardware's. On wavenet_a1_standard
# (20 layers of 16 / 8 Tanh channels, most pre-activations small) the strict float32 oracle with this form alone (ORC_EXP2_FORMS,
# no GPU involved) is 2.4 e32 from the truth at amplitude 1 and 1.5 e32 at 2.7, and nam_a1_p2_kernel and nam_a1_mfma_kernel measured
# 4.5 and 4.9 e32 against tanhf's yardstick (1.8 and 2.0 against this one). So the libm-mode cases of that model ON THOSE FOUR
# KERNELS, both amplitudes, are held to 4 x e32_exp2: the float32 oracle built with the kernels' documented forms against the same
# float64 truth. nam_a1_kernel and nam_generic_kernel call tanhf (device_common.h: d_act) and keep tanhf's yardstick, as does
# every other case, libm mode included.
EXP2_FORM_MODEL = "wavenet_a1_standard"
EXP2_FORM_CASES = {"q_session", "p4_short_bursts", "p2_buffers", "a1_mfma"}


def exp2_yardstick_keys():
    """The yardstick keys whose GPU cases in EXP2_FORM_CASES are held to e32_exp2 instead of e32."""
    return [k for k in yardstick_keys() if k[0] == EXP2_FORM_MODEL and not k[1]]
