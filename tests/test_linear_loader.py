"""Linear models on the host: the loader (nam::linear::parse_config_json / the Linear constructor, NAM/linear.cpp:61-80, 280-323),
what the model handle reports, the round trips, the refusals, and the accuracy yardstick's own checks (tests/linear_oracle.py).
No GPU."""
import json

import numpy as np
import pytest

import linear_oracle as lo
from conftest import model_path


def _load(nam, doc):
    return nam.get_dsp_json(json.dumps(doc))


def _with_config(doc, **kw):
    j = json.loads(json.dumps(doc))
    for k, v in kw.items():
        if v is None:
            j["config"].pop(k, None)
        else:
            j["config"][k] = v
    return j


def test_parse_defaults_and_info(nam_lib):
    nam = nam_lib
    doc = lo.linear_doc(65, True, seed=65)
    m = _load(nam, doc)
    assert m.info.architecture == 4 and m.architecture == "Linear"
    assert (m.NumInputChannels(), m.NumOutputChannels()) == (1, 1)
    assert m.GetPrewarmSamples() == 0
    assert m.num_weights == 66
    assert m.GetExpectedSampleRate() == 48000.0
    assert m.info.state_bytes_per_stream > 0
    assert not m.is_slimmable
    assert m.version == "0.5.4"
    assert "nam_linear_kernel" in m.describe() and "hist_frames=" in m.describe() and "splits=" in m.describe()
    # without a bias: exactly R weights; channels as given
    m = _load(nam, lo.linear_doc(64, False, in_ch=2, out_ch=3, seed=1))
    assert (m.NumInputChannels(), m.NumOutputChannels(), m.num_weights) == (2, 3, 64)
    # the history scales with the channels that carry signal: min(in, out)
    one = _load(nam, lo.linear_doc(64, False, seed=1)).info.state_bytes_per_stream
    assert m.info.state_bytes_per_stream == 2 * one
    # no sample rate in the file: unknown
    j = lo.linear_doc(3, True)
    del j["sample_rate"]
    assert _load(nam, j).GetExpectedSampleRate() == -1.0


def test_weight_count_messages(nam_lib):
    nam = nam_lib
    msg = "Params vector does not match expected size based on architecture parameters"
    for bias in (True, False):
        for delta in (+1, -1):
            j = lo.linear_doc(17, bias)
            if delta > 0:
                j["weights"].append(0.5)
            else:
                j["weights"].pop()
            with pytest.raises(nam.NamHipError, match=msg) as e:
                _load(nam, j)
            assert e.value.code == nam.ERR_MODEL
    # required fields
    for key in ("receptive_field", "bias"):
        with pytest.raises(nam.NamHipError):
            _load(nam, _with_config(lo.linear_doc(5, True), **{key: None}))


@pytest.mark.parametrize("spelling", ["auto", "direct", "legacy", "old", "fft", "partitioned_fft", "partitioned-fft", "AUTO", "Direct",
                                      "FFT", "Partitioned_FFT", "LeGaCy"])
def test_implementation_spellings_load_and_are_kept(nam_lib, spelling):
    m = _load(nam_lib, lo.linear_doc(9, True, implementation=spelling, seed=2))
    assert json.loads(m.dsp_data()["config"])["implementation"] == spelling  # kept as given, otherwise ignored
    base = _load(nam_lib, lo.linear_doc(9, True, seed=2))
    assert m.describe() == base.describe()  # one device engine: the plan does not depend on it


def test_bad_implementation(nam_lib):
    nam = nam_lib
    with pytest.raises(nam.NamHipError, match="Unsupported Linear implementation: Winograd") as e:
        _load(nam, lo.linear_doc(9, True, implementation="Winograd"))
    assert e.value.code == nam.ERR_MODEL


def test_bounds_and_device_limits(nam_lib):
    nam = nam_lib
    j = lo.linear_doc(1, False)
    j["config"]["receptive_field"] = 0
    j["weights"] = []
    with pytest.raises(nam.NamHipError, match="receptive_field") as e:
        _load(nam, j)
    assert e.value.code == nam.ERR_MODEL
    for key in ("in_channels", "out_channels"):
        with pytest.raises(nam.NamHipError, match="Channel counts must be positive") as e:
            _load(nam, _with_config(lo.linear_doc(4, True), **{key: 0}))
        assert e.value.code == nam.ERR_MODEL
    # the device limits: UNSUPPORTED, the limit in the message
    assert _load(nam, lo.linear_doc(65536, True)).num_weights == 65537
    with pytest.raises(nam.NamHipError, match="65536") as e:
        _load(nam, lo.linear_doc(65537, True))
    assert e.value.code == nam.ERR_UNSUPPORTED
    assert _load(nam, lo.linear_doc(4, True, in_ch=16, out_ch=16)).NumInputChannels() == 16
    for kw in ({"in_ch": 17}, {"out_ch": 17}):
        with pytest.raises(nam.NamHipError, match="16 channels") as e:
            _load(nam, lo.linear_doc(4, True, **kw))
        assert e.value.code == nam.ERR_UNSUPPORTED


def test_weights_and_dsp_data_round_trip(nam_lib):
    nam = nam_lib
    doc = lo.linear_doc(257, True, in_ch=2, out_ch=2, implementation="fft", seed=257)
    m = _load(nam, doc)
    d = m.dsp_data()
    assert d["architecture"] == "Linear" and d["version"] == "0.5.4" and d["expected_sample_rate"] == 48000.0
    assert np.array_equal(d["weights"], np.asarray(doc["weights"], dtype=np.float32))
    assert json.loads(d["config"]) == doc["config"]
    m2 = nam.get_dsp_data(d)
    d2 = m2.dsp_data()
    assert m2.architecture == "Linear" and np.array_equal(d2["weights"], d["weights"]) and d2["config"] == d["config"]
    assert m2.describe() == m.describe() and m2.info.state_bytes_per_stream == m.info.state_bytes_per_stream


def test_file_load(nam_lib, tmp_path):
    p = tmp_path / "ir.nam"
    p.write_text(json.dumps(lo.linear_doc(33, True, seed=5)))
    m = nam_lib.get_dsp(str(p))
    assert m.architecture == "Linear" and m.num_weights == 34
    assert nam_lib.get_sample_rate_from_nam_file(str(p)) == 48000.0


def test_refused_as_bank_member(nam_lib):
    nam = nam_lib
    lin = _load(nam, lo.linear_doc(65, True))
    with pytest.raises(nam.NamHipError, match=r"member 0 is a Linear model") as e:
        nam.ModelBank([lin])
    assert e.value.code == nam.ERR_UNSUPPORTED
    wn = nam.get_dsp(model_path("wavenet_a1_standard"))
    with pytest.raises(nam.NamHipError, match=r"member 1 is a Linear model.*shared impulse response") as e:
        nam.ModelBank([wn, lin])
    assert e.value.code == nam.ERR_UNSUPPORTED


def test_refused_inside_a_container(nam_lib):
    nam = nam_lib
    with open(model_path("lstm")) as f:
        lstm = json.load(f)
    lstm["sample_rate"] = 48000
    doc = {"version": "0.5.4", "architecture": "SlimmableContainer", "weights": [], "sample_rate": 48000,
           "config": {"submodels": [{"max_value": 0.5, "model": lstm}, {"max_value": 1.0, "model": lo.linear_doc(65, True)}]}}
    with pytest.raises(nam.NamHipError, match=r"SlimmableContainer: submodel 1 is a Linear model") as e:
        _load(nam, doc)
    assert e.value.code == nam.ERR_UNSUPPORTED


def test_still_refused_as_condition_dsp(nam_lib):
    nam = nam_lib
    with open(model_path("wavenet_condition_dsp")) as f:
        j = json.load(f)
    j["config"]["condition_dsp"] = lo.linear_doc(65, True, in_ch=1, out_ch=3)
    with pytest.raises(nam.NamHipError, match="a condition_dsp that is not a WaveNet") as e:
        _load(nam, j)
    assert e.value.code == nam.ERR_UNSUPPORTED


def test_convnet_is_still_refused(nam_lib):
    j = lo.linear_doc(5, True)
    j["architecture"] = "ConvNet"
    with pytest.raises(nam_lib.NamHipError, match="No config parser registered for architecture: ConvNet"):
        _load(nam_lib, j)


def test_library_version(nam_lib):
    import ctypes
    L = nam_lib.load_library()
    L.nam_hip_version.restype = ctypes.c_char_p
    assert L.nam_hip_version().decode().startswith("nam_hip 0.2.6")


# ---- the yardstick's own checks (no device involved) ----
def test_recipe():
    h = lo.impulse_response(4099, 4099)
    assert h.dtype == np.float32 and abs(float(np.sum(np.abs(h.astype(np.float64)))) - 3.6) < 1e-4
    assert abs(float(np.sum(np.abs(lo.impulse_response(2, 2).astype(np.float64)))) - 0.9 * np.sqrt(2)) < 1e-6
    doc = lo.linear_doc(5, True, seed=5)
    assert doc["version"] == "0.5.4" and doc["sample_rate"] == 48000 and doc["weights"][-1] == float(np.float32(0.0123))
    # truth is the convolution: an impulse reads the taps back
    h, b = lo.taps_and_bias(doc)
    x = np.zeros((1, 12), dtype=np.float32)
    x[0, 3] = 1.0
    t = lo.truth(h, b, x)
    assert np.array_equal(t[0, 3:8], h.astype(np.float64) + np.float64(b)) and np.all(t[0, :3] == np.float64(b))


@pytest.mark.parametrize("R,bias", lo.ACCURACY_CASES)
def test_yardstick_on_every_gpu_shape(R, bias):
    """The two float32 orders lie within their own bound, and a split-K fused-multiply-add model of the kernel (chunks of 128 taps,
    what nam_linear_kernel's plan cuts, oldest tap first inside a chunk; and the other direction) is within 4 e32."""
    h, b = lo.taps_and_bias(lo.linear_doc(R, bias, seed=R))
    for amp in lo.AMPLITUDES:
        ys = lo.yardstick(R, bias, amp)
        assert 0.0 < ys.e32 == max(ys.e_oldest, ys.e_newest)
        for order in ("oldest", "newest"):
            assert ys.passes(lo.f32_strict(h, b, ys.x, order))
        for chunk in (32, 128, 1024):
            for order in ("oldest", "newest"):
                if R > 1025 and (chunk, order) not in ((128, "oldest"), (1024, "newest")):
                    continue  # (the long impulse response: the kernel's own cut and one other, to keep the case quick)
                r = ys.ratio(lo.split_k_fma(h, b, ys.x, chunk, order))
                assert r <= lo.FACTOR, (R, amp, chunk, order, r)


@pytest.mark.parametrize("R,k", sorted(lo.TEETH.items()))
def test_yardstick_has_teeth(R, k):
    """One tap off by a factor 1 + 2^-k — evaluated in float64, the best any kernel could do with it — exceeds 4 e32."""
    doc = lo.linear_doc(R, True, seed=R)
    h, b = lo.taps_and_bias(lo.perturbed(doc, k))
    assert np.sum(h != lo.taps_and_bias(doc)[0]) == 1
    for amp in lo.AMPLITUDES:
        ys = lo.yardstick(R, True, amp)
        assert lo.error(lo.truth(h, b, ys.x), ys.truth) > lo.FACTOR * ys.e32
