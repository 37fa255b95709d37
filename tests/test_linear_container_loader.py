"""A SlimmableContainer whose submodels are all Linear, on the host: it loads, what the model handle reports, the round trips, what
stays refused (a mixed container, a multi-channel Linear submodel, the container as a bank member), and the checks of the yardstick
the GPU tests build themselves (R = 33). No GPU."""
import copy
import json
import re

import numpy as np
import pytest

import linear_container as lc
import linear_oracle as lo
from conftest import model_path


def test_loads_and_info(nam_lib):
    m = lc.load(nam_lib, lc.container_doc())
    assert m.info.architecture == 3 and m.architecture == "SlimmableContainer"
    assert m.is_slimmable
    assert (m.NumInputChannels(), m.NumOutputChannels()) == (1, 1)
    assert m.GetPrewarmSamples() == 0
    assert m.num_weights == 0  # a container has no weights of its own
    assert m.GetExpectedSampleRate() == 48000.0
    # the history one stream keeps: its column of the batch's one ring, as long as the longest submodel needs + one launch piece
    assert m.info.state_bytes_per_stream == 4 * lc.RING_FRAMES
    longest = lc.load(nam_lib, lc.sub_doc(1025))
    assert m.info.state_bytes_per_stream == longest.info.state_bytes_per_stream


def test_breakpoints(nam_lib):
    assert lc.load(nam_lib, lc.container_doc()).GetSlimmableSizeBreakpoints() == [0.25, 0.5, 0.75]
    assert lc.load(nam_lib, lc.container_doc(sizes=(33,), max_values=(1.0,))).GetSlimmableSizeBreakpoints() == []


def test_description_names_four_split_plans(nam_lib):
    text = lc.load(nam_lib, lc.container_doc()).describe()
    plans = re.findall(r"receptive_field=(\d+) hist_frames=\d+ splits=(\d+) split_taps=(\d+)", text)
    assert plans == [("33", "1", "64"), ("65", "1", "128"), ("257", "3", "128"), ("1025", "9", "128")], text
    assert "nam_linear_pairs_kernel" in text and f"ring_frames={lc.RING_FRAMES}" in text


def test_dsp_data_round_trip(nam_lib):
    nam = nam_lib
    doc = lc.container_doc()
    m = lc.load(nam, doc)
    d = m.dsp_data()
    assert d["architecture"] == "SlimmableContainer" and d["version"] == "0.5.4" and d["expected_sample_rate"] == 48000.0
    assert d["weights"].size == 0
    assert json.loads(d["config"]) == doc["config"]
    m2 = nam.get_dsp_data(d)
    assert m2.is_slimmable and m2.describe() == m.describe() and m2.dsp_data()["config"] == d["config"]
    assert m2.info.state_bytes_per_stream == m.info.state_bytes_per_stream


def test_fixture_is_the_recipe(nam_lib):
    with open(lc.FIXTURE) as f:
        assert json.load(f) == lc.container_doc()  # tests/golden/make_linear_container.py
    assert nam_lib.get_dsp(lc.FIXTURE).describe() == lc.load(nam_lib, lc.container_doc()).describe()


def test_container_rules_still_apply(nam_lib):
    nam = nam_lib
    with pytest.raises(nam.NamHipError, match="sorted by ascending max_value"):
        lc.load(nam, lc.container_doc(max_values=(0.25, 0.75, 0.5, 1.0)))
    with pytest.raises(nam.NamHipError, match=r"last submodel max_value must be >= 1.0"):
        lc.load(nam, lc.container_doc(max_values=(0.2, 0.4, 0.6, 0.8)))
    odd = lc.sub_doc(65)
    odd["sample_rate"] = 44100
    with pytest.raises(nam.NamHipError, match="submodel sample rate mismatch"):
        lc.load(nam, lc.container_doc(subs={1: odd}))


def test_mixed_container_is_still_refused_with_the_same_words(nam_lib):
    nam = nam_lib
    with open(model_path("lstm")) as f:
        lstm = json.load(f)
    lstm["sample_rate"] = 48000
    for at, first_linear in ((0, 1), (3, 0), (1, 0)):  # the LSTM first, last, in the middle: the first Linear submodel is named
        with pytest.raises(nam.NamHipError) as e:
            lc.load(nam, lc.container_doc(subs={at: copy.deepcopy(lstm)}))
        assert e.value.code == nam.ERR_UNSUPPORTED
        assert str(e.value).endswith(f"SlimmableContainer: submodel {first_linear} is a Linear model, which the device path runs only as a "
                                     "batch's one model"), str(e.value)


def test_two_channel_linear_submodel_is_refused_with_the_mono_message(nam_lib):
    nam = nam_lib
    for kw in (dict(in_ch=2, out_ch=2), dict(in_ch=1, out_ch=2), dict(in_ch=2, out_ch=1)):
        with pytest.raises(nam.NamHipError, match=r"SlimmableContainer: the device path needs mono submodels") as e:
            lc.load(nam, lc.container_doc(subs={2: lo.linear_doc(257, True, seed=257, **kw)}))
        assert e.value.code == nam.ERR_MODEL


def test_refused_as_bank_member(nam_lib):
    nam = nam_lib
    with pytest.raises(nam.NamHipError, match=r"member 0 is a SlimmableContainer whose largest submodel is not an A2-topology WaveNet") as e:
        nam.ModelBank([lc.load(nam, lc.container_doc())])
    assert e.value.code == nam.ERR_UNSUPPORTED


def test_version_prefix(nam_lib):
    assert nam_lib.load_library().nam_hip_version().decode().startswith("nam_hip 0.2.6")


def test_yardstick_for_33_taps():
    """The GPU accuracy test builds the yardstick of the 33-tap submodel itself (linear_oracle's table starts at other sizes): its
    float32 error is not zero, so FACTOR x e32 is a bound, and the truth is the direct convolution."""
    h, b = lo.taps_and_bias(lc.sub_doc(33))
    for a in lo.AMPLITUDES:
        ys = lo.Yardstick(h, b, lo.inputs(lo.n_frames_for(33), a))
        assert ys.e32 > 0 and ys.e_oldest > 0 and ys.e_newest > 0
        n = 200
        want = np.float64(b) + sum(np.float64(h[k]) * np.float64(ys.x[2, n - k]) for k in range(33))
        assert abs(ys.truth[2, n] - want) < 1e-15
        assert ys.passes(lo.split_k_fma(h, b, ys.x, 64, "oldest"))  # the kernel's order of summation, modelled on the CPU
