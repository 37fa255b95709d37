"""Model banks on the host side (include/nam_hip.h: nam_hip_bank_create is host-only): which sets of models one batch may run
side by side, what is refused and how the refusal names its member, and that a bank owns what it needs."""
import ctypes

import pytest

from bank_harness import fixture, refused, survives_its_models
from bank_models import write_standard
from conftest import model_path


def _seeded(nam, tmp_path, seed, fast_tanh=True):
    p = str(tmp_path / f"bank_{seed}.nam")
    write_standard(p, seed)
    return nam.get_dsp(p, fast_tanh=fast_tanh)


def test_bank_accepts_the_official_sizes_and_seeded_standards(nam_lib, tmp_path):
    nam = nam_lib
    models = [fixture(nam, "wavenet_a1_standard"), fixture(nam, "synth_a1_lite"), fixture(nam, "synth_a1_feather"),
              _seeded(nam, tmp_path, 101), _seeded(nam, tmp_path, 102)]
    bank = nam.ModelBank(models)
    assert len(bank) == 5
    assert len(nam.ModelBank(models[:1])) == 1  # a bank of one model is legal
    # ... with Tanh (fast tanh off) as well: the other activation instantiation
    assert len(nam.ModelBank([fixture(nam, "wavenet_a1_standard", False), fixture(nam, "synth_a1_lite", False)])) == 2


def test_bank_refusals_name_the_member(nam_lib, tmp_path):
    nam = nam_lib
    std = fixture(nam, "wavenet_a1_standard")
    refused(nam, [std, fixture(nam, "lstm")], 1)
    refused(nam, [std, fixture(nam, "synth_a1_nano")], 1)
    refused(nam, [std, std, fixture(nam, "synth_a1_feather_relu")], 2)  # another activation (and its own width: no nam_a1_q_kernel plan)
    refused(nam, [fixture(nam, "synth_a1_feather_relu"), std], 0)
    refused(nam, [std, fixture(nam, "slimmable_wavenet")], 1)
    refused(nam, [std, fixture(nam, "A2")], 1)
    # two standards loaded with different fast_tanh: ACT_FASTTANH next to ACT_TANH, two kernel instantiations
    msg = refused(nam, [std, _seeded(nam, tmp_path, 103, fast_tanh=False)], 1)
    assert "fast_tanh" in msg
    # a lookup table replaces the activation the kernels are compiled for
    lut = nam.get_dsp(model_path("wavenet_a1_standard"), fast_tanh=False, luts={"Tanh": (-5.0, 5.0, 1024)})
    refused(nam, [fixture(nam, "wavenet_a1_standard", False), lut], 1)


def test_bank_bad_arguments(nam_lib):
    nam = nam_lib
    L = nam.load_library()
    std = fixture(nam, "wavenet_a1_standard")
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 2)(std._h.value, None)
    assert L.nam_hip_bank_create(arr, 0, ctypes.byref(h)) == nam.ERR_INVALID_ARGUMENT
    assert L.nam_hip_bank_create(arr, 2, ctypes.byref(h)) == nam.ERR_INVALID_ARGUMENT
    assert b"member 1" in L.nam_hip_last_error()
    assert L.nam_hip_bank_create(None, 1, ctypes.byref(h)) == nam.ERR_INVALID_ARGUMENT
    assert L.nam_hip_bank_create(arr, 1, None) == nam.ERR_INVALID_ARGUMENT
    assert h.value is None
    assert L.nam_hip_bank_n_models(None) == nam.ERR_INVALID_ARGUMENT
    L.nam_hip_bank_free(None)  # like free(NULL)
    with pytest.raises(nam.NamHipError) as e:
        nam.ModelBank([])
    assert e.value.code == nam.ERR_INVALID_ARGUMENT
    # the member binding calls refuse what is not a bank batch / not a batch (no device needed to say so)
    assert L.nam_hip_batch_set_stream_model(None, None, 0, 0) == nam.ERR_INVALID_ARGUMENT
    assert L.nam_hip_batch_get_stream_model(None, 0) == nam.ERR_INVALID_ARGUMENT
    assert L.nam_hip_batch_create_bank(None, 0, 4, 64, None, ctypes.byref(h)) == nam.ERR_INVALID_ARGUMENT


def test_bank_survives_its_models(nam_lib, tmp_path):
    """The bank copies what it needs: the member models are freed (their handles through nam_hip_model_free) before the bank
    is asked anything, and a second bank over the same files is built while the first lives."""
    survives_its_models(nam_lib, [model_path("wavenet_a1_standard"), model_path("synth_a1_lite")],
                        lambda: [_seeded(nam_lib, tmp_path, 200 + i) for i in range(3)])


def test_version_says_banks(nam_lib):
    v = nam_lib.load_library().nam_hip_version().decode()
    assert tuple(int(t) for t in v.split()[1].split(".")) >= (0, 2, 2), v
