"""Model banks of the A2 family on the host side (include/nam_hip.h: nam_hip_bank_create is host-only): A2-topology WaveNets and
the containers A2 captures ship in share a batch on nam_kq_kernel / nam_kt_mfma_kernel; what is refused and how the refusal names
its member; that such a bank owns what it needs. The A1 family's side is tests/test_bank_abi.py."""
import ctypes
import gc

import pytest

from bank_models_a2 import write_a2
from conftest import model_path


def _seeded(nam, tmp_path, seed, fast_tanh=True, **kw):
    p = str(tmp_path / f"a2_bank_{seed}_{kw.get('act', 'LeakyReLU')}.nam")
    write_a2(p, seed, **kw)
    return nam.get_dsp(p, fast_tanh=fast_tanh)


def _fixture(nam, name, fast_tanh=True):
    return nam.get_dsp(model_path(name), fast_tanh=fast_tanh)


def _refused(nam, models, member):
    with pytest.raises(nam.NamHipError) as e:
        nam.ModelBank(models)
    assert e.value.code == nam.ERR_UNSUPPORTED, str(e.value)
    assert f"member {member}" in str(e.value), str(e.value)
    return str(e.value)


def test_a2_bank_accepts_the_container_and_seeded_members(nam_lib, tmp_path):
    nam = nam_lib
    # a container (A2-Lite + A2-Full: it stands for A2-Full) next to plain WaveNets of the topology; three LeakyReLU slopes
    models = [_fixture(nam, "A2"), _seeded(nam, tmp_path, 301), _seeded(nam, tmp_path, 302)]
    assert len(nam.ModelBank(models)) == 3
    assert len(nam.ModelBank(models[::-1])) == 3  # ... in any order
    assert len(nam.ModelBank(models[:1])) == 1  # a bank of one model is legal
    assert len(nam.ModelBank(models[1:2])) == 1


@pytest.mark.parametrize("fast_tanh", [True, False])
def test_a2_bank_accepts_tanh_members(nam_lib, tmp_path, fast_tanh):
    """Tanh members: ACT_FASTTANH with fast_tanh on, ACT_TANH off — the other two activation instantiations of nam_kq_kernel."""
    nam = nam_lib
    models = [_seeded(nam, tmp_path, 310 + i, fast_tanh=fast_tanh, act="Tanh") for i in range(2)]
    assert len(nam.ModelBank(models)) == 2


def test_a2_bank_accepts_relu_members(nam_lib, tmp_path):
    nam = nam_lib
    assert len(nam.ModelBank([_seeded(nam, tmp_path, 320 + i, act="ReLU") for i in range(2)])) == 2


def test_a2_bank_refusals_name_the_member(nam_lib, tmp_path):
    nam = nam_lib
    a2 = _fixture(nam, "A2")
    seeded = _seeded(nam, tmp_path, 330)
    std = _fixture(nam, "wavenet_a1_standard")
    # one family per bank, in either order: the LATER member is the one that differs
    assert "family" in _refused(nam, [a2, std], 1)
    assert "family" in _refused(nam, [std, a2], 1)
    assert "family" in _refused(nam, [seeded, seeded, std], 2)
    _refused(nam, [a2, _fixture(nam, "lstm")], 1)
    # the activation TYPE is a template argument of both kernels; LeakyReLU slopes may differ, the type may not
    msg = _refused(nam, [seeded, _seeded(nam, tmp_path, 331, act="Tanh")], 1)
    assert "act" in msg
    msg = _refused(nam, [_seeded(nam, tmp_path, 332, act="Tanh"), seeded], 1)
    assert "act" in msg
    # Tanh next to Fasttanh (two loads of the same kind of file with different fast_tanh)
    _refused(nam, [_seeded(nam, tmp_path, 333, fast_tanh=True, act="Tanh"), _seeded(nam, tmp_path, 334, fast_tanh=False, act="Tanh")], 1)
    # ReLU is a type of its own (nam_kt_mfma_kernel runs it through another instantiation than LeakyReLU)
    _refused(nam, [seeded, _seeded(nam, tmp_path, 335, act="ReLU")], 1)
    # the topology with an activation nam_kq_kernel is not compiled for
    _refused(nam, [a2, _seeded(nam, tmp_path, 336, act="Sigmoid")], 1)
    _refused(nam, [_seeded(nam, tmp_path, 336, act="Sigmoid")], 0)
    # a lookup table replaces the activation the kernels are compiled for
    p = str(tmp_path / "a2_tanh_lut.nam")
    write_a2(p, 337, act="Tanh")
    lut = nam.get_dsp(p, fast_tanh=False, luts={"Tanh": (-5.0, 5.0, 1024)})
    _refused(nam, [_seeded(nam, tmp_path, 338, fast_tanh=False, act="Tanh"), lut], 1)
    _refused(nam, [lut], 0)
    # K-tap, 8 channels, LeakyReLU — but not the topology (no nam_kq_kernel plan)
    _refused(nam, [a2, _fixture(nam, "synth_kt_c8")], 1)
    _refused(nam, [_fixture(nam, "synth_kt_c8"), a2], 0)
    # what no family takes stays refused next to an A2 member too
    _refused(nam, [a2, _fixture(nam, "slimmable_wavenet")], 1)
    _refused(nam, [a2, _fixture(nam, "synth_a1_nano")], 1)


def test_a2_bank_survives_its_models(nam_lib, tmp_path):
    """The bank copies what it needs — for a container member its largest submodel's spec and plan: the member models are freed
    (their handles through nam_hip_model_free) before the bank is asked anything."""
    nam = nam_lib
    L = nam.load_library()
    seeded = str(tmp_path / "a2_survivor.nam")
    write_a2(seeded, 340)
    handles = []
    for path in (model_path("A2"), seeded):
        h = ctypes.c_void_p()
        assert L.nam_hip_model_load(path.encode(), 1, ctypes.byref(h)) == 0
        handles.append(h)
    arr = (ctypes.c_void_p * 2)(*[h.value for h in handles])
    bank = ctypes.c_void_p()
    assert L.nam_hip_bank_create(arr, 2, ctypes.byref(bank)) == 0, L.nam_hip_last_error()
    for h in handles:
        L.nam_hip_model_free(h)
    junk = [_seeded(nam, tmp_path, 341 + i) for i in range(3)]  # (allocations over the freed models' memory)
    assert L.nam_hip_bank_n_models(bank) == 2
    # a stream_model entry outside the bank is refused before any device call
    out = ctypes.c_void_p()
    bad = (ctypes.c_int * 4)(0, 1, 2, 0)
    assert L.nam_hip_batch_create_bank(bank, 0, 4, 64, bad, ctypes.byref(out)) == nam.ERR_INVALID_ARGUMENT
    assert b"member 2" in L.nam_hip_last_error() and out.value is None
    L.nam_hip_bank_free(bank)
    del junk
    gc.collect()


def test_version_says_a2_banks(nam_lib):
    v = nam_lib.load_library().nam_hip_version().decode()
    assert tuple(int(t) for t in v.split()[1].split(".")) >= (0, 2, 3), v
