"""Model banks of the A2 family on the host side (include/nam_hip.h: nam_hip_bank_create is host-only): A2-topology WaveNets and
the containers A2 captures ship in share a batch on nam_kq_kernel / nam_kt_mfma_kernel; what is refused and how the refusal names
its member; that such a bank owns what it needs. The A1 family's side is tests/test_bank_abi.py."""
import pytest

from bank_harness import fixture, refused, survives_its_models
from bank_models import write_a2
from conftest import model_path


def _seeded(nam, tmp_path, seed, fast_tanh=True, **kw):
    p = str(tmp_path / f"a2_bank_{seed}_{kw.get('act', 'LeakyReLU')}.nam")
    write_a2(p, seed, **kw)
    return nam.get_dsp(p, fast_tanh=fast_tanh)


def test_a2_bank_accepts_the_container_and_seeded_members(nam_lib, tmp_path):
    nam = nam_lib
    # a container (A2-Lite + A2-Full: it stands for A2-Full) next to plain WaveNets of the topology; three LeakyReLU slopes
    models = [fixture(nam, "A2"), _seeded(nam, tmp_path, 301), _seeded(nam, tmp_path, 302)]
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
    a2 = fixture(nam, "A2")
    seeded = _seeded(nam, tmp_path, 330)
    std = fixture(nam, "wavenet_a1_standard")
    # one family per bank, in either order: the LATER member is the one that differs
    assert "family" in refused(nam, [a2, std], 1)
    assert "family" in refused(nam, [std, a2], 1)
    assert "family" in refused(nam, [seeded, seeded, std], 2)
    refused(nam, [a2, fixture(nam, "lstm")], 1)
    # the activation TYPE is a template argument of both kernels; LeakyReLU slopes may differ, the type may not
    msg = refused(nam, [seeded, _seeded(nam, tmp_path, 331, act="Tanh")], 1)
    assert "act" in msg
    msg = refused(nam, [_seeded(nam, tmp_path, 332, act="Tanh"), seeded], 1)
    assert "act" in msg
    # Tanh next to Fasttanh (two loads of the same kind of file with different fast_tanh)
    refused(nam, [_seeded(nam, tmp_path, 333, fast_tanh=True, act="Tanh"), _seeded(nam, tmp_path, 334, fast_tanh=False, act="Tanh")], 1)
    # ReLU is a type of its own (nam_kt_mfma_kernel runs it through another instantiation than LeakyReLU)
    refused(nam, [seeded, _seeded(nam, tmp_path, 335, act="ReLU")], 1)
    # the topology with an activation nam_kq_kernel is not compiled for
    refused(nam, [a2, _seeded(nam, tmp_path, 336, act="Sigmoid")], 1)
    refused(nam, [_seeded(nam, tmp_path, 336, act="Sigmoid")], 0)
    # a lookup table replaces the activation the kernels are compiled for
    p = str(tmp_path / "a2_tanh_lut.nam")
    write_a2(p, 337, act="Tanh")
    lut = nam.get_dsp(p, fast_tanh=False, luts={"Tanh": (-5.0, 5.0, 1024)})
    refused(nam, [_seeded(nam, tmp_path, 338, fast_tanh=False, act="Tanh"), lut], 1)
    refused(nam, [lut], 0)
    # K-tap, 8 channels, LeakyReLU — but not the topology (no nam_kq_kernel plan)
    refused(nam, [a2, fixture(nam, "synth_kt_c8")], 1)
    refused(nam, [fixture(nam, "synth_kt_c8"), a2], 0)
    # what no family takes stays refused next to an A2 member too
    refused(nam, [a2, fixture(nam, "slimmable_wavenet")], 1)
    refused(nam, [a2, fixture(nam, "synth_a1_nano")], 1)


def test_a2_bank_survives_its_models(nam_lib, tmp_path):
    """The bank copies what it needs — for a container member its largest submodel's spec and plan: the member models are freed
    (their handles through nam_hip_model_free) before the bank is asked anything."""
    seeded = str(tmp_path / "a2_survivor.nam")
    write_a2(seeded, 340)
    survives_its_models(nam_lib, [model_path("A2"), seeded], lambda: [_seeded(nam_lib, tmp_path, 341 + i) for i in range(3)])


def test_version_says_a2_banks(nam_lib):
    v = nam_lib.load_library().nam_hip_version().decode()
    assert tuple(int(t) for t in v.split()[1].split(".")) >= (0, 2, 3), v
