"""A SlimmableContainer of the official WaveNet topology's tiers (tests/a1_mixed.py) at load time: whether it has the mixed-size
residency of persistent mode is decided once per model, by the rules a BANK_A1_IL model bank admits its members by, and
NAM_HIP_FIELD_DESCRIPTION says which way it went. No GPU: plans are built on the host. The C ABI and the version string do not move
(the feature lives inside the existing entry points)."""
import a1_mixed as am


def container_note(model):
    """the sentence about the container in the description line"""
    notes = [part for part in model.describe().split(" | ") if part.startswith("container: ")]
    assert len(notes) == 1, model.describe()
    return notes[0]


def test_three_tier_container_qualifies(nam_lib):
    m = am.load(nam_lib)
    assert m.architecture == "SlimmableContainer" and m.is_slimmable
    assert m.GetSlimmableSizeBreakpoints() == list(am.MAX_VALUES[:-1])  # (the last submodel takes every ratio above)
    d = m.describe()
    assert d.count("plan ") >= 3 and d.count("a1_p2=1") == 3, d  # feather, lite and standard each plan onto the interleaved-frame kernels
    note = container_note(m)
    assert "a1_mixed_session=1" in note and "nam_a1_q_kernel" in note, note
    # the same with libm tanh: the tiers still share one activation and one fast_tanh
    assert "a1_mixed_session=1" in container_note(am.load(nam_lib, fast_tanh=False))


def test_four_tier_container_names_the_first_difference(nam_lib):
    m = am.load(nam_lib, am.four_tier_doc())
    assert m.is_slimmable and m.GetSlimmableSizeBreakpoints() == [0.1, 0.25, 0.5]
    note = container_note(m)
    # the nano tier (4 / 2 channels, head_size 2) is of nam_wn_reg_kernel's family: submodel 0, and the field is the family
    assert "a1_mixed_session=0" in note and "submodel 0 differs from the largest submodel in family" in note, note
    assert "WN_REG" in note and "A1_IL" in note, note


def test_another_activation_does_not_qualify(nam_lib):
    m = am.load(nam_lib, am.relu_doc())
    note = container_note(m)
    assert "a1_mixed_session=0" in note and "submodel 0 is" in note, note
    assert "Tanh or Fasttanh" in note or "activation" in note, note  # (what nam_hip_bank_create says of synth_a1_feather_relu)


def test_other_models_say_nothing_about_it(nam_lib):
    from conftest import model_path
    for name in ("wavenet_a1_standard", "A2", "synth_a1_lite"):
        assert "a1_mixed_session" not in nam_lib.get_dsp(model_path(name), fast_tanh=True).describe(), name


def test_abi_and_version_are_where_they_were(nam_lib):
    assert len(nam_lib.ABI_SYMBOLS) == len(set(nam_lib.ABI_SYMBOLS)) == 45
    assert nam_lib.load_library().nam_hip_version().decode().startswith("nam_hip 0.2.6")
