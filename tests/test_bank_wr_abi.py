"""Model banks of the nam_wn_reg_kernel family on the host side (include/nam_hip.h: nam_hip_bank_create is host-only): models a
one-model batch runs on nam_wn_reg_kernel under AUTO — the official nano size, a nested condition_dsp ... — share a batch when they
have ONE program (csrc/plan.h: WrPlan::structure_key); head_scale is per member although a per-model code object has it compiled
in. What is admitted, what is refused and how the refusal names its member and the field, and that such a bank owns what it needs.
Before the family existed nam_hip_bank_create refused a nano as member 0. The other families' sides: tests/test_bank_abi.py,
tests/test_bank_a2_abi.py, tests/test_bank_lstm_abi.py."""
import os
import subprocess
import sys

import pytest

from bank_harness import BLOCK, fixture, load, mono, refused, survives_its_models
from bank_wr_models import NANO_HEAD_SCALE, NANO_OTHER_SCALE, check_members, write_all
from conftest import ROOT, model_path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_all(tmp_path_factory.mktemp("wr_bank_members"))


def admission_checks(nam, files):
    """Three nano members make a bank of three that survives its models; two nano members with DIFFERENT head_scale are admitted."""
    nano = files["nano"]
    assert len(nam.ModelBank(load(nam, nano[:3]))) == 3
    survives_its_models(nam, nano[:2], lambda: load(nam, nano[2:5]))
    other = NANO_OTHER_SCALE[0]
    assert NANO_OTHER_SCALE[1] != NANO_HEAD_SCALE
    for pair in ([nano[0], nano[other]], [nano[other], nano[0]]):
        assert len(nam.ModelBank(load(nam, pair))) == 2


def test_members_are_finite_audible_and_distinct(oracle, files):
    """On the CPU oracle, on the harness signal: what the GPU tests' comparisons rely on."""
    x = mono(1, BLOCK * 6, 930)[0]
    for kind in ("nano", "cond", "head"):
        peaks = check_members(oracle, files[kind], x)
        print(kind, " ".join(f"{p:.4f}" for p in peaks))


def test_wr_bank_accepts_nano_members(nam_lib, files):
    admission_checks(nam_lib, files)
    nam = nam_lib
    # the fixture itself next to seeded members, and the nested condition_dsp's redraws; with libm tanh as well
    assert len(nam.ModelBank([fixture(nam, "synth_a1_nano")] + load(nam, files["nano"]))) == 9
    assert len(nam.ModelBank([fixture(nam, "wavenet_condition_dsp")] + load(nam, files["cond"]))) == 4
    assert len(nam.ModelBank([fixture(nam, "synth_posthead")] + load(nam, files["head"]))) == 4  # (a post-stack head)
    assert len(nam.ModelBank(load(nam, files["nano"][:2], fast_tanh=False))) == 2
    assert len(nam.ModelBank(load(nam, files["nano"][:1]))) == 1  # a bank of one model is legal


@pytest.mark.parametrize("switch", ["NAM_HIP_JIT", "NAM_HIP_WR_PROGRAM"])
def test_wr_bank_accepts_nano_members_without_a_compiled_in_program(files, switch):
    """NAM_HIP_JIT=0 (no per-model code object: the ahead-of-time instantiations walk the program) and NAM_HIP_WR_PROGRAM=0 (the
    ahead-of-time shapes come first): the same admissions. The planner reads the second switch once per process, so the loads run
    in a process of their own with the switch set from its start."""
    env = dict(os.environ)
    env[switch] = "0"
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import conftest, test_bank_wr_abi as t\n"
            "import neuralampmodelercore_amd as nam\n"
            "nam.load_library()\n"
            "files = dict(nano=%r)\n"
            "t.admission_checks(nam, files)\n"
            "print('admitted')\n") % (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle"), files["nano"])
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "admitted" in r.stdout, r.stdout + r.stderr


def test_wr_bank_refusals_name_the_member_and_the_field(nam_lib, files):
    nam = nam_lib
    nano = fixture(nam, "synth_a1_nano")
    seeded = load(nam, files["nano"][:2])
    cond = load(nam, files["cond"][:1])[0]
    # another program (a nested condition_dsp, other arrays): the first field that differs is the receptive field's prewarm
    assert "differs from member 0 in prewarm_samples (45 vs 4093)" in refused(nam, [nano, seeded[0], cond], 2)
    assert "differs from member 0 in prewarm_samples (4093 vs 45)" in refused(nam, [cond, nano], 1)
    # ... and between two programs of one prewarm length and one state size, the program itself
    msg = refused(nam, [nano, nam.get_dsp(files["nano_nobias"], fast_tanh=True)], 1)
    assert "wr.structure_key" in msg, msg
    # ACT_TANH next to ACT_FASTTANH: two run shapes
    assert "fast_tanh" in refused(nam, [nano, load(nam, files["nano"][2:3], fast_tanh=False)[0]], 1)
    assert "fast_tanh" in refused(nam, [fixture(nam, "synth_a1_nano", False), seeded[1]], 1)
    # one dilation changed (512 -> 256 in the second array): another receptive field, other rings
    msg = refused(nam, [nano, seeded[0], nam.get_dsp(files["nano_dil"], fast_tanh=True)], 2)
    assert any(f in msg for f in ("prewarm_samples", "state_floats", "wr.structure_key")), msg
    # one family per bank, in either order: the LATER member is the one that differs
    std, lstm = fixture(nam, "wavenet_a1_standard"), fixture(nam, "lstm")
    for a, b in ((nano, std), (std, nano), (nano, lstm), (lstm, nano)):
        assert "family" in refused(nam, [a, b], 1)
    assert "family" in refused(nam, [nano, seeded[0], fixture(nam, "A2")], 2)
    # a slimmable WaveNet runs nam_wn_reg_kernel too, but its widths are separate plans
    assert "slimmable" in refused(nam, [fixture(nam, "slimmable_wavenet"), nano], 0)
    # a lookup table replaces the activation: no nam_wn_reg_kernel plan, and the refusal says why
    lut = nam.get_dsp(model_path("synth_a1_nano"), fast_tanh=False, luts={"Tanh": (-5.0, 5.0, 1024)})
    msg = refused(nam, [lut, fixture(nam, "synth_a1_nano", False)], 0)
    assert "nam_wn_reg_kernel plan" in msg and "look-up-table" in msg, msg


def test_version_says_wn_reg_banks(nam_lib):
    v = nam_lib.load_library().nam_hip_version().decode()
    assert tuple(int(t) for t in v.split()[1].split(".")) >= (0, 2, 5), v
