"""Model banks on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams each run their own WaveNet
weights, in every launch class of the interleaved-frame kernel family. Two kinds of check:
  * against the CPU oracle of the stream's OWN member, with the project's bounds as they stand (relative _tol(fast_tanh) as in
    test_gpu_breadth.py, and the reference's absolute 5e-5, tools/test/test_a2_fast.cpp:296-298);
  * bit for bit against one-model batches of the members fed the same audio through the same calls — same kernel, same sums,
    no tolerance: what catches a wrong blob stride, a stale head_scale or a prewarm with the wrong member's weights.
Members: the committed standard / lite / feather fixtures and standard-topology models with seeded weights and distinct
head_scale values (tests/bank_models.py)."""
import numpy as np
import pytest

from bank_harness import (BLOCK, Family, bit_for_bit, check_tool, drive, host_paths, load, mono, oracle_errors, rebinding,
                          session_against_oracle, session_in_turns, singles)
from bank_models import head_scale_of, write_standard
from conftest import model_path

pytestmark = pytest.mark.gpu

FIXTURES = ("wavenet_a1_standard", "synth_a1_lite", "synth_a1_feather")
SEEDS = (101, 102, 103, 104, 105)


def _tol(fast_tanh):
    return 5e-5 if fast_tanh else 1e-4


ABS_BOUND = 5e-5  # tools/test/test_a2_fast.cpp:296-298


@pytest.fixture(scope="module")
def member_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("bank_members")
    paths = [model_path(n) for n in FIXTURES]
    for seed in SEEDS:
        p = str(d / f"standard_{seed}.nam")
        assert write_standard(p, seed) == head_scale_of(seed)
        paths.append(p)
    assert len({head_scale_of(s) for s in SEEDS}) == len(SEEDS)
    return paths


@pytest.fixture(scope="module")
def family(member_paths):
    # (il_singles: a lone 64-frame launch of a one-model batch runs nam_a1_mfma_kernel under AUTO; the bank runs the A1_IL family)
    return Family(member_paths, mono, il_singles=True)


def _assert_bounds(worst, fast_tanh=True):
    for m, (rel, abs_err, _) in worst.items():
        assert rel <= _tol(fast_tanh), (m, rel)
        assert abs_err <= (ABS_BOUND if fast_tanh else 1e-4), (m, abs_err)


def test_bank_session_every_stream_against_its_members_oracle(nam_lib, oracle, family):
    """256 streams over 8 members (stream s -> member s % 8) in persistent mode: six 64-frame commands, a flush after the third
    (the shape of test_gpu_breadth.py::test_bench_shapes_every_stream_in_persistent_mode). EVERY stream against the oracle
    of its member. The sharp members are the committed fixtures (|y| ~ 0.1 - 1); the seeded ones (|y|max 0.02 - 0.05) sit far
    inside the absolute bound — for them the bit-for-bit tests below are the sharp check."""
    _assert_bounds(session_against_oracle(nam_lib, oracle, family, "nam_a1_q_kernel", seed=902))


@pytest.mark.parametrize("mode,kernel", [("session", "nam_a1_q_kernel"), ("bursts", "nam_a1_p4_kernel"), ("blocks", "nam_a1_p2_kernel"),
                                         ("launch", "nam_a1_q_kernel")])
def test_bank_equals_one_model_batches_bit_for_bit(nam_lib, family, mode, kernel):
    """All 256 streams, np.array_equal, in the family's launch classes: the session (nam_a1_q_kernel), a session whose caller
    flushes after every buffer (its launches become nam_a1_p4_kernel after three bursts), a plain launch per buffer
    (nam_a1_p2_kernel) and one plain launch over eight buffers (nam_a1_q_kernel again, outside a session). The kernel is the
    runtime's choice: read from kernel_name and asserted for the bank AND for the one-model batches."""
    nb = 8 if mode in ("bursts", "launch") else 6
    bit_for_bit(nam_lib, family, mode, kernel, BLOCK * nb, seed=903, n=256)


def test_bank_tanh_instantiation_bit_for_bit(nam_lib, oracle, member_paths):
    """fast_tanh=False: the ACT_TANH instantiations, 32 streams, session; bit for bit and four streams against the oracle."""
    nam = nam_lib
    n = 32
    models = load(nam, member_paths, fast_tanh=False)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = mono(n, BLOCK * 6, 904)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = drive(b, x, "session")
    b.close()
    assert name == "nam_a1_q_kernel"
    want, names = singles(nam, models, member_of, x, "session")
    assert names == {"nam_a1_q_kernel"}
    assert all(np.array_equal(y[s], want[s]) for s in range(n))
    _assert_bounds(oracle_errors(oracle, member_paths, member_of, x, y, (0, 9, 18, 31), fast_tanh=False), fast_tanh=False)


@pytest.mark.parametrize("path", ["blocking", "tickets"])
def test_bank_host_paths(nam_lib, oracle, member_paths, family, path):
    """Host buffers on a 64-stream bank batch in persistent mode: blocking process calls of 64 frames, 20 back to back (the
    lingering launch serves them), and tickets with 16 in flight. Bit for bit against one-model batches driven the same way;
    five streams against the oracle."""
    x, y, member_of = host_paths(nam_lib, family, path, n=64, nb=(20 if path == "blocking" else 32), step=3, seed=905, depth=16)
    _assert_bounds(oracle_errors(oracle, member_paths, member_of, x, y, (0, 13, 27, 42, 63)))


def test_bank_rebinding_in_a_running_session(nam_lib, family):
    """After three commands of a session, streams {1, 17, 200} move to another member. From then on they equal a freshly
    reset (prewarmed) one-model batch of the new member fed the remaining input; every other stream equals the run without
    the swap; both bit for bit. An out-of-range member or stream fails and changes nothing."""
    nam = nam_lib
    bank, models = rebinding(nam, family, "nam_a1_q_kernel", n=256, moved=[1, 17, 200], new=6, probe=2, seed=906)
    # set_kernel: the family only; set_slimmable_size: what a non-slimmable model answers
    b = bank.batch(4, BLOCK)
    b.set_kernel(nam.KERNEL_A1_IL)
    b.set_kernel(nam.KERNEL_AUTO)
    for k in (nam.KERNEL_GENERIC, nam.KERNEL_A1, nam.KERNEL_A1_MFMA, nam.KERNEL_WN_REG):
        with pytest.raises(nam.NamHipError) as e:
            b.set_kernel(k)
        assert e.value.code == nam.ERR_UNSUPPORTED
    b.SetSlimmableSize(0.5)
    b.close()
    one = models[0].batch(2, BLOCK)  # a one-model batch has no members to set
    with pytest.raises(nam.NamHipError):
        one.set_stream_model(0)
    assert one.stream_model(1) == 0
    one.close()


def test_bank_session_in_turns(nam_lib, oracle, family):
    """600 streams over 8 members: more workgroups than CUs, the session's workgroups take turns. Every stream finite; streams
    s and s + 8 (same member) are fed identical input in every other group of eight and must produce identical output; one
    stream of every group of eight — 75 streams, the member rotating with the group — against the oracle (a fixed cap: the
    256-stream test above checks every stream, the pairwise equality covers the rest)."""
    _assert_bounds(session_in_turns(nam_lib, oracle, family, "nam_a1_q_kernel", seed=907))


def test_bank_check_tool(nam_lib):
    """cpp/tools/bank_check: nam::ModelBank / the bank form of nam::BatchDSP / SetStreamModel through the C++ adapter."""
    check_tool([model_path(n) for n in FIXTURES], refuse=model_path("lstm"))
