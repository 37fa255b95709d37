"""Model banks of the A2 family on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams each run
their own A2-topology weights on nam_kq_kernel (sessions, launches of several buffers) and nam_kt_mfma_kernel (a lone buffer).
Two kinds of check, as in tests/test_gpu_bank.py for the A1 family:
  * against the CPU oracle of the stream's OWN member: relative 5e-5 * max(1, |ref|max), the bound test_gpu_breadth.py uses for
    this kernel, and for the A2.nam member also the reference's absolute 5e-5 (tools/test/test_a2_fast.cpp:296-298);
  * bit for bit against one-model batches of the members fed the same audio through the same calls — same kernel, same sums, no
    tolerance: what catches a wrong blob stride, a stale head_scale / slope or a prewarm with the wrong member's weights.
Members: tests/golden/models/A2.nam (a container: it stands for A2-Full) and A2-topology models with seeded weights, distinct
head_scale values and distinct LeakyReLU slopes (tests/bank_models.py)."""
import os

import numpy as np
import pytest

from bank_harness import (BLOCK, Family, bit_for_bit, check_tool, drive, host_paths, load, mono, rebinding, session_against_oracle,
                          session_in_turns, singles)
from bank_models import head_scale_of, slope_of, write_a2
from conftest import model_path

pytestmark = pytest.mark.gpu

SEEDS = (401, 402, 403, 404, 405, 406, 407)
REL_BOUND = 5e-5  # test_gpu_breadth.py: test_a2_pipeline_kernel
ABS_BOUND = 5e-5  # tools/test/test_a2_fast.cpp:296-298, for A2.nam
RAGGED = BLOCK * 9 + 21


@pytest.fixture(scope="module")
def member_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("a2_bank_members")
    paths = [model_path("A2")]
    for seed in SEEDS:
        p = str(d / f"a2_{seed}.nam")
        assert write_a2(p, seed) == (head_scale_of(seed), slope_of(seed))
        paths.append(p)
    assert len({head_scale_of(s) for s in SEEDS}) == len(SEEDS) and len({slope_of(s) for s in SEEDS}) == len(SEEDS)
    return paths


@pytest.fixture(scope="module")
def family(member_paths):
    return Family(member_paths, mono)


def _assert_bounds(worst, paths):
    for m, (rel, abs_err, _) in worst.items():
        assert rel <= REL_BOUND, (m, rel)
        if os.path.basename(paths[m]) == "A2.nam":
            assert abs_err <= ABS_BOUND, (m, abs_err)


def test_a2_bank_session_every_stream_against_its_members_oracle(nam_lib, oracle, family):
    """256 streams over 8 members (stream s -> member s % 8) in persistent mode: six 64-frame commands, a flush after the third,
    after Reset with prewarm. EVERY stream against the oracle of its member."""
    _assert_bounds(session_against_oracle(nam_lib, oracle, family, "nam_kq_kernel", seed=912), family.paths)


@pytest.mark.parametrize("mode,kernel,T", [("session", "nam_kq_kernel", BLOCK * 6), ("blocks", "nam_kt_mfma_kernel", BLOCK * 6),
                                           ("launch", "nam_kq_kernel", RAGGED)])
def test_a2_bank_equals_one_model_batches_bit_for_bit(nam_lib, family, mode, kernel, T):
    """All 256 streams, np.array_equal, in the family's launch classes: the session (nam_kq_kernel), a plain launch per buffer
    (nam_kt_mfma_kernel) and one plain launch over nine buffers and a ragged tail of 21 frames (nam_kq_kernel outside a session).
    The kernel is the runtime's choice: read from kernel_name and asserted for the bank AND for the one-model batches."""
    bit_for_bit(nam_lib, family, mode, kernel, T, seed=913, n=256)


def test_a2_bank_without_the_pipeline(nam_lib, family, monkeypatch):
    """NAM_HIP_MAX_STAGES=1: nam_kt_mfma_kernel everywhere (a launch per buffer and one launch over a ragged length; the topology
    has no session then). Bit for bit against one-model batches, and the ragged launch within 1e-5 of the pipeline's output (the
    figure test_gpu_breadth.py::test_a2_pipeline_kernel uses for the two kernels)."""
    nam = nam_lib
    monkeypatch.setenv("NAM_HIP_MAX_STAGES", "1")
    bit_for_bit(nam, family, "blocks", "nam_kt_mfma_kernel", BLOCK * 6, seed=914, n=64)
    x, y_kt, member_of, models = bit_for_bit(nam, family, "launch", "nam_kt_mfma_kernel", RAGGED, seed=915, n=64)
    b = nam.ModelBank(models).batch(4, BLOCK)
    assert not b.set_persistent(True)
    b.close()
    monkeypatch.setenv("NAM_HIP_MAX_STAGES", "0")  # (no cap)
    b = nam.ModelBank(models).batch(64, RAGGED, stream_model=member_of)
    b.Reset(prewarm=True)
    y_kq, name = drive(b, x, "launch")
    b.close()
    assert name == "nam_kq_kernel"
    worst = float(np.max(np.abs(y_kq - y_kt)))
    print(f"pipeline against K-tap kernel, 64 streams x {RAGGED} frames: max |difference| {worst:.3e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("mode", ["session", "blocks"])
def test_a2_bank_per_member_scalars(nam_lib, tmp_path, mode):
    """Two members that differ ONLY in the LeakyReLU slope and two that differ ONLY in head_scale (same seed = same weights):
    outputs differ from each other and equal their one-model batches bit for bit, on both kernels."""
    nam = nam_lib
    specs = [dict(head_scale=0.05, slope=0.01), dict(head_scale=0.05, slope=0.2), dict(head_scale=0.07, slope=0.01)]
    paths = []
    for i, kw in enumerate(specs):
        paths.append(str(tmp_path / f"a2_scalar_{i}.nam"))
        write_a2(paths[-1], 450, **kw)
    models = load(nam, paths)
    bank = nam.ModelBank(models)
    n = 12
    member_of = [s % 3 for s in range(n)]
    x = np.repeat(mono(n // 3, BLOCK * 6, 916), 3, axis=0)  # streams 3 i, 3 i + 1, 3 i + 2: the same input
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = drive(b, x, mode)
    b.close()
    assert name == ("nam_kq_kernel" if mode == "session" else "nam_kt_mfma_kernel")
    want, _ = singles(nam, models, member_of, x, mode)
    for s in range(n):
        assert np.array_equal(y[s], want[s]), s
    for i in range(0, n, 3):
        assert not np.array_equal(y[i], y[i + 1])  # slope only
        assert not np.array_equal(y[i], y[i + 2])  # head_scale only
        # head_scale is a factor of the output and of nothing else
        assert np.allclose(y[i + 2], y[i] * np.float32(0.07 / 0.05), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("path", ["blocking", "tickets"])
def test_a2_bank_host_paths(nam_lib, family, path):
    """Host buffers on a 64-stream bank batch in persistent mode: blocking process calls of 64 frames, 20 back to back, and
    tickets with 8 in flight (nam_kq_kernel publishes every command). Bit for bit against one-model batches driven the same way."""
    host_paths(nam_lib, family, path, n=64, nb=(20 if path == "blocking" else 32), step=3, seed=917, depth=8, kernel="nam_kq_kernel")


def test_a2_bank_rebinding_in_a_running_session(nam_lib, family):
    """After three commands of a session, streams {1, 17, 200} move to another member. From then on they equal a freshly reset
    (prewarmed) one-model batch of the new member fed the remaining input; every other stream equals the run without the swap;
    both bit for bit. An out-of-range member or stream fails and changes nothing."""
    rebinding(nam_lib, family, "nam_kq_kernel", n=256, moved=[1, 17, 200], new=6, probe=2, seed=918)


def test_a2_bank_session_in_turns(nam_lib, oracle, family):
    """600 streams over 8 members: more workgroups than CUs, the session's workgroups take turns. Every stream finite; streams s
    and s + 8 (same member) are fed identical input in every other group of eight and must produce identical output; one stream
    of every group of eight — 75 streams, the member rotating with the group, so every member is covered — against the oracle
    (the 256-stream test above checks every stream, the pairwise equality covers the rest)."""
    _assert_bounds(session_in_turns(nam_lib, oracle, family, "nam_kq_kernel", seed=919), family.paths)


def test_a2_bank_set_kernel_and_slimmable_size(nam_lib, member_paths):
    """set_kernel: AUTO and KERNEL_A1_MFMA (what a one-model A2 batch runs), nothing else; set_slimmable_size: what a
    non-slimmable model answers, although member 0 came from a container."""
    nam = nam_lib
    models = load(nam, member_paths[:3])
    b = nam.ModelBank(models).batch(4, BLOCK)
    b.set_kernel(nam.KERNEL_A1_MFMA)
    assert b.kernel_name(BLOCK) == "nam_kt_mfma_kernel" and b.kernel_name(BLOCK * 4) == "nam_kq_kernel"
    b.set_kernel(nam.KERNEL_AUTO)
    assert b.kernel_name(BLOCK) == "nam_kt_mfma_kernel" and b.kernel_name(BLOCK * 4) == "nam_kq_kernel"
    for k in (nam.KERNEL_GENERIC, nam.KERNEL_A1, nam.KERNEL_A1_IL, nam.KERNEL_WN_REG):
        with pytest.raises(nam.NamHipError) as e:
            b.set_kernel(k)
        assert e.value.code == nam.ERR_UNSUPPORTED
    b.SetSlimmableSize(0.1)  # (A2.nam as a one-model batch would switch to A2-Lite here)
    assert b.kernel_name(BLOCK * 4) == "nam_kq_kernel"
    b.close()


def test_a2_bank_check_tool(nam_lib, tmp_path):
    """cpp/tools/bank_check: nam::ModelBank / the bank form of nam::BatchDSP / SetStreamModel through the C++ adapter, on A2
    members; a model of the other family is refused."""
    a, b = str(tmp_path / "a2_seed_a.nam"), str(tmp_path / "a2_seed_b.nam")
    write_a2(a, 461)
    write_a2(b, 462)
    check_tool([model_path("A2"), a, b], refuse=model_path("wavenet_a1_standard"))
