"""Model banks of the nam_wn_reg_kernel family on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams
each run their own capture on nam_wn_reg_kernel — a workgroup's prologue copies its stream's MEMBER's blob to LDS, and a per-model
code object (member 0's) takes head_scale from the member's own op table instead of its compiled-in constant. Two kinds of check,
as for the other families (tests/test_gpu_bank.py, _a2, _lstm):
  * against the CPU oracle of the stream's OWN member: 5e-5 x max(1, |ref|max) with fast tanh, 1e-4 with libm tanh — the bounds
    tests/test_gpu_breadth.py uses for this kernel;
  * bit for bit against one-model batches of the members fed the same audio through the same calls. With a dozen streams the bank
    and the one-model batches run the same form of the kernel (one, two or four wavefronts per stream: launch_wr decides on the
    stream count), so equality is of the same code on the same sums; NAM_HIP_MAX_STAGES = 1 / 2 / 4 puts each form's prologue
    in front of member blobs.
Members (tests/bank_wr_models.py): `nano` — eight seeded models of the official nano size, one of them with another head_scale
(another generated header, another code object: the bank runs member 0's for all eight); `cond` — three redraws of
wavenet_condition_dsp.nam (a nested WaveNet as condition: two compiled-in scales, both per member); `head` — three redraws of
synth_posthead.nam (a post-stack head, two output channels: head_scale is compiled into the head's first layer).
No bank test reaches the dense (two wavefronts per SIMD) forms: launch_wr picks none for a nano batch of up to 1,536 streams
(profiles/bank_wn_reg/README.md); their prologue is the same code."""
import numpy as np
import pytest

from bank_harness import (BLOCK, Family, bit_for_bit, check_tool, drive, host_paths, load, mono, oracle_errors, rebinding,
                          session_against_oracle, session_in_turns)
from bank_wr_models import NANO_OTHER_SCALE, write_all
from conftest import model_path

pytestmark = pytest.mark.gpu

KERNEL = "nam_wn_reg_kernel"
BOUND_FAST, BOUND_LIBM = 5e-5, 1e-4  # x max(1, |ref|max): tests/test_gpu_breadth.py, nam_wn_reg_kernel
RAGGED = 3 * BLOCK + 11


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_all(tmp_path_factory.mktemp("wr_bank_members"))


@pytest.fixture(scope="module")
def families(files):
    return dict(nano=Family(files["nano"], mono), cond=Family(files["cond"], mono), head=Family(files["head"], mono))


def _assert_bound(worst, bound):
    for m, (rel, _, _) in worst.items():
        assert rel <= bound, (m, rel)


def test_wr_bank_session_every_stream_against_its_members_oracle(nam_lib, oracle, families):
    """256 streams over the eight nano members (stream s -> member s % 8) in persistent mode: six 64-frame commands, a flush after
    the third, after Reset with prewarm. EVERY stream against the oracle of its member."""
    _assert_bound(session_against_oracle(nam_lib, oracle, families["nano"], KERNEL, seed=931), BOUND_FAST)


def test_wr_bank_session_with_libm_tanh(nam_lib, oracle, families):
    """Twelve streams with fast tanh off (ACT_TANH: the other run shapes, other code objects)."""
    nam, fam = nam_lib, families["nano"]
    n = 12
    bank = nam.ModelBank(load(nam, fam.paths, fast_tanh=False))
    member_of = [s % len(fam.paths) for s in range(n)]
    x = fam.signal(n, BLOCK * 6, 932)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = drive(b, x, "session")
    b.close()
    assert name == KERNEL and np.isfinite(y).all()
    worst = oracle_errors(oracle, fam.paths, member_of, x, y, range(n), fast_tanh=False)
    assert sorted(worst) == list(range(len(fam.paths)))
    _assert_bound(worst, BOUND_LIBM)


# (mode, frames, NAM_HIP_MAX_STAGES or None): the kernel's launch classes — the session, a session flushed after every buffer, a
# plain launch per buffer, one plain launch over three buffers and a ragged tail of 11 frames — and the session once more as one, at
# most two, at most four wavefronts per stream (the switch is read when a batch is made): every form of the prologue loads member
# blobs, the waves of a workgroup sharing the copy
CASES = [("session", BLOCK * 6, None), ("bursts", BLOCK * 6, None), ("blocks", BLOCK * 6, None), ("launch", RAGGED, None),
         ("session", BLOCK * 6, 1), ("session", BLOCK * 6, 2), ("session", BLOCK * 6, 4)]


@pytest.mark.parametrize("mode,T,stages", CASES)
@pytest.mark.parametrize("kind", ["nano", "cond", "head"])
def test_wr_bank_equals_one_model_batches_bit_for_bit(nam_lib, families, kind, mode, T, stages, monkeypatch):
    """Twelve streams, np.array_equal; the kernel is asserted for the bank AND for the one-model batches."""
    if stages:
        monkeypatch.setenv("NAM_HIP_MAX_STAGES", str(stages))
    bit_for_bit(nam_lib, families[kind], mode, KERNEL, T, seed=933, n=12)


@pytest.mark.parametrize("mode,T,stages", CASES)
def test_wr_bank_bit_for_bit_without_per_model_code_objects(nam_lib, families, mode, T, stages, monkeypatch):
    """NAM_HIP_JIT=0, read when a model is loaded: the ahead-of-time instantiations walk each member's program from the LDS copy of
    its own blob, the scales included."""
    monkeypatch.setenv("NAM_HIP_JIT", "0")
    if stages:
        monkeypatch.setenv("NAM_HIP_MAX_STAGES", str(stages))
    bit_for_bit(nam_lib, families["nano"], mode, KERNEL, T, seed=935, n=12)


def test_wr_bank_rebinding_in_a_running_session(nam_lib, families):
    """After three commands of a session, streams {1, 7} move onto the member with the other head_scale. From then on they equal a
    freshly reset (prewarmed) one-model batch of that member — which runs ITS code object, the bank member 0's — fed the remaining
    input; every other stream equals the run without the move; both bit for bit."""
    rebinding(nam_lib, families["nano"], KERNEL, n=12, moved=[1, 7], new=NANO_OTHER_SCALE[0], probe=2, seed=936)


@pytest.mark.parametrize("path", ["blocking", "tickets"])
def test_wr_bank_host_paths(nam_lib, families, path):
    """Host buffers on an eight-stream bank batch in persistent mode: six blocking process calls of 64 frames back to back, and
    tickets with four in flight. Bit for bit against one-model batches driven the same way."""
    host_paths(nam_lib, families["nano"], path, n=8, nb=6, step=3, seed=937, depth=4, kernel=KERNEL)


def test_wr_bank_session_in_turns(nam_lib, oracle, families):
    """600 streams over the eight nano members: more workgroups than the chip holds at once (the session runs four wavefronts per
    stream, one 104 KB workgroup per CU), the session's workgroups take turns. Every stream finite; streams s and s + 8 (same member) fed identical input produce identical output;
    75 streams, every member among them, against the oracle."""
    _assert_bound(session_in_turns(nam_lib, oracle, families["nano"], KERNEL, seed=938), BOUND_FAST)


def test_wr_bank_set_kernel(nam_lib, files):
    """set_kernel: AUTO and KERNEL_WN_REG, nothing else; the kernel's name for a 64-frame launch, a 256-frame launch and a session."""
    nam = nam_lib
    b = nam.ModelBank(load(nam, files["nano"][:3])).batch(4, BLOCK * 4)
    for k in (nam.KERNEL_WN_REG, nam.KERNEL_AUTO):
        b.set_kernel(k)
        assert b.kernel_name(BLOCK) == KERNEL and b.kernel_name(BLOCK * 4) == KERNEL
    for k in (nam.KERNEL_GENERIC, nam.KERNEL_A1, nam.KERNEL_A1_MFMA, nam.KERNEL_A1_IL):
        with pytest.raises(nam.NamHipError) as e:
            b.set_kernel(k)
        assert e.value.code == nam.ERR_UNSUPPORTED
    assert b.set_persistent(True)
    assert b.kernel_name() == KERNEL
    b.close()


def test_wr_bank_check_tool(nam_lib, files):
    """cpp/tools/bank_check: nam::ModelBank / the bank form of nam::BatchDSP / SetStreamModel through the C++ adapter, on nano
    members (one with the other head_scale); a model of another family is refused."""
    nano = files["nano"]
    check_tool([nano[0], nano[1], nano[NANO_OTHER_SCALE[0]]], refuse=model_path("wavenet_a1_standard"))
