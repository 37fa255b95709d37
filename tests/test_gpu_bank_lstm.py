"""Model banks of the LSTM family on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams each run
their own LSTM weights AND start from their own h0 / c0, on nam_lstm_row_kernel (hidden <= 4: four streams per wavefront, every
16-lane row its own member) and nam_lstm_wide_kernel (5 .. 32 units: one stream per wavefront). Two kinds of check, as in
tests/test_gpu_bank_a2.py:
  * against the CPU oracle of the stream's OWN member, with the bound of test_gpu_parity.py::test_lstm_kernels_match_oracle:
    5e-5 with fast tanh, 1e-4 without, times max(1, |ref|max);
  * bit for bit against one-model batches of the members fed the same audio through the same calls — same kernel, same sums, no
    tolerance: what catches a wrong blob stride, a head computed with another row's member, a stale initial state.
Members: a shipped fixture as member 0 plus seeded models of its shape (tests/bank_models.py).

Not here, and why:
  * a partial reset through a stream map: the Python mirror exposes no such call (Reset is whole-batch). The same launch form —
    a stream map over a bank batch, members looked up by STREAM — runs in the rebinding test (its prewarm of the moved streams).
  * sessions whose workgroups take turns: the LSTM kernels have none (api_session.cpp: persist_kind answers PERSIST_NONE beyond
    what the chip holds at once — 8 row-kernel workgroups per CU — and a few hundred streams are far below that)."""
import numpy as np
import pytest

from bank_harness import BLOCK, Family, bit_for_bit, check_tool, drive, host_paths, load, rebinding, singles
from bank_models import write_lstm
from conftest import model_path

pytestmark = pytest.mark.gpu

RAGGED = BLOCK * 3 + 11
ROW, WIDE = "nam_lstm_row_kernel", "nam_lstm_wide_kernel"
# name: fixture (member 0), its shape for the generator, the kernel, streams (row: a ragged last workgroup and rows of one
# wavefront on different members; wide: one workgroup per stream)
SHAPES = {
    "row_1x3": ("lstm", dict(num_layers=1, input_size=1, hidden=3, out_channels=1), ROW, 7),
    "row_2x4": ("synth_lstm_h4x2", dict(num_layers=2, input_size=1, hidden=4, out_channels=1), ROW, 7),
    "wide_2x18": ("synth_lstm_h18x2", dict(num_layers=2, input_size=1, hidden=18, out_channels=1), WIDE, 5),
    "wide_2x24io": ("synth_lstm_h24x2io", dict(num_layers=2, input_size=2, hidden=24, out_channels=2), WIDE, 5),
}


def _tol(fast_tanh):
    return 5e-5 if fast_tanh else 1e-4  # test_gpu_parity.py


@pytest.fixture(scope="module")
def member_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("lstm_bank_members")
    out = {}
    for i, (name, (fixture, kw, _, _)) in enumerate(SHAPES.items()):
        out[name] = [model_path(fixture)]
        for seed in (700 + 10 * i, 701 + 10 * i):
            p = str(d / f"{name}_{seed}.nam")
            write_lstm(p, seed, **kw)
            out[name].append(p)
    return out


def _signal(n, ic, T, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, ic, T)).astype(np.float32)


def _family(member_paths, shape):
    ic = SHAPES[shape][1]["input_size"]
    return Family(member_paths[shape], lambda n, T, seed: _signal(n, ic, T, seed))


@pytest.mark.parametrize("fast_tanh", [True, False])
@pytest.mark.parametrize("mode", ["launch", "session"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lstm_bank_every_stream_against_its_members_oracle(nam_lib, oracle, member_paths, shape, mode, fast_tanh):
    """stream s -> member s % 3, after Reset with prewarm: 64 * 3 + 11 frames in ONE launch, and six session commands with a flush
    after the third. EVERY stream against the oracle of its member."""
    nam = nam_lib
    _, kw, kernel, n = SHAPES[shape]
    paths = member_paths[shape]
    bank = nam.ModelBank(load(nam, paths, fast_tanh))
    member_of = [s % 3 for s in range(n)]
    T = RAGGED if mode == "launch" else BLOCK * 6
    max_frames = T if mode == "launch" else BLOCK
    x = _signal(n, kw["input_size"], T, seed=931)
    b = bank.batch(n, max_frames, stream_model=member_of)
    assert [b.stream_model(s) for s in range(n)] == member_of
    b.Reset(prewarm=True)
    y, name = drive(b, x, mode)
    b.close()
    assert name == kernel
    assert np.isfinite(y).all()
    for s in range(n):
        ref = oracle.get_dsp(paths[member_of[s]], fast_tanh=fast_tanh)
        ref.Reset(48000.0, max_frames)  # (prewarm: whole max_frames-sized buffers of silence, as the batch's)
        r = ref.process_stream(x[s], max_frames)
        err, scale = float(np.max(np.abs(r - y[s]))), max(1.0, float(np.max(np.abs(r))))
        print(f"{shape} {mode} fast_tanh={fast_tanh} stream {s} member {member_of[s]}: max |error| {err:.3e}, |ref|max {scale:.3f}")
        assert err <= _tol(fast_tanh) * scale, (shape, mode, s)


@pytest.mark.parametrize("mode,T", [("session", BLOCK * 6), ("blocks", BLOCK * 6), ("launch", RAGGED)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lstm_bank_equals_one_model_batches_bit_for_bit(nam_lib, member_paths, shape, mode, T):
    """np.array_equal, every stream, in the launch classes: the session, a plain launch per buffer, one ragged launch. The kernel
    is the runtime's choice: read from kernel_name and asserted for the bank AND for the one-model batches. And the members do
    differ: identical input through the three members gives three different outputs."""
    _, _, kernel, n = SHAPES[shape]
    bit_for_bit(nam_lib, _family(member_paths, shape), mode, kernel, T, seed=932, n=n)


@pytest.mark.parametrize("shape", ["row_1x3", "wide_2x18"])
def test_lstm_bank_initial_state_per_member(nam_lib, tmp_path, shape):
    """No prewarm (Reset(prewarm=False) on a fresh batch): the first buffer of a stream shows its member's h0 / c0. Members 0 and 1
    have EQUAL weights and different h0 / c0 (the generator's state_seed), member 2 is another seed. Every stream equals its
    member's one-model batch bit for bit, and members 0 and 1 differ on identical input."""
    nam = nam_lib
    _, kw, kernel, _ = SHAPES[shape]
    paths = [str(tmp_path / f"{shape}_{i}.nam") for i in range(3)]
    write_lstm(paths[0], 760, **kw)
    write_lstm(paths[1], 760, state_seed=1, **kw)
    write_lstm(paths[2], 761, **kw)
    models = load(nam, paths)
    bank = nam.ModelBank(models)
    n = 6
    member_of = [0, 1, 2, 1, 0, 2]
    x = np.repeat(_signal(1, kw["input_size"], BLOCK, seed=933), n, axis=0)  # identical input everywhere
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=False)
    y, name = drive(b, x, "blocks")
    b.close()
    assert name == kernel
    want, _ = singles(nam, models, member_of, x, "blocks", prewarm=False)
    for s in range(n):
        assert np.array_equal(y[s], want[s]), s
    assert np.array_equal(y[0], y[4]) and np.array_equal(y[1], y[3])
    assert not np.array_equal(y[0], y[1])  # h0 / c0 only
    assert not np.array_equal(y[0], y[2])


@pytest.mark.parametrize("shape", ["row_1x3", "wide_2x18"])
def test_lstm_bank_rebinding_in_a_running_session(nam_lib, member_paths, shape):
    """After three commands of a session, streams {0, 3, 6} move to another member — on the row kernel 0 and 3 share a wavefront
    with streams 1 and 2, 6 sits in the next one. An LSTM's Reset clears nothing, so the rebinding itself must give the moved
    streams the NEW member's h0 / c0 before their prewarm: from then on they equal a freshly created, prewarmed one-model batch of
    the new member fed the remaining input; every other stream (the row neighbours too) equals the run without the move; both
    bit for bit. An out-of-range member or stream fails and changes nothing."""
    rebinding(nam_lib, _family(member_paths, shape), SHAPES[shape][2], n=10, moved=[0, 3, 6], new=2, probe=1, seed=934)


@pytest.mark.parametrize("path", ["blocking", "tickets"])
@pytest.mark.parametrize("shape", ["row_1x3", "wide_2x18"])
def test_lstm_bank_host_paths(nam_lib, member_paths, shape, path):
    """Host buffers on a 16-stream bank batch in persistent mode: twenty blocking 64-frame process calls back to back, and tickets
    with eight in flight. Bit for bit against one-model batches driven the same way."""
    host_paths(nam_lib, _family(member_paths, shape), path, n=16, nb=20, step=2, seed=935, depth=8, kernel=SHAPES[shape][2])


@pytest.mark.parametrize("shape", ["row_1x3", "wide_2x18"])
def test_lstm_bank_set_kernel(nam_lib, member_paths, shape):
    """AUTO only: the other LSTM kernels share one wavefront's weights among their streams, the WaveNet kernels run no LSTM."""
    nam = nam_lib
    kernel = SHAPES[shape][2]
    b = nam.ModelBank(load(nam, member_paths[shape])).batch(4, BLOCK)
    b.set_kernel(nam.KERNEL_AUTO)
    for k in (nam.KERNEL_GENERIC, nam.KERNEL_A1_MFMA, nam.KERNEL_A1, nam.KERNEL_A1_IL, nam.KERNEL_WN_REG):
        with pytest.raises(nam.NamHipError) as e:
            b.set_kernel(k)
        assert e.value.code == nam.ERR_UNSUPPORTED
        assert ROW in str(e.value) and WIDE in str(e.value), str(e.value)
    assert b.kernel_name(BLOCK) == kernel and b.kernel_name(BLOCK * 4) == kernel and b.kernel_name() == kernel
    b.close()


def test_lstm_bank_check_tool(nam_lib, tmp_path):
    """cpp/tools/bank_check: nam::ModelBank / the bank form of nam::BatchDSP / SetStreamModel through the C++ adapter, on LSTM
    members; a model of another family is refused."""
    a, b = str(tmp_path / "lstm_seed_a.nam"), str(tmp_path / "lstm_seed_b.nam")
    write_lstm(a, 771)
    write_lstm(b, 772)
    check_tool([model_path("lstm"), a, b], refuse=model_path("wavenet_a1_standard"))
