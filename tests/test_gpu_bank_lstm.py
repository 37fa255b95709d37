"""Model banks of the LSTM family on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams each run
their own LSTM weights AND start from their own h0 / c0, on nam_lstm_row_kernel (hidden <= 4: four streams per wavefront, every
16-lane row its own member) and nam_lstm_wide_kernel (5 .. 32 units: one stream per wavefront). Two kinds of check, as in
tests/test_gpu_bank_a2.py:
  * against the CPU oracle of the stream's OWN member, with the bound of test_gpu_parity.py::test_lstm_kernels_match_oracle:
    5e-5 with fast tanh, 1e-4 without, times max(1, |ref|max);
  * bit for bit against one-model batches of the members fed the same audio through the same calls — same kernel, same sums, no
    tolerance: what catches a wrong blob stride, a head computed with another row's member, a stale initial state.
Members: a shipped fixture as member 0 plus seeded models of its shape (tests/bank_models_lstm.py).

Not here, and why:
  * a partial reset through a stream map: the Python mirror exposes no such call (Reset is whole-batch). The same launch form —
    a stream map over a bank batch, members looked up by STREAM — runs in the rebinding test (its prewarm of the moved streams).
  * sessions whose workgroups take turns: the LSTM kernels have none (api_session.cpp: persist_kind answers PERSIST_NONE beyond
    what the chip holds at once — 8 row-kernel workgroups per CU — and a few hundred streams are far below that)."""
import os
import subprocess

import numpy as np
import pytest

from bank_models_lstm import write_lstm
from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu

BLOCK = 64
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


def _load(nam, paths, fast_tanh=True):
    return [nam.get_dsp(p, fast_tanh=fast_tanh) for p in paths]


def _signal(n, ic, T, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, ic, T)).astype(np.float32)


def _drive(b, x, mode, hook=None):
    """x [n, ic, T] through batch `b` on device-resident buffers; returns (y [n, oc, T], the kernel the runtime names for the mode).
    session: persistent mode, one command per 64 frames, a flush after the third and at the end;
    blocks : a plain launch per 64 frames (T a multiple of 64);    launch : one plain launch over the whole signal (any T).
    hook(k): called before block k (session mode)."""
    import torch
    n, ic, T = x.shape
    oc = b.model.NumOutputChannels()
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.zeros((n, oc, T), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nb = T // BLOCK
    if mode == "session":
        assert T % BLOCK == 0
        assert b.set_persistent(True)
        for k in range(nb):
            if hook:
                hook(k)
            b.process_device(xd.data_ptr() + k * BLOCK * 4, yd.data_ptr() + k * BLOCK * 4, BLOCK, T)
            if k == 2:
                b.flush()
        b.flush()
        name = b.kernel_name()
    elif mode == "blocks":
        assert T % BLOCK == 0
        for k in range(nb):
            b.process_device(xd.data_ptr() + k * BLOCK * 4, yd.data_ptr() + k * BLOCK * 4, BLOCK, T)
        name = b.kernel_name(BLOCK)
    else:
        b.process_device(xd.data_ptr(), yd.data_ptr(), T, T)
        name = b.kernel_name(T)
    b.synchronize()
    torch.cuda.synchronize()
    return yd.cpu().numpy(), name


def _singles(models, member_of, x, mode, max_frames=BLOCK, prewarm=True):
    """The same audio through one-model batches under AUTO: for each member a batch of the streams bound to it. Returns y and the
    kernel names seen."""
    y, names = None, set()
    for m, model in enumerate(models):
        rows = [s for s in range(x.shape[0]) if member_of[s] == m]
        if not rows:
            continue
        b = model.batch(len(rows), max_frames)
        b.Reset(prewarm=prewarm)
        ym, name = _drive(b, np.ascontiguousarray(x[rows]), mode)
        b.close()
        if y is None:
            y = np.zeros((x.shape[0],) + ym.shape[1:], dtype=np.float32)
        y[rows] = ym
        names.add(name)
    return y, names


@pytest.mark.parametrize("fast_tanh", [True, False])
@pytest.mark.parametrize("mode", ["launch", "session"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lstm_bank_every_stream_against_its_members_oracle(nam_lib, oracle, member_paths, shape, mode, fast_tanh):
    """stream s -> member s % 3, after Reset with prewarm: 64 * 3 + 11 frames in ONE launch, and six session commands with a flush
    after the third. EVERY stream against the oracle of its member."""
    nam = nam_lib
    _, kw, kernel, n = SHAPES[shape]
    paths = member_paths[shape]
    bank = nam.ModelBank(_load(nam, paths, fast_tanh))
    member_of = [s % 3 for s in range(n)]
    T = RAGGED if mode == "launch" else BLOCK * 6
    max_frames = T if mode == "launch" else BLOCK
    x = _signal(n, kw["input_size"], T, seed=931)
    b = bank.batch(n, max_frames, stream_model=member_of)
    assert [b.stream_model(s) for s in range(n)] == member_of
    b.Reset(prewarm=True)
    y, name = _drive(b, x, mode)
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
    nam = nam_lib
    _, kw, kernel, n = SHAPES[shape]
    models = _load(nam, member_paths[shape])
    bank = nam.ModelBank(models)
    member_of = [s % 3 for s in range(n)]
    x = _signal(n, kw["input_size"], T, seed=932)
    max_frames = T if mode == "launch" else BLOCK
    b = bank.batch(n, max_frames, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = _drive(b, x, mode)
    b.close()
    assert name == kernel
    want, names = _singles(models, member_of, x, mode, max_frames=max_frames)
    assert names == {kernel}
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    bad = [s for s in range(n) if not np.array_equal(y[s], want[s])]
    assert not bad, (shape, mode, bad)
    xs = np.repeat(x[:1], 3, axis=0)
    b = bank.batch(3, max_frames, stream_model=[0, 1, 2])
    b.Reset(prewarm=True)
    y3, _ = _drive(b, xs, mode)
    b.close()
    for m, m2 in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(y3[m], y3[m2]), (m, m2)


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
    models = _load(nam, paths)
    bank = nam.ModelBank(models)
    n = 6
    member_of = [0, 1, 2, 1, 0, 2]
    x = np.repeat(_signal(1, kw["input_size"], BLOCK, seed=933), n, axis=0)  # identical input everywhere
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=False)
    y, name = _drive(b, x, "blocks")
    b.close()
    assert name == kernel
    want, _ = _singles(models, member_of, x, "blocks", prewarm=False)
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
    nam = nam_lib
    _, kw, kernel, _ = SHAPES[shape]
    n, nb = 10, 6
    models = _load(nam, member_paths[shape])
    bank = nam.ModelBank(models)
    member_of = [s % 3 for s in range(n)]
    moved, new = [0, 3, 6], 2
    assert all(member_of[s] != new for s in moved)
    x = _signal(n, kw["input_size"], BLOCK * nb, seed=934)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    plain, _ = _drive(b, x, "session")
    b.close()

    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)

    def hook(k):
        if k == 3:
            for bad_member, bad_stream in ((3, 5), (-1, 5), (1, n), (1, -1)):
                with pytest.raises(nam.NamHipError) as e:
                    b.set_stream_model(bad_member, [5, bad_stream])
                assert e.value.code == nam.ERR_INVALID_ARGUMENT
            assert [b.stream_model(s) for s in (5, 0, 3, 6)] == [2, 0, 0, 0]
            b.set_stream_model(new, moved)
            assert [b.stream_model(s) for s in moved] == [new] * 3 and b.stream_model(1) == 1
            b.set_stream_model(new, moved)  # already there: a no-op (the streams are NOT reset again)

    y, name = _drive(b, x, "session", hook=hook)
    b.close()
    assert name == kernel
    for s in range(n):
        if s not in moved:
            assert np.array_equal(y[s], plain[s]), s
    for s in moved:
        assert np.array_equal(y[s, :, :3 * BLOCK], plain[s, :, :3 * BLOCK]), s
    fresh = models[new].batch(len(moved), BLOCK)
    fresh.Reset(prewarm=True)
    want, _ = _drive(fresh, np.ascontiguousarray(x[moved][:, :, 3 * BLOCK:]), "session")
    fresh.close()
    for i, s in enumerate(moved):
        assert np.array_equal(y[s, :, 3 * BLOCK:], want[i]), s
        assert not np.array_equal(y[s, :, 3 * BLOCK:], plain[s, :, 3 * BLOCK:])


def _feed_tickets(batch, x, depth):
    nb = x.shape[-1] // BLOCK
    ys, tickets = [], []
    for k in range(nb):
        if len(tickets) == depth:
            ys.append(batch.wait(tickets.pop(0)))
        tickets.append(batch.submit(x[:, :, k * BLOCK:(k + 1) * BLOCK]))
    while tickets:
        ys.append(batch.wait(tickets.pop(0)))
    return np.concatenate(ys, axis=2)


@pytest.mark.parametrize("path", ["blocking", "tickets"])
@pytest.mark.parametrize("shape", ["row_1x3", "wide_2x18"])
def test_lstm_bank_host_paths(nam_lib, member_paths, shape, path):
    """Host buffers on a 16-stream bank batch in persistent mode: twenty blocking 64-frame process calls back to back, and tickets
    with eight in flight. Bit for bit against one-model batches driven the same way."""
    nam = nam_lib
    _, kw, kernel, _ = SHAPES[shape]
    n, nb = 16, 20
    models = _load(nam, member_paths[shape])
    bank = nam.ModelBank(models)
    member_of = [(s * 2) % 3 for s in range(n)]
    x = _signal(n, kw["input_size"], BLOCK * nb, seed=935)

    def run(b, xs):
        assert b.set_persistent(True)
        assert b.kernel_name() == kernel
        b.Reset(prewarm=True)
        if path == "blocking":
            y = np.concatenate([b.process(xs[:, :, k * BLOCK:(k + 1) * BLOCK]) for k in range(nb)], axis=2)
        else:
            y = _feed_tickets(b, xs, 8)
        b.close()
        return y

    y = run(bank.batch(n, BLOCK, stream_model=member_of), x)
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    assert sorted(set(member_of)) == [0, 1, 2]
    for m, model in enumerate(models):
        rows = [s for s in range(n) if member_of[s] == m]
        want = run(model.batch(len(rows), BLOCK), np.ascontiguousarray(x[rows]))
        for i, s in enumerate(rows):
            assert np.array_equal(y[s], want[i]), (path, m, s)


@pytest.mark.parametrize("shape", ["row_1x3", "wide_2x18"])
def test_lstm_bank_set_kernel(nam_lib, member_paths, shape):
    """AUTO only: the other LSTM kernels share one wavefront's weights among their streams, the WaveNet kernels run no LSTM."""
    nam = nam_lib
    kernel = SHAPES[shape][2]
    b = nam.ModelBank(_load(nam, member_paths[shape])).batch(4, BLOCK)
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
    tool = os.path.join(ROOT, "cpp", "tools", "bank_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/bank_check"
    a, b = str(tmp_path / "lstm_seed_a.nam"), str(tmp_path / "lstm_seed_b.nam")
    write_lstm(a, 771)
    write_lstm(b, 772)
    r = subprocess.run([tool, model_path("lstm"), a, b, "--refuse", model_path("wavenet_a1_standard")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAIL" not in r.stdout, r.stdout
