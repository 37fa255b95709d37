"""Model banks on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams each run their own WaveNet
weights, in every launch class of the interleaved-frame kernel family. Two kinds of check:
  * against the CPU oracle of the stream's OWN member, with the project's bounds as they stand (relative _tol(fast_tanh) as in
    test_gpu_breadth.py, and the reference's absolute 5e-5, tools/test/test_a2_fast.cpp:296-298);
  * bit for bit against one-model batches of the members fed the same audio through the same calls — same kernel, same sums,
    no tolerance: what catches a wrong blob stride, a stale head_scale or a prewarm with the wrong member's weights.
Members: the committed standard / lite / feather fixtures and standard-topology models with seeded weights and distinct
head_scale values (tests/bank_models.py)."""
import os
import subprocess

import numpy as np
import pytest

from bank_models import head_scale_of, write_standard
from conftest import ROOT, model_path
from signals import stream_bank

pytestmark = pytest.mark.gpu

BLOCK = 64
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


def _load(nam, paths, fast_tanh=True):
    return [nam.get_dsp(p, fast_tanh=fast_tanh) for p in paths]


def _drive(b, x, mode, hook=None):
    """x [n, T] through batch `b` on device-resident buffers; returns (y [n, T], the kernel the runtime names for the mode).
    session: persistent mode, one command per 64 frames, a flush after the third and at the end;
    bursts : persistent mode, a flush after every command (after three such bursts the launches start as the low-latency kernel);
    blocks : a plain launch per 64 frames;    launch : one plain launch over the whole signal.
    hook(k): called before block k (session mode)."""
    import torch
    n, T = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x[:, None, :])).cuda()
    yd = torch.zeros_like(xd)
    torch.cuda.synchronize()
    nb = T // BLOCK
    if mode in ("session", "bursts"):
        assert b.set_persistent(True)
        for k in range(nb):
            if hook:
                hook(k)
            b.process_device(xd.data_ptr() + k * BLOCK * 4, yd.data_ptr() + k * BLOCK * 4, BLOCK, T)
            if mode == "bursts" or k == 2:
                b.flush()
        b.flush()
        name = b.kernel_name()
    elif mode == "blocks":
        for k in range(nb):
            b.process_device(xd.data_ptr() + k * BLOCK * 4, yd.data_ptr() + k * BLOCK * 4, BLOCK, T)
        name = b.kernel_name(BLOCK)
    else:
        b.process_device(xd.data_ptr(), yd.data_ptr(), T, T)
        name = b.kernel_name(T)
    b.synchronize()
    torch.cuda.synchronize()
    return yd.cpu().numpy()[:, 0, :], name


def _singles(nam, models, member_of, x, mode, il=False, start=0, max_frames=BLOCK):
    """The same audio through one-model batches: for each member a batch of the streams bound to it. Returns y [n, T - start]
    (input from frame `start` on, after Reset with prewarm) and the kernel names seen."""
    y = np.zeros((x.shape[0], x.shape[1] - start), dtype=np.float32)
    names = set()
    for m, model in enumerate(models):
        rows = [s for s in range(x.shape[0]) if member_of[s] == m]
        if not rows:
            continue
        b = model.batch(len(rows), max_frames)
        if il:  # (a lone 64-frame launch of a one-model batch runs nam_a1_mfma_kernel under AUTO; the bank runs the A1_IL family)
            b.set_kernel(nam.KERNEL_A1_IL)
        b.Reset(prewarm=True)
        ym, name = _drive(b, x[rows][:, start:], mode)
        b.close()
        y[rows] = ym
        names.add(name)
    return y, names


def _oracle_errors(oracle, paths, member_of, x, y, streams, fast_tanh=True):
    """worst (relative, absolute) error per member over `streams`"""
    worst = {}
    for s in streams:
        ref = oracle.get_dsp(paths[member_of[s]], fast_tanh=fast_tanh)
        ref.Reset(48000.0, BLOCK)
        r = ref.process_stream(x[s], BLOCK)[0]
        abs_err = float(np.max(np.abs(r - y[s])))
        rel = abs_err / max(1.0, float(np.max(np.abs(r))))
        w = worst.setdefault(member_of[s], [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], rel), max(w[1], abs_err), max(w[2], float(np.max(np.abs(r))))
    for m in sorted(worst):
        print(f"member {m} ({os.path.basename(paths[m])}): worst relative {worst[m][0]:.3e}, absolute {worst[m][1]:.3e}, |y|max {worst[m][2]:.3f}")
    return worst


def _assert_bounds(worst, fast_tanh=True):
    for m, (rel, abs_err, _) in worst.items():
        assert rel <= _tol(fast_tanh), (m, rel)
        assert abs_err <= (ABS_BOUND if fast_tanh else 1e-4), (m, abs_err)


def test_bank_session_every_stream_against_its_members_oracle(nam_lib, oracle, member_paths):
    """256 streams over 8 members (stream s -> member s % 8) in persistent mode: six 64-frame commands, a flush after the third
    (the shape of test_gpu_breadth.py::test_bench_shapes_every_stream_in_persistent_mode). EVERY stream against the oracle
    of its member. The sharp members are the committed fixtures (|y| ~ 0.1 - 1); the seeded ones (|y|max 0.02 - 0.05) sit far
    inside the absolute bound — for them the bit-for-bit tests below are the sharp check."""
    nam = nam_lib
    n = 256
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * 6, seed=902)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    assert [b.stream_model(s) for s in (0, 1, 7, 255)] == [0, 1, 7, 7]
    b.Reset(prewarm=True)
    y, name = _drive(b, x, "session")
    b.close()
    assert name == "nam_a1_q_kernel"
    assert np.isfinite(y).all()
    worst = _oracle_errors(oracle, member_paths, member_of, x, y, range(n))
    assert sorted(worst) == list(range(8))
    _assert_bounds(worst)


@pytest.mark.parametrize("mode,kernel", [("session", "nam_a1_q_kernel"), ("bursts", "nam_a1_p4_kernel"), ("blocks", "nam_a1_p2_kernel"),
                                         ("launch", "nam_a1_q_kernel")])
def test_bank_equals_one_model_batches_bit_for_bit(nam_lib, member_paths, mode, kernel):
    """All 256 streams, np.array_equal, in the family's launch classes: the session (nam_a1_q_kernel), a session whose caller
    flushes after every buffer (its launches become nam_a1_p4_kernel after three bursts), a plain launch per buffer
    (nam_a1_p2_kernel) and one plain launch over eight buffers (nam_a1_q_kernel again, outside a session). The kernel is the
    runtime's choice: read from kernel_name and asserted for the bank AND for the one-model batches."""
    nam = nam_lib
    n = 256
    nb = 8 if mode in ("bursts", "launch") else 6
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * nb, seed=903)
    max_frames = BLOCK * nb if mode == "launch" else BLOCK
    b = bank.batch(n, max_frames, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = _drive(b, x, mode)
    b.close()
    assert name == kernel
    want, names = _singles(nam, models, member_of, x, mode, il=(mode == "blocks"), max_frames=max_frames)
    assert names == {kernel}
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    bad = [s for s in range(n) if not np.array_equal(y[s], want[s])]
    assert not bad, (mode, len(bad), bad[:8])
    # the members do differ: the same input through two members gives different output (else the test above shows nothing)
    xs = np.repeat(x[:1], 8, axis=0)
    b = bank.batch(8, max_frames, stream_model=list(range(8)))
    b.Reset(prewarm=True)
    y8, _ = _drive(b, xs, mode)
    b.close()
    for m in range(1, 8):
        assert not np.array_equal(y8[0], y8[m])


def test_bank_tanh_instantiation_bit_for_bit(nam_lib, oracle, member_paths):
    """fast_tanh=False: the ACT_TANH instantiations, 32 streams, session; bit for bit and four streams against the oracle."""
    nam = nam_lib
    n = 32
    models = _load(nam, member_paths, fast_tanh=False)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * 6, seed=904)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = _drive(b, x, "session")
    b.close()
    assert name == "nam_a1_q_kernel"
    want, names = _singles(nam, models, member_of, x, "session")
    assert names == {"nam_a1_q_kernel"}
    assert all(np.array_equal(y[s], want[s]) for s in range(n))
    _assert_bounds(_oracle_errors(oracle, member_paths, member_of, x, y, (0, 9, 18, 31), fast_tanh=False), fast_tanh=False)


def _feed_tickets(batch, x, depth):
    nb = x.shape[-1] // BLOCK
    ys, tickets = [], []
    for k in range(nb):
        if len(tickets) == depth:
            ys.append(batch.wait(tickets.pop(0)))
        tickets.append(batch.submit(x[:, k * BLOCK:(k + 1) * BLOCK]))
    while tickets:
        ys.append(batch.wait(tickets.pop(0)))
    return np.concatenate(ys, axis=2)[:, 0, :]


@pytest.mark.parametrize("path", ["blocking", "tickets"])
def test_bank_host_paths(nam_lib, oracle, member_paths, path):
    """Host buffers on a 64-stream bank batch in persistent mode: blocking process calls of 64 frames, 20 back to back (the
    lingering launch serves them), and tickets with 16 in flight. Bit for bit against one-model batches driven the same way;
    five streams against the oracle."""
    nam = nam_lib
    n, nb = 64, (20 if path == "blocking" else 32)
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [(s * 3) % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * nb, seed=905)

    def run(b, xs):
        assert b.set_persistent(True)
        b.Reset(prewarm=True)
        if path == "blocking":
            y = np.concatenate([b.process(xs[:, k * BLOCK:(k + 1) * BLOCK]) for k in range(nb)], axis=2)[:, 0, :]
        else:
            y = _feed_tickets(b, xs, 16)
        b.close()
        return y

    y = run(bank.batch(n, BLOCK, stream_model=member_of), x)
    assert np.isfinite(y).all()
    for m, model in enumerate(models):
        rows = [s for s in range(n) if member_of[s] == m]
        want = run(model.batch(len(rows), BLOCK), x[rows])
        for i, s in enumerate(rows):
            assert np.array_equal(y[s], want[i]), (path, m, s)
    _assert_bounds(_oracle_errors(oracle, member_paths, member_of, x, y, (0, 13, 27, 42, 63)))


def test_bank_rebinding_in_a_running_session(nam_lib, member_paths):
    """After three commands of a session, streams {1, 17, 200} move to another member. From then on they equal a freshly
    reset (prewarmed) one-model batch of the new member fed the remaining input; every other stream equals the run without
    the swap; both bit for bit. An out-of-range member or stream fails and changes nothing."""
    nam = nam_lib
    n, nb = 256, 6
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    moved, new = [1, 17, 200], 6
    assert all(member_of[s] != new for s in moved)
    x = stream_bank(n, BLOCK * nb, seed=906)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    plain, _ = _drive(b, x, "session")
    b.close()

    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)

    def hook(k):
        if k == 3:
            for bad_member, bad_stream in ((8, 5), (-1, 5), (2, n), (2, -1)):
                with pytest.raises(nam.NamHipError) as e:
                    b.set_stream_model(bad_member, [5, bad_stream])
                assert e.value.code == nam.ERR_INVALID_ARGUMENT
            assert [b.stream_model(s) for s in (5, 1, 17, 200)] == [5, 1, 1, 0]
            b.set_stream_model(new, moved)
            assert [b.stream_model(s) for s in moved] == [new] * 3 and b.stream_model(2) == 2
            b.set_stream_model(new, moved)  # already there: a no-op (the streams are NOT reset again)

    y, name = _drive(b, x, "session", hook=hook)
    b.close()
    assert name == "nam_a1_q_kernel"
    for s in range(n):
        if s not in moved:
            assert np.array_equal(y[s], plain[s]), s
    for s in moved:
        assert np.array_equal(y[s, :3 * BLOCK], plain[s, :3 * BLOCK]), s
    fresh = models[new].batch(len(moved), BLOCK)
    fresh.Reset(prewarm=True)
    want, _ = _drive(fresh, np.ascontiguousarray(x[moved][:, 3 * BLOCK:]), "session")
    fresh.close()
    for i, s in enumerate(moved):
        assert np.array_equal(y[s, 3 * BLOCK:], want[i]), s
        assert not np.array_equal(y[s, 3 * BLOCK:], plain[s, 3 * BLOCK:])
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


def test_bank_session_in_turns(nam_lib, oracle, member_paths):
    """600 streams over 8 members: more workgroups than CUs, the session's workgroups take turns. Every stream finite; streams
    s and s + 8 (same member) are fed identical input in every other group of eight and must produce identical output; one
    stream of every group of eight — 75 streams, the member rotating with the group — against the oracle (a fixed cap: the
    256-stream test above checks every stream, the pairwise equality covers the rest)."""
    nam = nam_lib
    n, nb = 600, 6
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * nb, seed=907)
    pairs = [s for s in range(n - 8) if (s // 8) % 2 == 0]
    for s in pairs:
        x[s + 8] = x[s]
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = _drive(b, x, "session")
    b.close()
    assert name == "nam_a1_q_kernel"
    assert np.isfinite(y).all()
    for s in pairs:
        assert np.array_equal(y[s], y[s + 8]), s
    picks = [s for s in range(n) if s % 8 == (s // 8) % 8]
    assert len(picks) == 75
    _assert_bounds(_oracle_errors(oracle, member_paths, member_of, x, y, picks))


def test_bank_check_tool(nam_lib):
    """cpp/tools/bank_check: nam::ModelBank / the bank form of nam::BatchDSP / SetStreamModel through the C++ adapter."""
    tool = os.path.join(ROOT, "cpp", "tools", "bank_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/bank_check"
    r = subprocess.run([tool] + [model_path(n) for n in FIXTURES] + ["--refuse", model_path("lstm")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAIL" not in r.stdout, r.stdout
