"""Model banks of the A2 family on the GPU (include/nam_hip.h: nam_hip_batch_create_bank): one batch whose streams each run
their own A2-topology weights on nam_kq_kernel (sessions, launches of several buffers) and nam_kt_mfma_kernel (a lone buffer).
Two kinds of check, as in tests/test_gpu_bank.py for the A1 family:
  * against the CPU oracle of the stream's OWN member: relative 5e-5 * max(1, |ref|max), the bound test_gpu_breadth.py uses for
    this kernel, and for the A2.nam member also the reference's absolute 5e-5 (tools/test/test_a2_fast.cpp:296-298);
  * bit for bit against one-model batches of the members fed the same audio through the same calls — same kernel, same sums, no
    tolerance: what catches a wrong blob stride, a stale head_scale / slope or a prewarm with the wrong member's weights.
Members: tests/golden/models/A2.nam (a container: it stands for A2-Full) and A2-topology models with seeded weights, distinct
head_scale values and distinct LeakyReLU slopes (tests/bank_models_a2.py)."""
import os
import subprocess

import numpy as np
import pytest

from bank_models_a2 import head_scale_of, slope_of, write_a2
from conftest import ROOT, model_path
from signals import stream_bank

pytestmark = pytest.mark.gpu

BLOCK = 64
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


def _load(nam, paths, fast_tanh=True):
    return [nam.get_dsp(p, fast_tanh=fast_tanh) for p in paths]


def _drive(b, x, mode, hook=None):
    """x [n, T] through batch `b` on device-resident buffers; returns (y [n, T], the kernel the runtime names for the mode).
    session: persistent mode, one command per 64 frames, a flush after the third and at the end;
    blocks : a plain launch per 64 frames (T a multiple of 64);    launch : one plain launch over the whole signal (any T).
    hook(k): called before block k (session mode)."""
    import torch
    n, T = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x[:, None, :])).cuda()
    yd = torch.zeros_like(xd)
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
    return yd.cpu().numpy()[:, 0, :], name


def _singles(models, member_of, x, mode, max_frames=BLOCK):
    """The same audio through one-model batches under AUTO: for each member a batch of the streams bound to it. Returns y [n, T]
    (after Reset with prewarm) and the kernel names seen."""
    y = np.zeros(x.shape, dtype=np.float32)
    names = set()
    for m, model in enumerate(models):
        rows = [s for s in range(x.shape[0]) if member_of[s] == m]
        if not rows:
            continue
        b = model.batch(len(rows), max_frames)
        b.Reset(prewarm=True)
        ym, name = _drive(b, np.ascontiguousarray(x[rows]), mode)
        b.close()
        y[rows] = ym
        names.add(name)
    return y, names


def _oracle_errors(oracle, paths, member_of, x, y, streams, fast_tanh=True):
    """worst (relative, absolute, |ref|max) per member over `streams`, printed"""
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


def _assert_bounds(worst, paths):
    for m, (rel, abs_err, _) in worst.items():
        assert rel <= REL_BOUND, (m, rel)
        if os.path.basename(paths[m]) == "A2.nam":
            assert abs_err <= ABS_BOUND, (m, abs_err)


def test_a2_bank_session_every_stream_against_its_members_oracle(nam_lib, oracle, member_paths):
    """256 streams over 8 members (stream s -> member s % 8) in persistent mode: six 64-frame commands, a flush after the third,
    after Reset with prewarm. EVERY stream against the oracle of its member."""
    nam = nam_lib
    n = 256
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * 6, seed=912)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    assert [b.stream_model(s) for s in (0, 1, 7, 255)] == [0, 1, 7, 7]
    b.Reset(prewarm=True)
    y, name = _drive(b, x, "session")
    b.close()
    assert name == "nam_kq_kernel"
    assert np.isfinite(y).all()
    worst = _oracle_errors(oracle, member_paths, member_of, x, y, range(n))
    assert sorted(worst) == list(range(8))
    _assert_bounds(worst, member_paths)


def _bit_for_bit(nam, member_paths, mode, kernel, T, seed, n=256):
    """bank against one-model batches, all streams; returns the bank's output. Also: the members differ on identical input."""
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, T, seed=seed)
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
    assert not bad, (mode, len(bad), bad[:8])
    # the members do differ: the same input through two members gives different output (a bank that ran member 0 for everyone
    # would have failed above already — this shows that the comparison above could tell)
    xs = np.repeat(x[:1], 8, axis=0)
    b = bank.batch(8, max_frames, stream_model=list(range(8)))
    b.Reset(prewarm=True)
    y8, _ = _drive(b, xs, mode)
    b.close()
    for m in range(8):
        for m2 in range(m + 1, 8):
            assert not np.array_equal(y8[m], y8[m2]), (m, m2)
    return x, y, member_of, models


@pytest.mark.parametrize("mode,kernel,T", [("session", "nam_kq_kernel", BLOCK * 6), ("blocks", "nam_kt_mfma_kernel", BLOCK * 6),
                                           ("launch", "nam_kq_kernel", RAGGED)])
def test_a2_bank_equals_one_model_batches_bit_for_bit(nam_lib, member_paths, mode, kernel, T):
    """All 256 streams, np.array_equal, in the family's launch classes: the session (nam_kq_kernel), a plain launch per buffer
    (nam_kt_mfma_kernel) and one plain launch over nine buffers and a ragged tail of 21 frames (nam_kq_kernel outside a session).
    The kernel is the runtime's choice: read from kernel_name and asserted for the bank AND for the one-model batches."""
    _bit_for_bit(nam_lib, member_paths, mode, kernel, T, seed=913)


def test_a2_bank_without_the_pipeline(nam_lib, member_paths, monkeypatch):
    """NAM_HIP_MAX_STAGES=1: nam_kt_mfma_kernel everywhere (a launch per buffer and one launch over a ragged length; the topology
    has no session then). Bit for bit against one-model batches, and the ragged launch within 1e-5 of the pipeline's output (the
    figure test_gpu_breadth.py::test_a2_pipeline_kernel uses for the two kernels)."""
    nam = nam_lib
    monkeypatch.setenv("NAM_HIP_MAX_STAGES", "1")
    _bit_for_bit(nam, member_paths, "blocks", "nam_kt_mfma_kernel", BLOCK * 6, seed=914, n=64)
    x, y_kt, member_of, models = _bit_for_bit(nam, member_paths, "launch", "nam_kt_mfma_kernel", RAGGED, seed=915, n=64)
    b = nam.ModelBank(models).batch(4, BLOCK)
    assert not b.set_persistent(True)
    b.close()
    monkeypatch.setenv("NAM_HIP_MAX_STAGES", "0")  # (no cap)
    b = nam.ModelBank(models).batch(64, RAGGED, stream_model=member_of)
    b.Reset(prewarm=True)
    y_kq, name = _drive(b, x, "launch")
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
    models = _load(nam, paths)
    bank = nam.ModelBank(models)
    n = 12
    member_of = [s % 3 for s in range(n)]
    x = np.repeat(stream_bank(n // 3, BLOCK * 6, seed=916), 3, axis=0)  # streams 3 i, 3 i + 1, 3 i + 2: the same input
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = _drive(b, x, mode)
    b.close()
    assert name == ("nam_kq_kernel" if mode == "session" else "nam_kt_mfma_kernel")
    want, _ = _singles(models, member_of, x, mode)
    for s in range(n):
        assert np.array_equal(y[s], want[s]), s
    for i in range(0, n, 3):
        assert not np.array_equal(y[i], y[i + 1])  # slope only
        assert not np.array_equal(y[i], y[i + 2])  # head_scale only
        # head_scale is a factor of the output and of nothing else
        assert np.allclose(y[i + 2], y[i] * np.float32(0.07 / 0.05), rtol=1e-5, atol=1e-7)


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
def test_a2_bank_host_paths(nam_lib, member_paths, path):
    """Host buffers on a 64-stream bank batch in persistent mode: blocking process calls of 64 frames, 20 back to back, and
    tickets with 8 in flight (nam_kq_kernel publishes every command). Bit for bit against one-model batches driven the same way."""
    nam = nam_lib
    n, nb = 64, (20 if path == "blocking" else 32)
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [(s * 3) % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * nb, seed=917)

    def run(b, xs):
        assert b.set_persistent(True)
        assert b.kernel_name() == "nam_kq_kernel"
        b.Reset(prewarm=True)
        if path == "blocking":
            y = np.concatenate([b.process(xs[:, k * BLOCK:(k + 1) * BLOCK]) for k in range(nb)], axis=2)[:, 0, :]
        else:
            y = _feed_tickets(b, xs, 8)
        b.close()
        return y

    y = run(bank.batch(n, BLOCK, stream_model=member_of), x)
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    assert sorted(set(member_of)) == list(range(8))
    for m, model in enumerate(models):
        rows = [s for s in range(n) if member_of[s] == m]
        want = run(model.batch(len(rows), BLOCK), np.ascontiguousarray(x[rows]))
        for i, s in enumerate(rows):
            assert np.array_equal(y[s], want[i]), (path, m, s)


def test_a2_bank_rebinding_in_a_running_session(nam_lib, member_paths):
    """After three commands of a session, streams {1, 17, 200} move to another member. From then on they equal a freshly reset
    (prewarmed) one-model batch of the new member fed the remaining input; every other stream equals the run without the swap;
    both bit for bit. An out-of-range member or stream fails and changes nothing."""
    nam = nam_lib
    n, nb = 256, 6
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    moved, new = [1, 17, 200], 6
    assert all(member_of[s] != new for s in moved)
    x = stream_bank(n, BLOCK * nb, seed=918)
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
    assert name == "nam_kq_kernel"
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


def test_a2_bank_session_in_turns(nam_lib, oracle, member_paths):
    """600 streams over 8 members: more workgroups than CUs, the session's workgroups take turns. Every stream finite; streams s
    and s + 8 (same member) are fed identical input in every other group of eight and must produce identical output; one stream
    of every group of eight — 75 streams, the member rotating with the group, so every member is covered — against the oracle
    (the 256-stream test above checks every stream, the pairwise equality covers the rest)."""
    nam = nam_lib
    n, nb = 600, 6
    models = _load(nam, member_paths)
    bank = nam.ModelBank(models)
    member_of = [s % 8 for s in range(n)]
    x = stream_bank(n, BLOCK * nb, seed=919)
    pairs = [s for s in range(n - 8) if (s // 8) % 2 == 0]
    for s in pairs:
        x[s + 8] = x[s]
    b = bank.batch(n, BLOCK, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = _drive(b, x, "session")
    b.close()
    assert name == "nam_kq_kernel"
    assert np.isfinite(y).all()
    for s in pairs:
        assert np.array_equal(y[s], y[s + 8]), s
    picks = [s for s in range(n) if s % 8 == (s // 8) % 8]
    assert len(picks) == 75
    worst = _oracle_errors(oracle, member_paths, member_of, x, y, picks)
    assert sorted(worst) == list(range(8))
    _assert_bounds(worst, member_paths)


def test_a2_bank_set_kernel_and_slimmable_size(nam_lib, member_paths):
    """set_kernel: AUTO and KERNEL_A1_MFMA (what a one-model A2 batch runs), nothing else; set_slimmable_size: what a
    non-slimmable model answers, although member 0 came from a container."""
    nam = nam_lib
    models = _load(nam, member_paths[:3])
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
    tool = os.path.join(ROOT, "cpp", "tools", "bank_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/bank_check"
    a, b = str(tmp_path / "a2_seed_a.nam"), str(tmp_path / "a2_seed_b.nam")
    write_a2(a, 461)
    write_a2(b, 462)
    r = subprocess.run([tool, model_path("A2"), a, b, "--refuse", model_path("wavenet_a1_standard")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAIL" not in r.stdout, r.stdout
