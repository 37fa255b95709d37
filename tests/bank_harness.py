"""What the model-bank tests of the three families share (test_gpu_bank.py, test_gpu_bank_a2.py, test_gpu_bank_lstm.py and their
host-side *_abi.py files): how a batch is driven in each launch class, the one-model batches a bank is compared with, and the
bodies of the tests that are the same for every family. A family's file keeps its constants (members, kernels, stream counts,
seeds, bounds) and the tests only it has.

Signals are rank 3 throughout, x [n, in_channels, T] -> y [n, out_channels, T]: the mono families add the axis where they make
their signal (`mono`)."""
import ctypes
import gc
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from conftest import ROOT, model_path
from signals import stream_bank

BLOCK = 64

# What the shared bodies need to know of a family: `paths` the member files (stream s runs member s % len(paths)), `signal(n, T,
# seed)` its test input [n, in_channels, T], `il_singles` whether one-model batches of the `blocks` class are told KERNEL_A1_IL (see
# singles).
Family = namedtuple("Family", "paths signal il_singles", defaults=(False,))


def mono(n, T, seed):
    """signals.stream_bank as [n, 1, T]"""
    return stream_bank(n, T, seed=seed)[:, None, :]


def load(nam, paths, fast_tanh=True):
    return [nam.get_dsp(p, fast_tanh=fast_tanh) for p in paths]


def fixture(nam, name, fast_tanh=True):
    return nam.get_dsp(model_path(name), fast_tanh=fast_tanh)


def drive(b, x, mode, hook=None):
    """x [n, ic, T] through batch `b` on device-resident buffers; returns (y [n, oc, T], the kernel the runtime names for the mode).
    session: persistent mode, one command per 64 frames, a flush after the third and at the end;
    bursts : persistent mode, a flush after every command (after three such bursts the launches start as the low-latency kernel);
    blocks : a plain launch per 64 frames (all three: T a multiple of 64);    launch : one plain launch over the whole signal (any T).
    hook(k): called before block k (session mode)."""
    import torch
    n, _, T = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.zeros((n, b.model.NumOutputChannels(), T), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nb = T // BLOCK
    assert mode == "launch" or T % BLOCK == 0
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
    return yd.cpu().numpy(), name


def singles(nam, models, member_of, x, mode, il=False, max_frames=BLOCK, prewarm=True):
    """The same audio through one-model batches: for each member a batch of the streams bound to it, after Reset(prewarm). Returns y
    and the kernel names seen. `il`: the batches are told KERNEL_A1_IL (a lone 64-frame launch of a one-model batch of the official
    topology runs nam_a1_mfma_kernel under AUTO; the bank runs the A1_IL family); else they run under AUTO."""
    y, names = None, set()
    for m, model in enumerate(models):
        rows = [s for s in range(x.shape[0]) if member_of[s] == m]
        if not rows:
            continue
        b = model.batch(len(rows), max_frames)
        if il:
            b.set_kernel(nam.KERNEL_A1_IL)
        b.Reset(prewarm=prewarm)
        ym, name = drive(b, np.ascontiguousarray(x[rows]), mode)
        b.close()
        if y is None:
            y = np.zeros((x.shape[0],) + ym.shape[1:], dtype=np.float32)
        y[rows] = ym
        names.add(name)
    return y, names


def feed_tickets(batch, x, depth):
    """x in 64-frame buffers through submit / wait with up to `depth` tickets in flight"""
    nb = x.shape[-1] // BLOCK
    ys, tickets = [], []
    for k in range(nb):
        if len(tickets) == depth:
            ys.append(batch.wait(tickets.pop(0)))
        tickets.append(batch.submit(x[:, :, k * BLOCK:(k + 1) * BLOCK]))
    while tickets:
        ys.append(batch.wait(tickets.pop(0)))
    return np.concatenate(ys, axis=2)


def oracle_errors(oracle, paths, member_of, x, y, streams, fast_tanh=True):
    """worst (relative, absolute, |ref|max) per member over `streams`, printed"""
    worst = {}
    for s in streams:
        ref = oracle.get_dsp(paths[member_of[s]], fast_tanh=fast_tanh)
        ref.Reset(48000.0, BLOCK)
        r = ref.process_stream(x[s], BLOCK)
        abs_err = float(np.max(np.abs(r - y[s])))
        rel = abs_err / max(1.0, float(np.max(np.abs(r))))
        w = worst.setdefault(member_of[s], [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], rel), max(w[1], abs_err), max(w[2], float(np.max(np.abs(r))))
    for m in sorted(worst):
        print(f"member {m} ({os.path.basename(paths[m])}): worst relative {worst[m][0]:.3e}, absolute {worst[m][1]:.3e}, |y|max {worst[m][2]:.3f}")
    return worst


def run_reset(bank, member_of, max_frames, x, mode, hook=None):
    """a fresh bank batch, Reset with prewarm, `x` through it: (y, kernel name)"""
    b = bank.batch(len(member_of), max_frames, stream_model=member_of)
    b.Reset(prewarm=True)
    y, name = drive(b, x, mode, hook=(lambda k: hook(b, k)) if hook else None)
    b.close()
    return y, name


def session_against_oracle(nam, oracle, fam, kernel, seed):
    """256 streams (stream s -> member s % members) in persistent mode: six 64-frame commands, a flush after the third, after Reset
    with prewarm. EVERY stream against the oracle of its member: returns oracle_errors' answer, every member in it."""
    n = 256
    bank = nam.ModelBank(load(nam, fam.paths))
    M = len(fam.paths)
    member_of = [s % M for s in range(n)]
    x = fam.signal(n, BLOCK * 6, seed)
    b = bank.batch(n, BLOCK, stream_model=member_of)
    assert [b.stream_model(s) for s in (0, 1, M - 1, n - 1)] == [0, 1, M - 1, (n - 1) % M]
    b.Reset(prewarm=True)
    y, name = drive(b, x, "session")
    b.close()
    assert name == kernel
    assert np.isfinite(y).all()
    worst = oracle_errors(oracle, fam.paths, member_of, x, y, range(n))
    assert sorted(worst) == list(range(M))
    return worst


def session_in_turns(nam, oracle, fam, kernel, seed):
    """600 streams over 8 members: more workgroups than CUs, the session's workgroups take turns. Every stream finite; streams s and
    s + 8 (same member) are fed identical input in every other group of eight and must produce identical output; one stream of every
    group of eight — 75 streams, the member rotating with the group, so every member is covered — against the oracle: returns
    oracle_errors' answer."""
    n = 600
    bank = nam.ModelBank(load(nam, fam.paths))
    assert len(fam.paths) == 8
    member_of = [s % 8 for s in range(n)]
    x = fam.signal(n, BLOCK * 6, seed)
    pairs = [s for s in range(n - 8) if (s // 8) % 2 == 0]
    for s in pairs:
        x[s + 8] = x[s]
    y, name = run_reset(bank, member_of, BLOCK, x, "session")
    assert name == kernel
    assert np.isfinite(y).all()
    for s in pairs:
        assert np.array_equal(y[s], y[s + 8]), s
    picks = [s for s in range(n) if s % 8 == (s // 8) % 8]
    assert len(picks) == 75
    worst = oracle_errors(oracle, fam.paths, member_of, x, y, picks)
    assert sorted(worst) == list(range(8))
    return worst


def bit_for_bit(nam, fam, mode, kernel, T, seed, n):
    """The bank against one-model batches, all `n` streams, np.array_equal; the kernel is asserted for the bank AND for the
    one-model batches. Also: every two members differ on identical input (a bank that ran member 0 for everyone would have failed
    already — this shows that the comparison could tell). Returns (x, the bank's output, member_of, models)."""
    models = load(nam, fam.paths)
    bank = nam.ModelBank(models)
    M = len(models)
    member_of = [s % M for s in range(n)]
    x = fam.signal(n, T, seed)
    max_frames = T if mode == "launch" else BLOCK
    y, name = run_reset(bank, member_of, max_frames, x, mode)
    assert name == kernel
    want, names = singles(nam, models, member_of, x, mode, il=fam.il_singles and mode == "blocks", max_frames=max_frames)
    assert names == {kernel}
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    bad = [s for s in range(n) if not np.array_equal(y[s], want[s])]
    assert not bad, (mode, len(bad), bad[:8])
    yM, _ = run_reset(bank, list(range(M)), max_frames, np.repeat(x[:1], M, axis=0), mode)
    for m in range(M):
        for m2 in range(m + 1, M):
            assert not np.array_equal(yM[m], yM[m2]), (m, m2)
    return x, y, member_of, models


def rebinding(nam, fam, kernel, n, moved, new, probe, seed):
    """After three commands of a six-command session the streams `moved` go to member `new`. From then on they equal a freshly reset
    (prewarmed) one-model batch of the new member fed the remaining input; every other stream equals the run without the move; both
    bit for bit. An out-of-range member (with in-range streams) or stream (with the in-range member `probe`) fails and changes
    nothing."""
    models = load(nam, fam.paths)
    bank = nam.ModelBank(models)
    M = len(models)
    member_of = [s % M for s in range(n)]
    assert all(member_of[s] != new for s in moved)
    x = fam.signal(n, BLOCK * 6, seed)
    plain, _ = run_reset(bank, member_of, BLOCK, x, "session")

    def hook(b, k):
        if k == 3:
            for bad_member, bad_stream in ((M, 5), (-1, 5), (probe, n), (probe, -1)):
                with pytest.raises(nam.NamHipError) as e:
                    b.set_stream_model(bad_member, [5, bad_stream])
                assert e.value.code == nam.ERR_INVALID_ARGUMENT
            assert [b.stream_model(s) for s in range(n)] == member_of
            b.set_stream_model(new, moved)
            assert [b.stream_model(s) for s in range(n)] == [new if s in moved else member_of[s] for s in range(n)]
            b.set_stream_model(new, moved)  # already there: a no-op (the streams are NOT reset again)

    y, name = run_reset(bank, member_of, BLOCK, x, "session", hook=hook)
    assert name == kernel
    for s in range(n):
        if s not in moved:
            assert np.array_equal(y[s], plain[s]), s
    for s in moved:
        assert np.array_equal(y[s, :, :3 * BLOCK], plain[s, :, :3 * BLOCK]), s
    fresh = models[new].batch(len(moved), BLOCK)
    fresh.Reset(prewarm=True)
    want, _ = drive(fresh, np.ascontiguousarray(x[moved][:, :, 3 * BLOCK:]), "session")
    fresh.close()
    for i, s in enumerate(moved):
        assert np.array_equal(y[s, :, 3 * BLOCK:], want[i]), s
        assert not np.array_equal(y[s, :, 3 * BLOCK:], plain[s, :, 3 * BLOCK:])
    return bank, models


def host_paths(nam, fam, path, n, nb, step, seed, depth, kernel=None):
    """Host buffers on an `n`-stream bank batch (stream s on member s * step % members) in persistent mode: `nb` blocking process
    calls of 64 frames back to back (path "blocking"; the lingering launch serves them), or tickets with `depth` in flight. Bit for
    bit against one-model batches driven the same way. `kernel`: what kernel_name() must say once the session is on.
    Returns (x, y, member_of)."""
    models = load(nam, fam.paths)
    bank = nam.ModelBank(models)
    member_of = [(s * step) % len(models) for s in range(n)]
    x = fam.signal(n, BLOCK * nb, seed)

    def run(b, xs):
        assert b.set_persistent(True)
        assert kernel is None or b.kernel_name() == kernel
        b.Reset(prewarm=True)
        if path == "blocking":
            y = np.concatenate([b.process(xs[:, :, k * BLOCK:(k + 1) * BLOCK]) for k in range(nb)], axis=2)
        else:
            y = feed_tickets(b, xs, depth)
        b.close()
        return y

    y = run(bank.batch(n, BLOCK, stream_model=member_of), x)
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    assert sorted(set(member_of)) == list(range(len(models)))
    for m, model in enumerate(models):
        rows = [s for s in range(n) if member_of[s] == m]
        want = run(model.batch(len(rows), BLOCK), np.ascontiguousarray(x[rows]))
        for i, s in enumerate(rows):
            assert np.array_equal(y[s], want[i]), (path, m, s)
    return x, y, member_of


def check_tool(members, refuse):
    """cpp/tools/bank_check on the member files; the file `refuse` must be refused next to them"""
    tool = os.path.join(ROOT, "cpp", "tools", "bank_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/bank_check"
    r = subprocess.run([tool] + list(members) + ["--refuse", refuse], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAIL" not in r.stdout, r.stdout


# --- the host side (no device): test_bank_abi.py, test_bank_a2_abi.py, test_bank_lstm_abi.py

def refused(nam, models, member):
    with pytest.raises(nam.NamHipError) as e:
        nam.ModelBank(models)
    assert e.value.code == nam.ERR_UNSUPPORTED, str(e.value)
    assert f"member {member}" in str(e.value), str(e.value)
    return str(e.value)


def survives_its_models(nam, paths, make_junk):
    """A bank of the two files at `paths` copies what it needs: the member models are freed (their handles through
    nam_hip_model_free) before the bank is asked anything; make_junk() allocates over the freed models' memory."""
    L = nam.load_library()
    handles = []
    for path in paths:
        h = ctypes.c_void_p()
        assert L.nam_hip_model_load(path.encode(), 1, ctypes.byref(h)) == 0
        handles.append(h)
    arr = (ctypes.c_void_p * 2)(*[h.value for h in handles])
    bank = ctypes.c_void_p()
    assert L.nam_hip_bank_create(arr, 2, ctypes.byref(bank)) == 0, L.nam_hip_last_error()
    for h in handles:
        L.nam_hip_model_free(h)
    junk = make_junk()
    assert L.nam_hip_bank_n_models(bank) == 2
    # a stream_model entry outside the bank is refused before any device call
    out = ctypes.c_void_p()
    bad = (ctypes.c_int * 4)(0, 1, 2, 0)
    assert L.nam_hip_batch_create_bank(bank, 0, 4, 64, bad, ctypes.byref(out)) == nam.ERR_INVALID_ARGUMENT
    assert b"member 2" in L.nam_hip_last_error() and out.value is None
    L.nam_hip_bank_free(bank)
    del junk
    gc.collect()
