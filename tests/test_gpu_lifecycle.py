"""-m gpu: what a batch owns, created, used, destroyed and created again (csrc/device_owner.h: every device allocation, pinned or
mapped host buffer, stream and event of the host runtime is an owner that releases when the batch goes). One case per class of
resource, four cycles each on one device: every cycle bit for bit what the first gave, the first cycle's stream 0 against the CPU
oracle. Then a batch whose state buffer the device must refuse: the half-built batch goes, the next one works.

The smallest shapes that reach the code: 3 streams, max_frames 64 (tickets: 128, for two buffers of different length). Only what
the API documents as legal; nothing here is meant to fail on the device. The LSTM scratch buffer's grow path is covered by
test_gpu_breadth.py::test_lstm_larger_than_lds_runs_from_global_scratch."""
import ctypes

import numpy as np
import pytest

from bank_harness import BLOCK, drive
from conftest import model_path
from signals import stream_bank
from test_gpu_parity import _oracle_run, _tol

pytestmark = pytest.mark.gpu

N, CYCLES = 3, 4


def _blocking(b, x, persistent):
    assert bool(b.set_persistent(persistent)) == persistent
    b.Reset(prewarm=True)
    return b.process_stream(x, BLOCK)


def _plain(nam, x):
    """(a) plain launches, the staging buffers of the blocking entry points"""
    b = nam.get_dsp(model_path("wavenet_a1_standard"), fast_tanh=True).batch(N, BLOCK)
    y = _blocking(b, x, False)
    b.close()
    return y


def _session_device(nam, x, name="wavenet_a1_standard", kernel=None):
    """(b) a session on device buffers: three 64-frame commands, a flush — destroyed with persistent mode still on"""
    b = nam.get_dsp(model_path(name), fast_tanh=True).batch(N, BLOCK)
    b.Reset(prewarm=True)
    y, seen = drive(b, x[:, None, :], "session")
    assert kernel is None or seen == kernel
    b.close()
    return y


def _session_host(nam, x):
    """(c) blocking host calls inside a session: the windows both sides can reach"""
    b = nam.get_dsp(model_path("wavenet_a1_standard"), fast_tanh=True).batch(N, BLOCK)
    y = _blocking(b, x, True)
    b.close()
    return y


def _tickets(nam, x, persistent):
    """(d) two tickets (128 and 64 frames), both waited for, then destroyed. Outside persistent mode: the copying form's staging and
    the slots' events; inside: the ticket windows."""
    b = nam.get_dsp(model_path("wavenet_a1_standard"), fast_tanh=True).batch(N, 2 * BLOCK)
    assert bool(b.set_persistent(persistent)) == persistent
    b.Reset(prewarm=True)
    t0 = b.submit(x[:, :2 * BLOCK])
    t1 = b.submit(x[:, 2 * BLOCK:])
    y = np.concatenate([b.wait(t0), b.wait(t1)], axis=2)
    b.close()
    return y


def _lstm_session(nam, x):
    """(e) an LSTM in a session"""
    return _session_device(nam, x, "lstm", "nam_lstm_row_kernel")


def _slimmable(nam, x):
    """(f) stream 1 to the narrowest width and back, a call in between: the groups' stream maps and the moved streams' reset"""
    b = nam.get_dsp(model_path("slimmable_wavenet"), fast_tanh=True).batch(N, BLOCK)
    b.Reset(prewarm=True)
    ys = [b.process(x[:, :BLOCK])]
    b.SetSlimmableSize(0.0, [1])
    ys.append(b.process(x[:, BLOCK:2 * BLOCK]))
    b.SetSlimmableSize(1.0, [1])
    ys.append(b.process(x[:, 2 * BLOCK:]))
    b.close()
    return np.concatenate(ys, axis=2)


def _bank(nam, x):
    """(g) a two-member bank of the standard topology, stream 2 rebound between two calls"""
    bank = nam.ModelBank([nam.get_dsp(model_path(n), fast_tanh=True) for n in ("wavenet_a1_standard", "synth_a1_lite")])
    b = bank.batch(N, BLOCK, stream_model=[0, 1, 0])
    b.Reset(prewarm=True)
    ys = [b.process(x[:, :BLOCK])]
    b.set_stream_model(1, [2])
    assert [b.stream_model(s) for s in range(N)] == [0, 1, 1]
    ys.append(b.process_stream(x[:, BLOCK:], BLOCK))
    b.close()
    return np.concatenate(ys, axis=2)


def _timeline_then_call(nam, x):
    """(h) the profiling instantiation once (it runs silence through the streams), a Reset, then an ordinary call: the profiling
    buffer is gone with the call that made it, the launches that follow are the ordinary ones"""
    b = nam.get_dsp(model_path("wavenet_a1_standard"), fast_tanh=True).batch(N, BLOCK)
    b.Reset(prewarm=True)
    stamps = b.debug_timeline(BLOCK)
    assert stamps.shape == (96, 8)
    y = _blocking(b, x, False)
    b.close()
    return y


# case -> (what a cycle does, the model stream 0 runs, the buffer size its oracle is reset with)
CASES = {
    "a_plain_launches": (_plain, "wavenet_a1_standard", BLOCK),
    "b_session_device_buffers": (_session_device, "wavenet_a1_standard", BLOCK),
    "c_session_host_windows": (_session_host, "wavenet_a1_standard", BLOCK),
    "d_tickets_copies": (lambda nam, x: _tickets(nam, x, False), "wavenet_a1_standard", 2 * BLOCK),
    "d_tickets_session": (lambda nam, x: _tickets(nam, x, True), "wavenet_a1_standard", 2 * BLOCK),
    "e_lstm_session": (_lstm_session, "lstm", BLOCK),
    "f_slimmable_moves": (_slimmable, "slimmable_wavenet", BLOCK),
    "g_bank_rebinding": (_bank, "wavenet_a1_standard", BLOCK),
    "h_debug_timeline": (_timeline_then_call, "wavenet_a1_standard", BLOCK),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_create_use_destroy_create_again(nam_lib, oracle, case):
    cycle, name, block = CASES[case]
    x = stream_bank(N, 3 * BLOCK, seed=900 + len(case))
    first = cycle(nam_lib, x)
    assert first.shape == (N, 1, 3 * BLOCK) and np.isfinite(first).all()
    for k in range(1, CYCLES):
        assert np.array_equal(cycle(nam_lib, x), first), (case, k)
    r = _oracle_run(oracle, name, x[0], block, True)
    err, scale = float(np.max(np.abs(r - first[0]))), max(1.0, float(np.max(np.abs(r))))
    print(f"{case}: stream 0 against the oracle {err:.3e} (|y|max {scale:.3f})")
    assert err <= _tol(True) * scale, (case, err, scale)
    if case == "h_debug_timeline":  # what a batch that never ran the profiling instantiation gives
        assert np.array_equal(first, _plain(nam_lib, x))


@pytest.mark.parametrize("name,kernel", [("wavenet_a1_standard", "nam_a1_q_kernel"), ("wavenet_a2_max", "nam_wn_reg_kernel")])
def test_call_forms_interleaved_on_one_batch(nam_lib, oracle, name, kernel):
    """What a launch runs depends on the call it serves (a blocking host call of up to four buffers starts nam_a1_p4_kernel where
    nam_a1_q_kernel would run; one of a single buffer runs nam_wn_reg_kernel as one wavefront per stream) and on nothing an earlier
    call left behind: blocking calls of every class, tickets, a blocking call again and a call outside persistent mode on ONE
    batch, each followed by a call of another class. The calls run different kernels of one family, so the concatenated output
    is held against the oracle, every stream, not against another call form."""
    max_frames = 8 * BLOCK
    lengths = [BLOCK, 8 * BLOCK, 4 * BLOCK, BLOCK, 2 * BLOCK, BLOCK, BLOCK, 8 * BLOCK]
    at = np.concatenate([[0], np.cumsum(lengths)])
    x = stream_bank(N, int(at[-1]), seed=977)
    part = lambda k: x[:, at[k]:at[k + 1]]
    b = nam_lib.get_dsp(model_path(name), fast_tanh=True).batch(N, max_frames)
    assert b.set_persistent(True)
    assert b.kernel_name(BLOCK) == kernel
    b.Reset(prewarm=True)
    ys = [b.process(part(k)) for k in range(4)]
    tickets = [b.submit(part(4)), b.submit(part(5))]
    ys += [b.wait(t) for t in tickets]
    ys.append(b.process(part(6)))
    assert not b.set_persistent(False)
    ys.append(b.process(part(7)))
    b.close()
    y = np.concatenate(ys, axis=2)
    assert y.shape == (N, 1, at[-1]) and np.isfinite(y).all()
    for s in range(N):
        r = _oracle_run(oracle, name, x[s], max_frames, True)
        err, scale = float(np.max(np.abs(r - y[s]))), max(1.0, float(np.max(np.abs(r))))
        print(f"{name}, stream {s}: against the oracle {err:.3e} (|y|max {scale:.3f})")
        assert err <= _tol(True) * scale, (name, s, err, scale)


def test_refused_allocation_leaves_nothing_behind(nam_lib, oracle):
    """nam_hip_batch_create with so many streams that the STATE buffer alone ([n_streams][state bytes per stream]: the oversized
    request, ensure_state's hipMalloc) exceeds the device's total memory: the runtime refuses that one request at once — nothing of
    the size is ever allocated — after the blobs were uploaded; the half-built batch is destroyed through its owners. The call
    answers NAM_HIP_ERR_DEVICE with a null handle and names the allocation; a 3-stream batch made right afterwards renders what
    the oracle renders."""
    import torch
    nam = nam_lib
    L = nam.load_library()
    model = nam.get_dsp(model_path("wavenet_a1_standard"), fast_tanh=True)
    total = torch.cuda.mem_get_info()[1]
    per_stream = int(model.info.state_bytes_per_stream)
    assert per_stream > 0
    n_streams = total // per_stream + 1
    assert n_streams * per_stream > total
    assert n_streams <= 1 << 26, "the host-side per-stream vectors stay small (else: oversize the staging buffer through max_frames)"
    h = ctypes.c_void_p()
    rc = L.nam_hip_batch_create(model._h, 0, int(n_streams), BLOCK, ctypes.byref(h))
    msg = L.nam_hip_last_error().decode()
    assert rc == nam.ERR_DEVICE and not h.value, (rc, h.value, msg)
    assert "hipMalloc" in msg and "d_state" in msg, msg
    x = stream_bank(N, 3 * BLOCK, seed=77)
    y = _plain(nam, x)
    for s in range(N):
        r = _oracle_run(oracle, "wavenet_a1_standard", x[s], BLOCK, True)
        assert float(np.max(np.abs(r - y[s]))) <= _tol(True) * max(1.0, float(np.max(np.abs(r)))), s
