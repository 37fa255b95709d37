"""Stream slots of a live batch on the GPU (include/nam_hip.h: nam_hip_batch_restart_streams, nam_hip_batch_get_stream_state,
nam_hip_batch_set_stream_state): one case per kernel row of INTEGRATION.md's table, the kernel asserted through kernel_name.

Shapes: 5 streams (nam_lstm_row_kernel packs four streams per wavefront: one shared and one partial wavefront), 64-frame buffers
of signals.stream_bank, at most ten buffers per case. The Linear case R = 257 / max_frames 256 feeds 256-frame buffers: its ring of
896 rows wraps only then (six buffers: 1,536 frames). Prewarm on for wavenet_a1_standard, lstm and the A1 bank, off elsewhere.
Session-eligible cases run with persistent mode off ("plain") and on ("session"); everything is compared WITHIN one mode
(kernels of different launch classes differ by ~1e-7 by design). Every buffer is a blocking process() call: the kernel a call
runs then does not depend on what the batch did before.

Properties 1 to 3 compare GPU against GPU bit for bit (np.array_equal):
  1. restart  A: Reset, x, restart_streams([1, 3]), y.  B: fresh, Reset, y.  C: x then y undisturbed.  A's streams 1 and 3 on y
              equal B's, A's streams 0, 2, 4 equal C's; A's stream 1 on y is within the parity tolerance (test_gpu_parity.py: 5e-5
              x max(1, |ref|); Linear: tests/linear_oracle.py) of the oracle reset the same way; an LSTM's B differs from a batch
              that went x, Reset, y (Reset leaves h / c alone; restart_streams writes h0 / c0).
  2. rewind   x; blob = get(2); two buffers; set(2, blob); the same two buffers: stream 2 repeats its bits, the others equal an
              undisturbed run.
  3. move     the blob of A's stream 4 after x goes into stream 0 of a 3-stream batch D that has processed one unrelated buffer
              (other ring positions, Linear's lin_pos included): D's stream 0 on y equals A's stream 4 on y. The slimmable case
              moves into a slot of another width, the bank cases into a slot bound to another member (stream_model reports the
              blob's member afterwards).
  4. tickets  two tickets in flight, restart_streams, wait: the tickets' outputs equal a run without the restart.
  5. refusals another model's blob, a truncated blob, a flipped byte, Linear max_frames 256 against 1,024, a synth_a1_lite blob
              written under the A1 kernels set on a batch that has run under KERNEL_GENERIC: NamHipError(ERR_INVALID_ARGUMENT)
              naming the field, and the destination continues bit for bit as if nothing had been called."""
import json
import os

import numpy as np
import pytest

import linear_oracle as lo
from bank_models import write_lstm
from conftest import model_path
from signals import stream_bank

pytestmark = pytest.mark.gpu

N, ND = 5, 3  # streams of A / B / C, and of the move's destination D
SLIM = (1.0, 0.0, 1.0, 0.0, 1.0)  # slimmable_wavenet: widths 3 and 1 (tests/accuracy.py); D: all 0.0
MEMBERS, MEMBERS_D = (0, 1, 0, 1, 0), (1, 0, 1)


def _tol(fast_tanh):
    return 5e-5 if fast_tanh else 1e-4  # test_gpu_parity.py


class Case:
    """How a case's batches are made and what they must run. `plain` / `session`: the kernel kernel_name() reports with
    persistent mode off / on (session None: the case has no session); `force`: a NAM_HIP_KERNEL_* name for set_kernel."""

    def __init__(self, id, model=None, plain=None, session=None, force=None, prewarm=False, frames=64, max_frames=64, slim=False,
                 bank=None, doc=None, lstm=None):
        self.id, self.model, self.plain, self.session, self.force, self.prewarm = id, model, plain, session, force, prewarm
        self.frames, self.max_frames, self.slim, self.bank, self.doc, self.lstm = frames, max_frames, slim, bank, doc, lstm

    def paths(self, tmp):
        """the .nam files behind the case: one, or a bank's members"""
        if self.lstm is not None:
            p = os.path.join(tmp, f"{self.id}.nam")
            if not os.path.exists(p):
                write_lstm(p, 4040, **self.lstm)
            return [p]
        if self.bank is not None:
            out = []
            for i, m in enumerate(self.bank):
                if isinstance(m, str):
                    out.append(model_path(m))
                else:
                    p = os.path.join(tmp, f"{self.id}_{i}.nam")
                    if not os.path.exists(p):
                        write_lstm(p, 4100 + i, **m)
                    out.append(p)
            return out
        return [model_path(self.model)]

    def batch(self, nam, tmp, mode, n=N, dest=False, max_frames=None):
        """a batch of the case: kernel forced, widths / members set, persistent mode as `mode` says, NOT reset yet"""
        mf = max_frames or self.max_frames
        if self.doc is not None:
            b = nam.get_dsp_json(json.dumps(self.doc)).batch(n, mf)
        elif self.bank is not None:
            models = [nam.get_dsp(p, fast_tanh=True) for p in self.paths(tmp)]
            members = MEMBERS_D if dest else MEMBERS
            b = nam.ModelBank(models).batch(n, mf, stream_model=list(members[:n]))
        else:
            b = nam.get_dsp(self.paths(tmp)[0], fast_tanh=True).batch(n, mf)
        if self.force:
            b.set_kernel(getattr(nam, self.force))
        if self.slim:
            b.SetSlimmableSize(0.0, list(range(n)) if dest else [s for s in range(n) if SLIM[s] == 0.0])
        if mode == "session":
            assert b.set_persistent(True), self.id
        want = self.session if mode == "session" else self.plain
        names = want if isinstance(want, tuple) else (want,)
        assert b.kernel_name() in names, (self.id, mode, b.kernel_name())
        return b

    def oracle_run(self, oracle, tmp, stream, x):
        """the CPU reference of stream `stream` of A / B / C from a fresh instance, Reset as the case resets: (reference, tolerance)"""
        if self.doc is not None:
            h, bias = lo.taps_and_bias(self.doc)
            ys = lo.Yardstick(h, bias, x[None, :])
            return ys.truth[0], lo.FACTOR * ys.e32
        paths = self.paths(tmp)
        ref = oracle.get_dsp(paths[MEMBERS[stream] if self.bank is not None else 0], fast_tanh=True)
        if self.slim:
            ref.SetSlimmableSize(SLIM[stream])
        ref.Reset(48000.0, self.max_frames, prewarm=self.prewarm)
        r = ref.process_stream(x, self.frames)[0]
        return r, _tol(True) * max(1.0, float(np.max(np.abs(r))))


LSTM40 = dict(num_layers=1, input_size=1, hidden=40, out_channels=1)
LSTM3 = dict(num_layers=1, input_size=1, hidden=3, out_channels=1)
MFMA_LSTM = ("nam_lstm_mfma_kernel", "nam_lstm_mfma_reg_kernel")
CASES = [
    Case("a1_standard", "wavenet_a1_standard", "nam_a1_mfma_kernel", "nam_a1_q_kernel", prewarm=True),
    Case("a1_lite_padded", "synth_a1_lite", "nam_a1_mfma_kernel", "nam_a1_q_kernel"),
    Case("a1_nano", "synth_a1_nano", "nam_wn_reg_kernel", "nam_wn_reg_kernel"),
    Case("slimmable", "slimmable_wavenet", "nam_wn_reg_kernel", "nam_wn_reg_kernel", slim=True),
    Case("a2", "A2", "nam_kt_mfma_kernel", "nam_kq_kernel"),
    Case("kt_c8", "synth_kt_c8", "nam_kt_mfma_kernel"),
    Case("wavenet_generic", "wavenet", "nam_generic_kernel", force="KERNEL_GENERIC"),
    Case("wavenet_a1", "wavenet", "nam_a1_kernel", force="KERNEL_A1"),
    Case("lstm_row", "lstm", "nam_lstm_row_kernel", "nam_lstm_row_kernel", prewarm=True),
    Case("lstm_wide", "synth_lstm_h18x2", "nam_lstm_wide_kernel", "nam_lstm_wide_kernel"),
    Case("lstm_40", None, MFMA_LSTM, lstm=LSTM40),
    Case("linear_65", None, "nam_linear_kernel", doc=lo.linear_doc(65, True, seed=65)),
    Case("linear_257_wraps", None, "nam_linear_kernel", doc=lo.linear_doc(257, True, seed=257), frames=256, max_frames=256),
    Case("bank_a1", None, "nam_a1_p2_kernel", "nam_a1_q_kernel", prewarm=True, bank=("wavenet_a1_standard", "synth_a1_lite")),
    Case("bank_lstm", None, "nam_lstm_row_kernel", "nam_lstm_row_kernel", bank=("lstm", LSTM3)),
]
BY_ID = {c.id: c for c in CASES}
RUNS = [pytest.param(c.id, mode, id=f"{c.id}-{mode}") for c in CASES for mode in (("plain", "session") if c.session else ("plain",))]
LSTMS = {"lstm_row", "lstm_wide", "lstm_40", "bank_lstm"}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("stream_state_models"))


def _signal(n, frames, buffers, seed):
    x = stream_bank(n, frames * buffers, seed=seed)
    x.setflags(write=False)
    return x


def _feed(b, x, frames):
    """x [n, T] through blocking process() calls of `frames`: [n, T] (every case here has one output channel)"""
    ys = [b.process(np.ascontiguousarray(x[:, None, k:k + frames])) for k in range(0, x.shape[1], frames)]
    y = np.concatenate(ys, axis=2)
    assert y.shape[1] == 1 and np.isfinite(y).all()
    return y[:, 0, :]


_undisturbed = {}


def _xy(case):
    """the case's two signals, three buffers each: x (what the slots' first players send) and y"""
    return _signal(N, case.frames, 3, 11), _signal(N, case.frames, 3, 12)


def _run_c(nam, tmp, case, mode):
    """batch C, once per (case, mode): Reset, x then y undisturbed -> (its output on x, on y)"""
    key = (case.id, mode)
    if key not in _undisturbed:
        x, y = _xy(case)
        c = case.batch(nam, tmp, mode)
        c.Reset(prewarm=case.prewarm)
        out = (_feed(c, x, case.frames), _feed(c, y, case.frames))
        c.close()
        for a in out:
            a.setflags(write=False)
        _undisturbed[key] = out
    return _undisturbed[key]


# ---- 1. restart ----
@pytest.mark.parametrize("cid,mode", RUNS)
def test_restart(nam_lib, oracle, tmp, cid, mode):
    nam, case = nam_lib, BY_ID[cid]
    x, y = _xy(case)
    cx, cy = _run_c(nam, tmp, case, mode)
    a = case.batch(nam, tmp, mode)
    a.Reset(prewarm=case.prewarm)
    ax = _feed(a, x, case.frames)
    with pytest.raises(nam.NamHipError) as e:  # an id out of range changes nothing (the checks below would see it)
        a.restart_streams([1, N], prewarm=case.prewarm)
    assert e.value.code == nam.ERR_INVALID_ARGUMENT
    a.restart_streams([1, 3, 3], prewarm=case.prewarm)  # (duplicates are allowed)
    ay = _feed(a, y, case.frames)
    if case.bank is not None:  # (a bank stream keeps its member; a slimmable stream its width: B's streams 1 and 3 are narrow too)
        assert [a.stream_model(s) for s in range(N)] == list(MEMBERS)
    a.close()
    b = case.batch(nam, tmp, mode)
    b.Reset(prewarm=case.prewarm)
    by = _feed(b, y, case.frames)
    b.close()
    assert np.array_equal(ax, cx)
    for s in (1, 3):
        assert np.array_equal(ay[s], by[s]), (cid, mode, s, float(np.max(np.abs(ay[s] - by[s]))))
        assert not np.array_equal(ay[s], cy[s]), (cid, mode, s)  # (the restart did something)
    for s in (0, 2, 4):
        assert np.array_equal(ay[s], cy[s]), (cid, mode, s, float(np.max(np.abs(ay[s] - cy[s]))))
    ref, bound = case.oracle_run(oracle, tmp, 1, y[1])
    err = float(np.max(np.abs(ay[1].astype(np.float64) - ref)))
    print(f"restart {cid} {mode}: stream 1 against the oracle {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (cid, mode, err, bound)
    if cid in LSTMS:
        r = case.batch(nam, tmp, mode)
        r.Reset(prewarm=case.prewarm)
        _feed(r, x, case.frames)
        r.Reset(prewarm=case.prewarm)  # h / c stay as x left them (then the prewarm, if any)
        ry = _feed(r, y, case.frames)
        r.close()
        assert not np.array_equal(ry[1], by[1]), (cid, mode)


# ---- 2. rewind ----
@pytest.mark.parametrize("cid,mode", RUNS)
def test_rewind(nam_lib, tmp, cid, mode):
    nam, case = nam_lib, BY_ID[cid]
    x, y = _xy(case)
    u = y[:, :2 * case.frames]
    cx, cy = _run_c(nam, tmp, case, mode)
    a = case.batch(nam, tmp, mode)
    a.Reset(prewarm=case.prewarm)
    assert np.array_equal(_feed(a, x, case.frames), cx)
    blob = a.get_stream_state(2)
    assert isinstance(blob, bytes) and len(blob) > 80
    first = _feed(a, u, case.frames)
    assert np.array_equal(first, cy[:, :2 * case.frames])  # (get disturbs nothing)
    a.set_stream_state(2, blob)
    again = _feed(a, u, case.frames)
    a.close()
    assert np.array_equal(again[2], first[2]), (cid, mode, float(np.max(np.abs(again[2] - first[2]))))
    und = case.batch(nam, tmp, mode)  # x, u, u undisturbed
    und.Reset(prewarm=case.prewarm)
    _feed(und, x, case.frames)
    _feed(und, u, case.frames)
    want = _feed(und, u, case.frames)
    und.close()
    for s in (0, 1, 3, 4):
        assert np.array_equal(again[s], want[s]), (cid, mode, s)
    assert not np.array_equal(again[2], want[2]), (cid, mode)  # (the rewind did something)


# ---- 3. move ----
@pytest.mark.parametrize("cid,mode", RUNS)
def test_move(nam_lib, tmp, cid, mode):
    nam, case = nam_lib, BY_ID[cid]
    x, y = _xy(case)
    cx, cy = _run_c(nam, tmp, case, mode)
    a = case.batch(nam, tmp, mode)
    a.Reset(prewarm=case.prewarm)
    _feed(a, x, case.frames)
    blob = a.get_stream_state(4)
    a.close()  # (the blob outlives its batch)
    d = case.batch(nam, tmp, mode, n=ND, dest=True)
    d.Reset(prewarm=case.prewarm)
    _feed(d, _signal(ND, case.frames, 1, 99), case.frames)  # one unrelated buffer: D's rings stand elsewhere
    if case.bank is not None:
        assert d.stream_model(0) == MEMBERS_D[0] != MEMBERS[4]
    d.set_stream_state(0, blob)
    if case.bank is not None:
        assert [d.stream_model(s) for s in range(ND)] == [MEMBERS[4], MEMBERS_D[1], MEMBERS_D[2]]
    yd = np.ascontiguousarray(np.stack([y[4], y[0], y[1]]))
    dy = _feed(d, yd, case.frames)
    d.close()
    assert np.array_equal(dy[0], cy[4]), (cid, mode, float(np.max(np.abs(dy[0] - cy[4]))))
    # D's other streams: as if nothing had been called
    w = case.batch(nam, tmp, mode, n=ND, dest=True)
    w.Reset(prewarm=case.prewarm)
    _feed(w, _signal(ND, case.frames, 1, 99), case.frames)
    wy = _feed(w, yd, case.frames)
    w.close()
    for s in (1, 2):
        assert np.array_equal(dy[s], wy[s]), (cid, mode, s)
    assert not np.array_equal(dy[0], wy[0]), (cid, mode)


# ---- 4. tickets ----
@pytest.mark.parametrize("cid,mode", RUNS)
def test_tickets_in_flight_complete_before_a_restart(nam_lib, tmp, cid, mode):
    nam, case = nam_lib, BY_ID[cid]
    x, _ = _xy(case)
    cx, _ = _run_c(nam, tmp, case, mode)
    F = case.frames
    a = case.batch(nam, tmp, mode)
    a.Reset(prewarm=case.prewarm)
    first = _feed(a, x[:, :F], F)
    t1 = a.submit(np.ascontiguousarray(x[:, None, F:2 * F]))
    t2 = a.submit(np.ascontiguousarray(x[:, None, 2 * F:3 * F]))
    a.restart_streams([0, 4], prewarm=case.prewarm)
    got = np.concatenate([first, a.wait(t1)[:, 0, :], a.wait(t2)[:, 0, :]], axis=1)
    a.close()
    if mode == "plain":  # (a ticket and a blocking call run the same launches outside a session)
        assert np.array_equal(got, cx), (cid, mode)
        return
    t = case.batch(nam, tmp, mode)  # the same calls without the restart
    t.Reset(prewarm=case.prewarm)
    want = _feed(t, x[:, :F], F)
    w1 = t.submit(np.ascontiguousarray(x[:, None, F:2 * F]))
    w2 = t.submit(np.ascontiguousarray(x[:, None, 2 * F:3 * F]))
    want = np.concatenate([want, t.wait(w1)[:, 0, :], t.wait(w2)[:, 0, :]], axis=1)
    t.close()
    assert np.array_equal(got, want), (cid, mode)


# ---- 5. refusals ----
def _refused(nam, batch, stream, blob, field):
    with pytest.raises(nam.NamHipError) as e:
        batch.set_stream_state(stream, blob)
    assert e.value.code == nam.ERR_INVALID_ARGUMENT, str(e.value)
    assert "nam_hip_batch_set_stream_state: " + field in str(e.value), str(e.value)
    return str(e.value)


def _blob_after_x(nam, tmp, case, stream=4, max_frames=None):
    x, _ = _xy(case)
    a = case.batch(nam, tmp, "plain", max_frames=max_frames)
    a.Reset(prewarm=case.prewarm)
    _feed(a, x, case.frames)
    blob = a.get_stream_state(stream)
    a.close()
    return blob


def test_refusals_leave_the_destination_alone(nam_lib, tmp):
    nam, case = nam_lib, BY_ID["a1_standard"]
    x, y = _xy(case)
    cx, cy = _run_c(nam, tmp, case, "plain")
    good = _blob_after_x(nam, tmp, case)
    other = _blob_after_x(nam, tmp, BY_ID["a1_lite_padded"])
    d = case.batch(nam, tmp, "plain")
    d.Reset(prewarm=case.prewarm)
    assert np.array_equal(_feed(d, x, case.frames), cx)
    _refused(nam, d, 0, other, "model_fp")  # another model's blob
    for cut in (0, 3, 79, 80, len(good) // 2, len(good) - 1):  # truncated
        _refused(nam, d, 0, good[:cut], "size")
    _refused(nam, d, 0, good + b"\0", "size")
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x40
    _refused(nam, d, 0, bytes(flipped), "payload_sum")  # a flipped payload byte
    flipped = bytearray(good)
    flipped[17] ^= 0x01
    _refused(nam, d, 0, bytes(flipped), "model_fp")  # ... and a header byte
    with pytest.raises(nam.NamHipError):
        d.set_stream_state(N, good)  # (a stream out of range)
    with pytest.raises(nam.NamHipError):
        d.get_stream_state(-1)
    assert np.array_equal(_feed(d, y, case.frames), cy)
    d.set_stream_state(0, good)  # (the blob itself is fine: stream 0 goes on as stream 4 of C went on y)
    L = nam.load_library()
    import ctypes
    size = ctypes.c_int64(0)
    small = ctypes.create_string_buffer(16)
    assert L.nam_hip_batch_get_stream_state(d._h, 0, small, 16, ctypes.byref(size)) == nam.ERR_INVALID_ARGUMENT
    assert size.value == len(good) == L.nam_hip_batch_stream_state_size(d._h, 0)  # too small: the needed size comes back
    d.close()


def test_linear_blob_of_another_max_frames_class_is_refused(nam_lib, tmp):
    nam, case = nam_lib, BY_ID["linear_257_wraps"]
    x, y = _xy(case)
    blob = _blob_after_x(nam, tmp, case)  # max_frames 256: a ring of 896 rows
    d = case.batch(nam, tmp, "plain", max_frames=1024)  # 1,408 rows
    d.Reset()
    dx = _feed(d, x, case.frames)
    msg = _refused(nam, d, 0, blob, "lin_hist_frames")
    assert "max_frames" in msg
    dy = _feed(d, y, case.frames)
    d.close()
    w = case.batch(nam, tmp, "plain", max_frames=1024)
    w.Reset()
    assert np.array_equal(_feed(w, x, case.frames), dx) and np.array_equal(_feed(w, y, case.frames), dy)
    w.close()


def test_blob_of_another_state_layout_is_refused(nam_lib, tmp):
    """synth_a1_lite runs the A1 kernels on zero-padded rings and the op program on [R][C] rings: a blob written under the A1
    kernels does not fit a batch that has run under KERNEL_GENERIC (the existing "reset first"); it fits once that batch is
    freshly reset without prewarm."""
    nam, case = nam_lib, BY_ID["a1_lite_padded"]
    x, y = _xy(case)
    blob = _blob_after_x(nam, tmp, case)

    def generic():
        b = nam.get_dsp(model_path("synth_a1_lite"), fast_tanh=True).batch(N, 64)
        b.set_kernel(nam.KERNEL_GENERIC)
        assert b.kernel_name() == "nam_generic_kernel"
        b.Reset(prewarm=False)
        return b

    d = generic()
    dx = _feed(d, x, 64)
    msg = _refused(nam, d, 0, blob, "state_family")
    assert "reset first" in msg
    dy = _feed(d, y, 64)
    d.Reset(prewarm=False)
    d.set_stream_state(0, blob)  # freshly zeroed streams take the blob's layout
    d.close()
    w = generic()
    assert np.array_equal(_feed(w, x, 64), dx) and np.array_equal(_feed(w, y, 64), dy)
    w.close()


def test_stream_state_check_tool(nam_lib):
    """cpp/tools/stream_state_check: the move property once through BatchDSP (RestartStreams, GetStreamState, SetStreamState)"""
    import subprocess
    from conftest import ROOT
    tool = os.path.join(ROOT, "cpp", "tools", "stream_state_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/stream_state_check"
    r = subprocess.run([tool, model_path("wavenet_a1_standard")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAIL" not in r.stdout, r.stdout
