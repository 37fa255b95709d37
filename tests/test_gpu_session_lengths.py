"""Persistent sessions of nam_wn_reg_kernel, nam_lstm_row_kernel and nam_lstm_wide_kernel take calls of ANY length: a call of n
frames is n / 64 whole commands and one partial command (csrc/session_command.h; tests/test_session_command.py holds the word
itself on the CPU). One fixed schedule of call lengths (tests/session_lengths.py: partial commands first, last and between whole
ones, 1 .. 480 frames, an odd sum, repeated past twice the longest history ring) runs through every case, walking one device window
(offsets of any alignment) and on one buffer at offset 0 with a flush between calls, and three contracts hold:
  1. every stream equals, np.array_equal, the same calls on a fresh batch with persistent mode off after the same Reset(prewarm) —
     where the session runs the form a plain launch runs (NOT_BIT_EQUAL_TO_PLAIN_LAUNCHES below names the others and what holds
     for them instead); and in every case the same signal through a session in whole 64-frame commands, and the two addressing
     variants against each other;
  2. streams against the CPU oracle of their model / member / width: 5e-5 x max(1, |ref|max) with fast tanh, the bound of
     tests/test_gpu_parity.py, test_gpu_bank_wr.py and test_gpu_bank_lstm.py for these fixtures;
  3. the session stayed resident: the `nam_hip session:` line (NAM_HIP_SESSION_STATS=1, read once per process: every case is a child
     process) reports exactly 1 start and sum(ceil(n / 64)) commands. Before variable-length commands the same run reported a start
     per run of whole buffers and only the whole buffers as commands (nano: 4 starts, 4 commands instead of 1 and 56).
Then the host paths (blocking 32-frame calls, 48-frame tickets and a 480-frame one), the stream slots across a partial command, and
a guard: the pipeline kernels (nam_a1_q_kernel, nam_kq_kernel) keep the multiple-of-64 rule exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import session_lengths as sl
from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = 5e-5  # x max(1, |ref|max), fast tanh: test_gpu_parity.py::_tol


def run_child(what, name, tmp, extra_env=None):
    """tests/session_lengths.py as a process of its own: (its JSON answer, its `nam_hip session:` lines)"""
    env = {k: v for k, v in os.environ.items() if k != "NAM_HIP_MAX_STAGES"}
    env["NAM_HIP_SESSION_STATS"] = "1"
    env.update(extra_env or {})
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "session_lengths.py"), what, name, str(tmp)],
                       env=env, capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139):  # the child was killed by a signal: nothing more on this GPU from this run
        pytest.exit(f"tests/session_lengths.py {what} {name} ended with {r.returncode}:\n{r.stdout}{r.stderr}", returncode=3)
    said = [ln for ln in r.stdout.splitlines() if ln.startswith("session_lengths: ")]
    assert r.returncode == 0 and len(said) == 1, r.stdout + r.stderr
    ans = json.loads(said[0][len("session_lengths: "):])
    lines = sl.session_lines(r.stderr)
    print(said[0])
    print("nam_hip session lines (starts, launches, commands):", lines)
    return ans, lines


# Contract 1 compares with persistent mode off, where a call of up to 64 frames is a launch of ONE wavefront per stream. Twelve
# streams of these cases run their sessions as two or four wavefronts per stream (the op program cut into stages: the head
# accumulator is summed in another order), and that form is not bit-equal to the one-wavefront launch — measured BEFORE this
# feature, on whole and ragged calls alike (profiles/session_lengths/README.md). They are held to the oracle bound instead, every
# stream of both addressing variants (the plugin pattern's flush per call makes such a session start its launches as one wavefront
# per stream after three one-call bursts — DESIGN.md 4.6 —, so it equals neither the walk nor the plain launches throughout). For
# EVERY case the walk must equal, bit for bit, the same signal through a session in whole 64-frame commands: the same form, and
# where a call ends changes no frame's arithmetic.
NOT_BIT_EQUAL_TO_PLAIN_LAUNCHES = {("nano", None), ("nano", 2), ("a2_max", None), ("nano_bank3", None)}


def check_schedule(oracle, name, tmp, max_stages=None):
    ans, lines = run_child("schedule", name, tmp, {"NAM_HIP_MAX_STAGES": str(max_stages)} if max_stages else None)
    n = ans["streams"]
    exact = (name, max_stages) not in NOT_BIT_EQUAL_TO_PLAIN_LAUNCHES
    # contract 1
    for how in ("walk", "plugin"):
        assert ans[how]["finite"] and ans[how]["peak"] > 1e-3, (how, ans[how])
        if exact:
            assert ans[how]["differ"] == [], (how, "streams that differ from persistent mode off", ans[how]["differ"])
    assert ans["walk64"]["differ"] == [], ("streams that differ from the session in whole commands", ans["walk64"]["differ"])
    if exact:
        assert ans["plugin"]["differ_from_walk"] == [], ("streams of the plugin pattern that differ from the walk", ans["plugin"]["differ_from_walk"])
    # contract 3: the walk's batch, the plugin pattern's (a flush is no session end: one start there too), the whole-command walk's
    assert ans["order"] == ["walk", "plugin", "walk64"] and len(lines) == 3, (ans["order"], lines)
    for how, (starts, _, n_cmds) in zip(ans["order"], lines):
        want = ans["walk64"]["commands"] if how == "walk64" else ans["commands"]
        assert (starts, n_cmds) == (1, want), (how, "starts, commands", starts, n_cmds, "expected", 1, want)
    # contract 2 (every stream where contract 1 cannot be exact)
    x, y, yp = (np.load(os.path.join(tmp, f)) for f in ("x.npy", "y_walk.npy", "y_plugin.npy"))
    paths, member_of, ratio_of = ans["paths"], ans["member_of"], ans["ratio_of"]
    for s in ((0, 1, n - 1) if exact else range(n)):
        ref = oracle.get_dsp(paths[member_of[s]], fast_tanh=True)
        if ratio_of[s] is not None:
            ref.SetSlimmableSize(ratio_of[s])
        ref.Reset(48000.0, sl.BLOCK)
        r = ref.process_stream(x[s], sl.BLOCK)
        scale = max(1.0, float(np.max(np.abs(r))))
        for how, got in (("walk", y), ("plugin", yp)):
            err = float(np.max(np.abs(r - got[s])))
            print(f"{name} stream {s} {how}: max|gpu - oracle| {err:.3e}, |ref|max {scale:.3f}")
            assert err <= TOL * scale, (name, how, s, err, scale)


@pytest.mark.parametrize("name", list(sl.CASES))
def test_any_length_schedule(oracle, tmp_path, name):
    check_schedule(oracle, name, str(tmp_path))


@pytest.mark.parametrize("max_stages", [2, 1])
def test_any_length_schedule_nano_fewer_wavefronts(oracle, tmp_path, max_stages):
    """the nano case as two wavefronts per stream and as one (twelve streams run four under the default policy:
    tests/test_gpu_launch_policy.py)"""
    check_schedule(oracle, "nano", str(tmp_path), max_stages)


@pytest.mark.parametrize("name", ["slimmable_two_widths", "lstm_row"])  # (sessions that are bit-equal to plain launches: see above)
@pytest.mark.parametrize("what", ["blocking", "tickets"])
def test_host_paths_any_length(tmp_path, what, name):
    """40 blocking process() calls of 32 frames back to back; tickets of 48 frames with 8 in flight, then a 480-frame ticket: bit for
    bit the same calls with persistent mode off, one command per 32- or 48-frame buffer and 8 for the 480-frame one."""
    ans, lines = run_child(what, name, str(tmp_path))
    assert ans[what]["finite"] and ans[what]["peak"] > 1e-3, ans[what]
    assert ans[what]["differ"] == [], ans[what]["differ"]
    assert len(lines) == 1 and lines[0][2] == ans["commands"], (lines, ans["commands"])


@pytest.mark.parametrize("name,kernels", [("wavenet_a1_standard", ("nam_a1_q_kernel", "nam_a1_p4_kernel")), ("A2", ("nam_kq_kernel",))])
def test_pipeline_kernels_keep_the_multiple_of_64_rule(oracle, tmp_path, name, kernels):
    """64, 64, 32, 64, 64 frames in persistent mode: only the four whole buffers are commands, in two sessions (the ragged call ends
    the first and runs as a plain launch) — the statistics of before this feature, unchanged. The outputs: a session of these
    kernels and a plain launch are different kernels of a family and were never bit-equal (measured before this feature:
    profiles/session_lengths/README.md), so every stream is held to the oracle bound; what persistent mode off gives is printed."""
    ans, lines = run_child("guard", name, str(tmp_path))
    assert ans["kernel"] in kernels, ans["kernel"]
    assert ans["guard"]["finite"] and ans["guard"]["peak"] > 1e-3, ans["guard"]
    print("streams that differ from persistent mode off:", ans["guard"]["differ"])
    assert lines == [(2, lines[0][1], 4)], lines
    x, y = np.load(os.path.join(str(tmp_path), "x.npy")), np.load(os.path.join(str(tmp_path), "y_guard.npy"))
    for s in range(x.shape[0]):
        ref = oracle.get_dsp(sl.model_file(name), fast_tanh=True)
        ref.Reset(48000.0, sl.BLOCK)
        r = ref.process_stream(x[s], sl.BLOCK)
        err, scale = float(np.max(np.abs(r - y[s]))), max(1.0, float(np.max(np.abs(r))))
        assert err <= TOL * scale, (name, s, err, scale)


# --- stream slots across a partial command (no statistics needed: in this process)

@pytest.fixture(scope="module")
def slot_cases(nam_lib, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("session_lengths_slots"))
    return {name: sl.Case(nam_lib, name, tmp) for name in ("nano", "lstm_row")}


LENS_SLOTS = [64, 17] + sl.LENS  # the control call comes after the 17-frame command


@pytest.mark.parametrize("name", ["nano", "lstm_row"])
def test_stream_state_moves_after_a_partial_command(slot_cases, name):
    """get_stream_state of stream 3 behind a 17-frame command, set_stream_state into slot 7 (fed stream 3's input from there on): the
    destination continues bit for bit as the source, and the source as in the run without the calls"""
    c = slot_cases[name]
    x = c.signal(seed=979, T=sum(LENS_SLOTS))
    x[7, :, 81:] = x[3, :, 81:]
    b = c.make(True)
    plain = sl.walk(b, x, LENS_SLOTS, True)
    b.close()

    def hook(b, k):
        if k == 2:
            b.set_stream_state(7, b.get_stream_state(3))

    b = c.make(True)
    y = sl.walk(b, x, LENS_SLOTS, True, hook=hook)
    b.close()
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 1e-3
    assert np.array_equal(y[7, :, 81:], y[3, :, 81:])
    assert not np.array_equal(plain[7, :, 81:], plain[3, :, 81:])  # (without the move the two differ: their histories do)
    for s in range(c.n):
        if s != 7:
            assert np.array_equal(y[s], plain[s]), s
    assert np.array_equal(y[7, :, :81], plain[7, :, :81])


@pytest.mark.parametrize("name", ["nano", "lstm_row"])
def test_restart_streams_after_a_partial_command(slot_cases, name):
    """restart_streams of stream 5 behind a 17-frame command leaves every other stream bit-identical to the run without it; stream 5
    continues as a fresh batch after Reset(prewarm) fed the remaining input"""
    c = slot_cases[name]
    x = c.signal(seed=980, T=sum(LENS_SLOTS))
    b = c.make(True)
    plain = sl.walk(b, x, LENS_SLOTS, True)
    b.close()
    b = c.make(True)
    y = sl.walk(b, x, LENS_SLOTS, True, hook=lambda b, k: b.restart_streams([5]) if k == 2 else None)
    b.close()
    for s in range(c.n):
        if s != 5:
            assert np.array_equal(y[s], plain[s]), s
    assert np.array_equal(y[5, :, :81], plain[5, :, :81])
    assert not np.array_equal(y[5, :, 81:], plain[5, :, 81:])
    b = c.make(True)
    fresh = sl.walk(b, np.ascontiguousarray(x[:, :, 81:]), sl.LENS, True)
    b.close()
    assert np.array_equal(y[5, :, 81:], fresh[5])
