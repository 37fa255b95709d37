"""A container of the official WaveNet topology's tiers (feather 8 / 4, lite 12 / 6, standard 16 / 8: tests/a1_mixed.py) at mixed
sizes in persistent mode: the streams share ONE session of nam_a1_q_kernel through the interleaved-frame kernels' bank path, every
stream's rings in the standard submodel's rows; a control call that mixes or un-mixes the batch copies the other streams' rows
(nam_state_rows_copy_kernel) without disturbing them.

The shape: six streams on (standard, lite, feather, lite, standard, feather), 64-frame buffers of signals.stream_bank, one
37-frame call in front (control calls and row copies land at odd ring positions), 20 whole buffers = 1,280 frames on each side of a
transition (more than the longest ring's 2 x 512 + 64 rows: every ring wraps), prewarm on. The yardsticks: np.array_equal against
ModelBank([feather, lite, standard]) with the same assignment, which runs this very mix in the BANK_A1_IL family; the flat bound
5e-5 x max(1, |ref|max) of tests/test_gpu_parity.py against the CPU oracle of the stream's own submodel; 4 x e32 against the
float64 oracle (tests/accuracy.py). Scenarios that read the `nam_hip session:` line (NAM_HIP_SESSION_STATS is read once per
process) run tests/a1_mixed.py as a child process, as tests/test_gpu_a2_mixed.py does.

Before this feature set_persistent answered 0 on such a batch and every call was a plain launch per size:
test_mixed_batch_is_one_session fails there on its first assertion."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import a1_mixed as am
import accuracy
import session_lengths as sl
from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu

TOL = 5e-5  # x max(1, |ref|max), fast tanh: test_gpu_parity.py::_tol


def run_child(what, tmp):
    env = {k: v for k, v in os.environ.items() if k != "NAM_HIP_MAX_STAGES"}
    env["NAM_HIP_SESSION_STATS"] = "1"
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "a1_mixed.py"), what, str(tmp)],
                       env=env, capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139):  # the child was killed by a signal: nothing more on this GPU from this run
        pytest.exit(f"tests/a1_mixed.py {what} ended with {r.returncode}:\n{r.stdout}{r.stderr}", returncode=3)
    said = [ln for ln in r.stdout.splitlines() if ln.startswith("a1_mixed: ")]
    assert r.returncode == 0 and len(said) == 1, r.stdout + r.stderr
    ans = json.loads(said[0][len("a1_mixed: "):])
    lines = sl.session_lines(r.stderr)
    print(said[0])
    print("nam_hip session lines (starts, launches, commands):", lines)
    print("\n".join(ln for ln in r.stderr.splitlines() if "mixed sizes" in ln or "session launches" in ln))
    ans["launch_lines"] = [(int(m.group(1)), int(m.group(2))) for m in
                           re.finditer(r"^nam_hip session launches: (\d+) publish every command, (\d+) of them linger$", r.stderr, re.M)]
    return ans, lines


def load(tmp, *names):
    return [np.load(os.path.join(str(tmp), f + ".npy")) for f in names]


def oracle_run(oracle, x, tier):
    """a fresh reference of the tier's own submodel after Reset (prewarm included), 64-frame calls over x [frames]"""
    ref = oracle.get_dsp(model_path(am.FIXTURES[tier]), fast_tanh=True)
    ref.Reset(48000.0, am.BLOCK)
    return np.asarray(ref.process_stream(np.ascontiguousarray(x), am.BLOCK)).reshape(-1)  # (one output channel)


def within(what, got, ref):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    err, scale = float(np.max(np.abs(ref - got))), max(1.0, float(np.max(np.abs(ref))))
    print(f"{what}: max|gpu - oracle| {err:.3e}, bound {TOL * scale:.3e}")
    assert np.isfinite(got).all() and err <= TOL * scale, (what, err, scale)


def test_mixed_batch_is_one_session(oracle, tmp_path):
    """set_persistent answers True on the batch at mixed sizes and the batch names nam_a1_q_kernel; behind the 37-frame call 20
    device-window calls are exactly 1 start and 20 commands; the bank twin runs the same kernel and gives the same bits; the
    four-tier container (with nano) at mixed sizes answers False as before; every stream within the flat bound of its own
    submodel's oracle (the 37 frames of the plain launch included)."""
    ans, lines = run_child("session", tmp_path)
    assert ans["persistent"], "set_persistent answered 0 on the container at mixed sizes"
    assert ans["kernel"] == am.Q and ans["kernel_1024"] == am.Q, ans
    assert (ans["kernel_bank"], ans["kernel_bank_1024"]) == (ans["kernel"], ans["kernel_1024"]), ans
    assert ans["commands"] == am.SIDE and lines == [(1, lines[0][1], am.SIDE), (1, lines[1][1], am.SIDE)], (lines, ans["commands"])
    assert ans["differ_from_bank"] == [], ("streams that differ from the bank batch's", ans["differ_from_bank"])
    assert ans["persistent_four_tier"] is False, ans
    x, y = load(tmp_path, "x", "y")
    assert float(np.abs(y).max()) > 1e-3
    for s, t in enumerate(am.TIERS):
        within(f"stream {s} on {am.FIXTURES[t]}", y[s, 0], oracle_run(oracle, x[s, 0], t))


@pytest.mark.parametrize("what", ["tickets", "blocking"])
def test_host_paths_equal_the_bank(oracle, tmp_path, what):
    """Tickets of 64 frames eight deep, and 20 blocking 64-frame calls back to back: one session each, a command per buffer, the
    same kernel names as the bank twin before and after (the short-burst switch to nam_a1_p4_kernel included) and the same bits;
    every stream within the flat bound of its submodel's oracle."""
    ans, lines = run_child(what, tmp_path)
    assert ans["kernel"] == am.Q and ans["kernel_bank"] == ans["kernel"] and ans["kernel_bank_end"] == ans["kernel_end"], ans
    assert ans["kernel_end"] in (am.Q, am.P4), ans
    assert [(ln[0], ln[2]) for ln in lines] == [(1, ans["commands"])] * 2, (lines, ans["commands"])
    for publishing, lingering in ans["launch_lines"]:  # (tests/test_gpu_a2_mixed.py: the launch publishes every command and lingers)
        assert publishing >= 1 and lingering >= 1, ans["launch_lines"]
    assert ans["differ_from_bank"] == [], ("streams that differ from the bank batch's", ans["differ_from_bank"])
    x, y = load(tmp_path, "x", "y")
    for s, t in enumerate(am.TIERS):
        within(f"{what}: stream {s} on {am.FIXTURES[t]}", y[s, 0], oracle_run(oracle, x[s, 0], t))


def test_transitions_do_not_disturb_the_other_streams(oracle, tmp_path):
    """Behind the 37-frame call and 20 buffers stream 1 goes from lite to standard; 20 buffers later every lite and feather stream
    goes to standard (the batch is at one size: the plain form of the kernel); 20 buffers later stream 0 goes to feather (mixed
    again). A stream equals the twin batch nothing happened to, bit for bit, up to the first call that names it — stream 4
    throughout — and from that call on it equals the same stream of a fresh batch at the sizes behind the call, bit for bit."""
    ans, lines = run_child("transitions", tmp_path)
    assert [ans[k] for k in ("kernel_before_a", "kernel_after_a", "kernel_after_b", "kernel_after_c")] == [am.Q] * 4, ans
    assert ans["differ_from_twin"] == [], ("streams that differ from the undisturbed twin before any call named them", ans["differ_from_twin"], ans["until"])
    for name in "abc":
        f = ans["fresh"][name]
        assert f["moved"] and f["differ"] == [], (name, "moved streams that differ from a fresh stream of their new size", f)
    # a control call ends the session: the batch with the three calls starts four, the twin one
    assert [(ln[0], ln[2]) for ln in lines[:2]] == [(4, 4 * am.SIDE), (1, 4 * am.SIDE)], lines
    x, y = load(tmp_path, "x", "y")
    c_a, c_b, c_c = ans["cuts"]
    within("stream 1 as a fresh standard from A on", y[1, 0, c_a:], oracle_run(oracle, x[1, 0, c_a:], am.STANDARD))
    within("stream 2 as a fresh standard from B on", y[2, 0, c_b:], oracle_run(oracle, x[2, 0, c_b:], am.STANDARD))
    within("stream 0 as a fresh feather from C on", y[0, 0, c_c:], oracle_run(oracle, x[0, 0, c_c:], am.FEATHER))
    within("stream 5, feather up to B", y[5, 0, :c_b], oracle_run(oracle, x[5, 0, :c_b], am.FEATHER))


def test_stream_slots_in_the_resident_state(oracle, tmp_path):
    """restart_streams([2]) of the resident batch: nobody else notices, stream 2 starts over as a fresh feather. get_stream_state(3),
    two buffers, set_stream_state(3, blob): the two buffers give the same bits again. The lite stream's blob out of the resident
    batch is byte for byte the blob it gives once persistent mode is off, and as long as an all-lite batch's; set into an all-lite
    batch (which has no session, as ever) that batch goes on with the source's bits in launches of four buffers, which run the
    session's kernel, nam_a1_q_kernel; in one-buffer launches (nam_a1_mfma_kernel) it goes on within the oracle bound."""
    ans, _ = run_child("slots", tmp_path)
    r = ans["restart"]
    assert r["kernel_after_restart"] == am.Q and r["differ"] == [] and r["named_before_equal"], r
    x, y_restart = load(tmp_path, "x", "y_restart")
    within("restarted stream 2: a fresh feather", y_restart[2, 0, r["cut"]:], oracle_run(oracle, x[2, 0, r["cut"]:], am.FEATHER))
    assert ans["kernel"] == am.Q and ans["kernel_after_get"] == am.Q and ans["kernel_after_set"] == am.Q, ans
    assert ans["rewind_repeats"], "set_stream_state did not take stream 3 back to where get_stream_state found it"
    assert ans["blob_identical"] and ans["blob_bytes"][0] == ans["blob_bytes_all_lite"], ans
    # an all-lite batch launches per call, as ever: where its launches run the session's kernel it goes on with the source's bits ...
    print("destination against the source, max |difference|: nam_a1_q_kernel", ans["dst_max_diff_q"], "nam_a1_mfma_kernel", ans["dst_max_diff_mfma"])
    assert ans["kernel_dst_q"] == am.Q and ans["dst_continues_source_q"], ans
    # ... and in one-buffer launches (nam_a1_mfma_kernel: another summation order) within the oracle bound of the uninterrupted stream
    assert ans["kernel_dst_mfma"] == "nam_a1_mfma_kernel", ans
    y_dst, = load(tmp_path, "y_dst_mfma")
    within("the blob continued by nam_a1_mfma_kernel", y_dst[0], oracle_run(oracle, x[3, 0], am.LITE)[r["cut"]:])


def test_ragged_call_inside_the_mode(oracle, tmp_path):
    """Calls of 64, 64, 32, 64, 64 frames: the 32-frame call ends the session and runs as one plain launch of the bank form
    (nam_a1_p2_kernel, as a bank batch), the next whole buffer starts the session again — two starts, four commands; every stream
    within the flat bound of its submodel's oracle."""
    ans, lines = run_child("guard", tmp_path)
    assert ans["kernel"] == am.Q and ans["kernel_32"] == am.P2 and ans["kernel_bank_32"] == am.P2, ans
    assert lines == [(2, lines[0][1], 4)], lines
    x, y = load(tmp_path, "x", "y")
    for s, t in enumerate(am.TIERS):
        within(f"stream {s} on {am.FIXTURES[t]}", y[s, 0], oracle_run(oracle, x[s, 0], t))


def test_mixed_session_within_four_e32_of_the_truth(nam_lib):
    """tests/accuracy.py's float64 yardstick on the mixed session: eight streams, stream s on tier s % 3, twelve buffers through
    one session of nam_a1_q_kernel; every stream is held to 4 x e32 of its own submodel (the suite's bound,
    tests/test_gpu_accuracy.py), so each tier is held at least twice."""
    import torch
    nam = nam_lib
    tiers = [s % 3 for s in range(accuracy.N_STREAMS)]
    x = accuracy.inputs(1.0)
    b = am.make(nam, tiers)
    assert b.kernel_name() == am.Q, b.kernel_name()
    xd = torch.from_numpy(x[:, None, :].copy()).cuda()
    yd = torch.zeros((x.shape[0], 1, x.shape[1]), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k in range(x.shape[1] // 64):
        b.process_device(xd.data_ptr() + k * 64 * 4, yd.data_ptr() + k * 64 * 4, 64, x.shape[1])
    b.flush()
    assert b.kernel_name() == am.Q
    b.synchronize()
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    b.close()
    assert np.isfinite(y).all()
    for tier, name in enumerate(am.FIXTURES):
        streams = [s for s, t in enumerate(tiers) if t == tier]
        ys = accuracy.yardstick(name, True, 1.0)
        e_gpu = float(np.max(np.abs(y[streams].astype(np.float64) - ys.truth[streams])))
        print(f"ACCURACY a1_mixed_session {name} fast_tanh=1 amp=1.0 peak={ys.peak:.3f} e32={ys.e32:.3e} e_gpu={e_gpu:.3e} "
              f"e_gpu/e32={e_gpu / ys.e32:.2f}")
        assert e_gpu <= accuracy.FACTOR * ys.e32, (name, e_gpu, ys.e32, e_gpu / ys.e32)
