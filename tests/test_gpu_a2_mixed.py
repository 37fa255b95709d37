"""A2.nam at mixed sizes in persistent mode: Lite and Full streams share ONE session of nam_kq_kernel, the Lite streams zero-padded
onto the Full layout through the kernels' bank path, and a size change that mixes or un-mixes the batch moves the other streams'
state between nam_wn_reg_kernel's layout and the padded rings (nam_a2_transcode_kernel) without disturbing them.

The shape: six streams at ratios [1.0, 0.0, 0.4, 0.7, 0.2, 0.9] (A2-Lite below 0.5), 64-frame buffers, 38 buffers = 2,432 frames
on each side of a transition (twice the longest reach, 5 x 239, and every ring wraps), a 17-frame call in front of every
transition. The oracle bound is 5e-5 x max(1, |ref|max), what tests/test_gpu_parity.py holds this fixture to. Scenarios that read
the `nam_hip session:` line (NAM_HIP_SESSION_STATS is read once per process) run tests/a2_mixed.py as a child process, in the
pattern of tests/session_lengths.py.

Before this feature set_persistent answered 0 on such a batch and every call was two plain launches:
test_mixed_batch_is_one_session fails there on its first assertion."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import a2_mixed as am
import accuracy
import session_lengths as sl
from conftest import ROOT, model_path

pytestmark = pytest.mark.gpu

TOL = 5e-5  # x max(1, |ref|max), fast tanh: test_gpu_parity.py::_tol


def run_child(what, tmp):
    env = {k: v for k, v in os.environ.items() if k != "NAM_HIP_MAX_STAGES"}
    env["NAM_HIP_SESSION_STATS"] = "1"
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "a2_mixed.py"), what, str(tmp)],
                       env=env, capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139):  # the child was killed by a signal: nothing more on this GPU from this run
        pytest.exit(f"tests/a2_mixed.py {what} ended with {r.returncode}:\n{r.stdout}{r.stderr}", returncode=3)
    said = [ln for ln in r.stdout.splitlines() if ln.startswith("a2_mixed: ")]
    assert r.returncode == 0 and len(said) == 1, r.stdout + r.stderr
    ans = json.loads(said[0][len("a2_mixed: "):])
    lines = sl.session_lines(r.stderr)
    print(said[0])
    print("nam_hip session lines (starts, launches, commands):", lines)
    print("\n".join(ln for ln in r.stderr.splitlines() if "A2 mixed sizes" in ln or "session launches" in ln))
    ans["launch_lines"] = [(int(m.group(1)), int(m.group(2))) for m in
                           re.finditer(r"^nam_hip session launches: (\d+) publish every command, (\d+) of them linger$", r.stderr, re.M)]
    return ans, lines


def load(tmp, *names):
    return [np.load(os.path.join(str(tmp), f + ".npy")) for f in names]


def oracle_run(oracle, x, ratio):
    """a fresh reference at `ratio` after Reset (prewarm included), 64-frame calls over x [frames]"""
    ref = oracle.get_dsp(model_path("A2"), fast_tanh=True)
    ref.SetSlimmableSize(ratio)
    ref.Reset(48000.0, am.BLOCK)
    return np.asarray(ref.process_stream(np.ascontiguousarray(x), am.BLOCK)).reshape(-1)  # (one output channel)


def within(what, got, ref):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    err, scale = float(np.max(np.abs(ref - got))), max(1.0, float(np.max(np.abs(ref))))
    print(f"{what}: max|gpu - oracle| {err:.3e}, bound {TOL * scale:.3e}")
    assert np.isfinite(got).all() and err <= TOL * scale, (what, err, scale)


def test_mixed_batch_is_one_session(oracle, tmp_path):
    """set_persistent answers True on the batch at mixed sizes; 76 buffers are exactly 1 start and 76 commands of nam_kq_kernel; every
    stream within the oracle bound at its own ratio."""
    ans, lines = run_child("session", tmp_path)
    assert ans["persistent"] and ans["kernel"] == am.KQ and ans["kernel_1024"] == am.KQ, ans
    assert lines == [(1, lines[0][1], ans["commands"])] and ans["commands"] == 2 * am.SIDE, (lines, ans["commands"])
    x, y = load(tmp_path, "x", "y")
    assert float(np.abs(y).max()) > 1e-3
    for s, r in enumerate(am.RATIOS):
        within(f"stream {s} at ratio {r}", y[s, 0], oracle_run(oracle, x[s, 0], r))


def test_a_size_change_does_not_disturb_the_other_streams(oracle, tmp_path):
    """The sharp one. An all-Lite persistent batch (nam_wn_reg_kernel); behind a 17-frame call stream 2 goes to Full and — no process
    call in between — back: the batch was mixed (every other stream moved to the padded rings) and un-mixed (and back), and every
    stream the calls did not name equals the run without them bit for bit. Then the same with the episode spanning 40 buffers on
    nam_kq_kernel: the other streams stay within the oracle bound of an uninterrupted A2-Lite throughout, the named stream continues
    as a fresh A2-Full from its first buffer at that size and as a fresh A2-Lite from its first buffer back."""
    ans, _ = run_child("continuity", tmp_path)
    assert ans["kernel_all_lite"] == am.WR, ans
    t = ans["there_and_back"]
    assert t["kernel_mixed"] == am.KQ and t["kernel_after"] == am.WR, t
    assert t["differ"] == [], ("streams the size change did not name, and that differ from the run without it", t["differ"])
    assert t["named_before_equal"] and t["named_after_differs"], t
    x, ya, yb, yc = load(tmp_path, "x", "ya", "yb", "yc")
    named, (c1, c2) = ans["episode"]["named"], ans["episode"]["cuts"]
    cut = c1
    within("there and back: the named stream, a fresh A2-Lite from the transition on", yb[named, 0, cut:],
           oracle_run(oracle, x[named, 0, cut:ya.shape[2]], am.LITE))
    e = ans["episode"]
    assert e["kernel_in"] == am.KQ and e["kernel_episode_end"] == am.KQ and e["kernel_out"] == am.WR, e
    for s in range(x.shape[0]):
        if s == named:
            continue
        within(f"episode: stream {s}, A2-Lite throughout", yc[s, 0], oracle_run(oracle, x[s, 0], am.LITE))
    within("episode: the named stream before", yc[named, 0, :c1], oracle_run(oracle, x[named, 0, :c1], am.LITE))
    within("episode: the named stream as a fresh A2-Full", yc[named, 0, c1:c2], oracle_run(oracle, x[named, 0, c1:c2], am.FULL))
    within("episode: the named stream as a fresh A2-Lite again", yc[named, 0, c2:], oracle_run(oracle, x[named, 0, c2:], am.LITE))


def test_stream_slots_on_the_mixed_batch(oracle, tmp_path):
    """get_stream_state of a Lite stream that lives padded is a blob in nam_wn_reg_kernel's layout, the size an all-Lite batch's is:
    set into all-Lite batches of four streams it continues there on that batch's own kernel — the same bits whichever slot takes it,
    and within the oracle bound of the uninterrupted stream. The other way round a blob of an all-Lite batch continues in a padded
    slot. restart_streams of a Lite and a Full stream of the mixed batch: nobody else notices, the two start over as fresh models."""
    ans, _ = run_child("slots", tmp_path)
    assert ans["kernel"] == am.KQ and ans["kernel_dst"] == am.WR and ans["kernel_after_set"] == am.KQ, ans
    assert ans["blob_bytes_mixed"] == ans["blob_bytes_all_lite"], ans
    assert ans["dst_slots_equal"], "the same blob continued differently in two slots of the same kind of batch"
    x, y_src, y_dst, y_restart, x_set, y_set = load(tmp_path, "x", "y_src", "y_dst", "y_restart", "x_set", "y_set")
    src, cut = 1, ans["restart"]["cut"]
    ref = oracle_run(oracle, x[src, 0], am.RATIOS[src])
    within("the source stream, undisturbed by get_stream_state", y_src[src, 0], ref)
    within("the destination continues the source", y_dst[0], ref[cut:])
    r = ans["restart"]
    assert r["kernel_after_restart"] == am.KQ and r["differ"] == [] and r["named_before_equal"], r
    for s in r["who"]:
        within(f"restarted stream {s}: a fresh model at ratio {am.RATIOS[s]}", y_restart[s, 0, cut:], oracle_run(oracle, x[s, 0, cut:], am.RATIOS[s]))
    ref = oracle_run(oracle, x_set[0], am.LITE)
    within("a blob of an all-Lite batch continues in a padded slot", y_set[0], ref[ans["set_cut"]:])


@pytest.mark.parametrize("what", ["tickets", "blocking"])
def test_host_paths_on_the_mixed_batch(oracle, tmp_path, what):
    """Tickets of 64 frames eight deep, and 40 blocking 64-frame calls back to back: one session, a command per buffer, every stream
    within the oracle bound at its ratio; the launch publishes every command and lingers for the next buffer, so the calls ride a
    few launches — tests/test_gpu_session_completion.py's bounds: at most ten for the 40 blocking calls, at most a quarter of the
    tickets."""
    ans, lines = run_child(what, tmp_path)
    assert ans["kernel"] == am.KQ and ans["kernel_end"] == am.KQ, ans
    assert lines == [(1, lines[0][1], ans["commands"])], (lines, ans["commands"])
    (publishing, lingering), = ans["launch_lines"]
    assert publishing >= 1 and lingering >= 1, ans["launch_lines"]
    assert lines[0][1] <= (10 if what == "blocking" else ans["commands"] // 4), lines
    x, y = load(tmp_path, "x", "y")
    for s, r in enumerate(am.RATIOS):
        within(f"{what}: stream {s} at ratio {r}", y[s, 0], oracle_run(oracle, x[s, 0], r))


def test_mixed_session_within_four_e32_of_the_truth(nam_lib):
    """tests/accuracy.py's float64 yardstick on one mixed case: eight streams, even ones A2-Lite, odd ones A2-Full, twelve buffers
    through one session of nam_kq_kernel; a stream is held to 4 x e32 of its own size (the suite's bound, tests/test_gpu_accuracy.py).
    Measured on an MI355X: e_gpu / e32 = 1.47 (A2-Lite, zero-padded) and 2.02 (A2-Full), see profiles/a2_mixed/README.md."""
    import torch
    nam = nam_lib
    widths = {am.LITE: [0, 2, 4, 6], am.FULL: [1, 3, 5, 7]}
    x = accuracy.inputs(1.0)
    model = nam.get_dsp(model_path("A2"), fast_tanh=True)
    b = model.batch(accuracy.N_STREAMS, 64)
    b.Reset(prewarm=True)
    for ratio, streams in widths.items():
        b.SetSlimmableSize(ratio, streams)
    assert b.set_persistent(True) and b.kernel_name() == am.KQ, b.kernel_name()
    xd = torch.from_numpy(x[:, None, :].copy()).cuda()
    yd = torch.zeros((x.shape[0], 1, x.shape[1]), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k in range(x.shape[1] // 64):
        b.process_device(xd.data_ptr() + k * 64 * 4, yd.data_ptr() + k * 64 * 4, 64, x.shape[1])
    b.flush()
    assert b.kernel_name() == am.KQ
    b.synchronize()
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    b.close()
    assert np.isfinite(y).all()
    for ratio, streams in widths.items():
        ys = accuracy.yardstick("A2", True, 1.0, ratio)
        e_gpu = float(np.max(np.abs(y[streams].astype(np.float64) - ys.truth[streams])))
        print(f"ACCURACY a2_mixed_session A2 ratio={ratio} fast_tanh=1 amp=1.0 peak={ys.peak:.3f} e32={ys.e32:.3e} e_gpu={e_gpu:.3e} "
              f"e_gpu/e32={e_gpu / ys.e32:.2f}")
        assert e_gpu <= accuracy.FACTOR * ys.e32, (ratio, e_gpu, ys.e32, e_gpu / ys.e32)
