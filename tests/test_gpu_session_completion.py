"""Sessions of nam_wn_reg_kernel, nam_lstm_row_kernel and nam_lstm_wide_kernel publish every command (csrc/persist_wave.h:
complete) when they serve host buffers: a ticket completes when ITS last command has, a blocking call waits for its own command
and the next call finds the launch still there (it lingers: wait_command). Every case of tests/session_lengths.py — the counter
with 12 workgroups and with one, a last wavefront of one stream, two width groups in one launch, the BANK instantiations, one,
two and four wavefronts per stream, the per-model code object and the table form — runs in a child process
(tests/session_completion.py: NAM_HIP_SESSION_STATS is read once per process) that feeds it 40 blocking calls of 64 and of 32
frames and three ticket feeds, and:
  1. blocking calls ride one launch: 1 start, 40 commands, at most 10 launches (40 before: every such call ended in a flush of
     the whole launch), and the foreign device-wide synchronize in the middle returns in under 50 ms;
  2. tickets: 1 start, sum(ceil(n / 64)) commands, launches at most a quarter of the tickets;
  3. values: every stream of every run against the CPU oracle at 5e-5 x max(1, |ref|max) — the bound of these fixtures' parity
     tests —; bit for bit the same calls with persistent mode off for the forms that are held to it (NAM_HIP_MAX_STAGES=1, the
     slimmable case, the LSTM cases: profiles/session_lengths/README.md); bit for bit a device-window session fed the same call
     lengths in the same wavefront form (NAM_HIP_MAX_STAGES is set for the whole child);
  4. a batch of more streams than the chip holds at once publishes and never lingers;
  5. Reset, restart_streams and set_stream_state complete the tickets in flight."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import session_lengths as sl
from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = 5e-5  # x max(1, |ref|max), fast tanh: test_gpu_parity.py::_tol
SYNC_BOUND_S = 0.05  # tests/test_gpu_tickets.py: test_blocking_calls_back_to_back_ride_one_lingering_launch
MAX_LAUNCHES_BLOCKING = 10

# variant: (case, streams (0: the case's own), environment, bit-equal to persistent mode off)
# NAM_HIP_MAX_STAGES=4 is the default cap said aloud: every batch of the child, ticket run and device-window run alike, is held to it
VARIANTS = {
    "nano": ("nano", 0, {"NAM_HIP_MAX_STAGES": "4"}, False),
    "a2_max": ("a2_max", 0, {"NAM_HIP_MAX_STAGES": "4"}, False),
    "slimmable_two_widths": ("slimmable_two_widths", 0, {"NAM_HIP_MAX_STAGES": "4"}, True),
    "nano_bank3": ("nano_bank3", 0, {"NAM_HIP_MAX_STAGES": "4"}, False),
    "lstm_row": ("lstm_row", 0, {"NAM_HIP_MAX_STAGES": "4"}, True),
    "lstm_wide": ("lstm_wide", 0, {"NAM_HIP_MAX_STAGES": "4"}, True),
    "lstm_bank2": ("lstm_bank2", 0, {"NAM_HIP_MAX_STAGES": "4"}, True),
    "nano_one_wavefront": ("nano", 0, {"NAM_HIP_MAX_STAGES": "1"}, True),
    "nano_two_wavefronts": ("nano", 0, {"NAM_HIP_MAX_STAGES": "2"}, False),
    "nano_one_stream": ("nano", 1, {"NAM_HIP_MAX_STAGES": "4"}, False),
    "a2_max_table_form": ("a2_max", 0, {"NAM_HIP_MAX_STAGES": "4", "NAM_HIP_JIT": "0"}, False),
}


def launch_lines(stderr):
    """[(publishing, lingering)] of the `nam_hip session launches:` lines, one per batch that ran a session"""
    return [(int(m.group(1)), int(m.group(2)))
            for m in re.finditer(r"^nam_hip session launches: (\d+) publish every command, (\d+) of them linger$", stderr, re.M)]


def run_child(what, name, tmp, streams=0, plain_too=False, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("NAM_HIP_MAX_STAGES", "NAM_HIP_JIT")}
    env["NAM_HIP_SESSION_STATS"] = "1"
    env.update(extra_env or {})
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else [])
                       + [os.path.join(ROOT, "tests", "session_completion.py"), what, name, str(tmp), str(streams), "1" if plain_too else "0"],
                       env=env, capture_output=True, text=True, timeout=240)
    if r.returncode < 0 or r.returncode in (134, 139):  # the child was killed by a signal: nothing more on this GPU from this run
        pytest.exit(f"tests/session_completion.py {what} {name} ended with {r.returncode}:\n{r.stdout}{r.stderr}", returncode=3)
    said = [ln for ln in r.stdout.splitlines() if ln.startswith("session_completion: ")]
    assert r.returncode == 0 and len(said) == 1, r.stdout + r.stderr
    ans = json.loads(said[0][len("session_completion: "):])
    ans["lines"] = sl.session_lines(r.stderr)
    ans["launch_lines"] = launch_lines(r.stderr)
    ans["stderr"] = r.stderr
    print(said[0])
    print("nam_hip session lines (starts, launches, commands):", ans["lines"])
    print("nam_hip session launches lines (publishing, lingering):", ans["launch_lines"])
    return ans


_children = {}


@pytest.fixture(scope="module")
def host_paths(tmp_path_factory):
    """variant -> (the child's answer, its directory); one child per variant, shared by the tests below"""
    def get(variant):
        if variant not in _children:
            name, streams, env, plain_too = VARIANTS[variant]
            tmp = str(tmp_path_factory.mktemp("completion_" + variant))
            _children[variant] = (run_child("host_paths", name, tmp, streams, plain_too, env), tmp)
        return _children[variant]
    return get


_refs = {}


def oracle_ref(oracle, path, ratio, x_s, key):
    """one stream's oracle rendering of the whole signal, computed once (the variants of a case share the signal)"""
    if key not in _refs:
        ref = oracle.get_dsp(path, fast_tanh=True)
        if ratio is not None:
            ref.SetSlimmableSize(ratio)
        ref.Reset(48000.0, sl.BLOCK)
        _refs[key] = ref.process_stream(x_s, sl.BLOCK)
    return _refs[key]


def line_of(ans, tag):
    assert len(ans["lines"]) == len(ans["order"]), (ans["order"], ans["lines"])
    return ans["lines"][ans["order"].index(tag)]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_blocking_calls_ride_one_launch(host_paths, variant):
    """The test that fails without per-command completion: 40 such calls were 40 launches by construction."""
    ans, _ = host_paths(variant)
    for tag in ("b64", "b32"):
        starts, launches, n_cmds = line_of(ans, tag)
        run = ans["runs"][tag]
        print(f"{variant} {tag}: {starts} starts, {launches} launches, {n_cmds} commands, foreign synchronize {run['t_sync'] * 1e3:.3f} ms")
        assert run["finite"] and run["peak"] > 1e-3, run
        assert (starts, n_cmds) == (1, run["commands"]), (tag, starts, n_cmds)
        assert launches <= MAX_LAUNCHES_BLOCKING, (tag, launches)
        assert run["t_sync"] < SYNC_BOUND_S, (tag, run["t_sync"])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tickets_complete_per_buffer(host_paths, variant):
    ans, _ = host_paths(variant)
    for tag in ("t64", "t48", "t480"):
        starts, launches, n_cmds = line_of(ans, tag)
        run = ans["runs"][tag]
        print(f"{variant} {tag}: {starts} starts, {launches} launches, {n_cmds} commands for {run['calls']} tickets")
        assert run["finite"] and run["peak"] > 1e-3, run
        assert (starts, n_cmds) == (1, run["commands"]), (tag, starts, n_cmds)
        assert 4 * launches <= run["calls"], (tag, launches, run["calls"])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_values(oracle, host_paths, variant):
    ans, tmp = host_paths(variant)
    name, _, _, plain_too = VARIANTS[variant]
    x = np.load(os.path.join(tmp, "x.npy"))
    for tag, run in ans["runs"].items():
        y = np.load(os.path.join(tmp, f"y_{tag}.npy"))
        T = run["frames"]
        assert y.shape[2] == T
        for s in range(ans["streams"]):
            r = oracle_ref(oracle, ans["paths"][ans["member_of"][s]], ans["ratio_of"][s], x[s], (name, ans["streams"], s))
            scale = max(1.0, float(np.max(np.abs(r[:, :T]))))
            err = float(np.max(np.abs(r[:, :T] - y[s])))
            if s in (0, ans["streams"] - 1):
                print(f"{variant} {tag} stream {s}: max|gpu - oracle| {err:.3e}, |ref|max {scale:.3f}")
            assert err <= TOL * scale, (variant, tag, s, err, scale)
        if plain_too:
            assert run["differ_from_plain"] == [], (tag, "streams that differ from persistent mode off", run["differ_from_plain"])
        if tag.startswith("t"):
            assert run["differ_from_window"] == [], (tag, "streams that differ from the device-window session", run["differ_from_window"])


def test_turns_publish_and_never_linger(oracle, tmp_path):
    """nano as tickets runs four wavefronts per stream while that is the fastest form: one such workgroup per CU
    (csrc/launch_policy.h: wr_workgroups_per_cu(.., 4, 1) == 1), so CUs + 32 streams are 32 more than fit at once: the launches take
    turns, publish every command and leave when the ring is empty"""
    torch = pytest.importorskip("torch")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus + 32
    ans = run_child("turns", "nano", str(tmp_path), n, False, {"NAM_HIP_MAX_STAGES": "4"})
    assert f"{n} workgroups as 4 wavefront(s) per stream" in ans["stderr"], "the form this stream count was chosen for"
    (starts, launches, n_cmds), = ans["lines"]
    (publishing, lingering), = ans["launch_lines"]
    print(f"turns: {n} streams, {starts} starts, {launches} launches ({publishing} publishing, {lingering} lingering), {n_cmds} commands")
    assert (starts, n_cmds) == (1, 12)
    assert publishing == launches and publishing >= 1 and lingering == 0
    x, y = np.load(os.path.join(str(tmp_path), "x.npy")), np.load(os.path.join(str(tmp_path), "y_turns.npy"))
    assert ans["runs"]["turns"]["finite"]
    for s in (0, 1, cus - 1, cus, n - 1):  # both sides of the turn boundary
        ref = oracle.get_dsp(ans["paths"][0], fast_tanh=True)
        ref.Reset(48000.0, sl.BLOCK)
        r = ref.process_stream(x[s], sl.BLOCK)
        scale = max(1.0, float(np.max(np.abs(r))))
        assert float(np.max(np.abs(r - y[s]))) <= TOL * scale, s


@pytest.mark.parametrize("name", ["a2_max", "lstm_row"])
def test_control_calls_complete_the_tickets_in_flight(tmp_path, name):
    ans = run_child("control", name, str(tmp_path), 0, False, {"NAM_HIP_MAX_STAGES": "4"})
    n = ans["streams"]
    for what, touched in (("reset", list(range(n))), ("restart", [3]), ("set_state", [7])):
        got = ans["calls"][what]
        assert got["finite"], what
        assert got["before_differ"] == [], (what, "tickets up to the call differ from the undisturbed run", got["before_differ"])
        assert got["after_untouched_differ"] == [], (what, "streams the call does not touch", got["after_untouched_differ"])
        assert got["after_touched_same"] == [], (what, "the call changed nothing on", got["after_touched_same"])
