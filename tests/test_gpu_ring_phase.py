"""Ring-phase sweep: every pipelined kernel started at every position of every ring.

The kernels keep their convolution history in rings whose addressing depends on the write position (kernel_a1_q.hip: the mirror's
second store in a ring's first 15 rows and over its end, tap windows that reach into the mirror, the HBM rings' scalar-offset
addressing with its per-lane fallback at a ring's end, ring_to_lds / lds_to_ring at a launch's edges; kernel_kq.hip: the windows'
tails and the resident rings; kernel_wn_reg.hip: the history shift by a call's frames). Sessions of 64-frame buffers only reach
the positions 64 k mod R. Here ONE continuous stream per case goes through a call pattern of tests/ring_phase.py —
  session: cycles of one ragged call (a plain launch of the one-buffer kernel, which ends the session) and a burst of seven
           session commands, 449 frames per cycle, as many cycles as the longest ring has rows: a burst, i.e. a resident launch
           with ring_to_lds, the mirror's rebuild and lds_to_ring, starts at every position of every ring;
  launch:  plain launches of 128 + r frames, r in 1 .. 63: the non-session instantiation with a ragged last block, started at
           every position of every LDS-resident ring
(tests/test_ring_phase_schedule.py proves the coverage on the CPU) — three streams, the whole input and output resident on the
device, every call at its running offset; every stream over the whole length against the CPU oracle, with the soak's criterion
(tests/test_gpu_soak.py: 5e-5 * max(1, max|ref|) with fast tanh, 1e-4 * ... with libm's). A mismatch is reported as a place: the
stream, the first bad frame, the cycle it lies in and where every ring stood in that cycle, with the class of the position.
The kernel names are asserted before the first burst, in mid-sweep and at the end: a sweep that drifts onto another kernel fails.

Measured on an MI355X (profiles/ring_phase/README.md): 0.1 - 3.3 s per case, 13 s for the twelve."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ring_phase as rp
from bank_models import write_a2, write_standard
from conftest import model_path
from signals import stream_bank

pytestmark = pytest.mark.gpu

N_STREAMS = 3
SEED = 7321

# model: a fixture's name, or "bank_a1" / "bank_a2": three members, one per stream
# kernel: None = AUTO, "il" = set_kernel(KERNEL_A1_IL)
# session / ragged / launch: what kernel_name() (a session command), kernel_name(1) and kernel_name(128 + r) must say
CASES = {
    "a1_q_session": dict(model="wavenet_a1_standard", family="a1", mode="session", session="nam_a1_q_kernel", ragged="nam_a1_mfma_kernel",
                         launch="nam_a1_mfma_kernel"),
    "a1_q_session_il": dict(model="wavenet_a1_standard", family="a1", mode="session", kernel="il", session="nam_a1_q_kernel",
                            ragged="nam_a1_p2_kernel", launch="nam_a1_q_kernel"),
    "a1_q_session_libm": dict(model="wavenet_a1_standard", family="a1", mode="session", fast_tanh=False, session="nam_a1_q_kernel",
                              ragged="nam_a1_mfma_kernel", launch="nam_a1_mfma_kernel"),
    "a1_q_launch": dict(model="wavenet_a1_standard", family="a1", mode="launch", kernel="il", ragged="nam_a1_p2_kernel", launch="nam_a1_q_kernel"),
    "a1_lite_padded": dict(model="synth_a1_lite", family="a1", mode="session", session="nam_a1_q_kernel", ragged="nam_a1_mfma_kernel",
                           launch="nam_a1_mfma_kernel"),
    "a1_p4_session": dict(model="synth_a1_feather_relu", family="a1", mode="session", session="nam_a1_p4_kernel", ragged="nam_a1_mfma_kernel",
                          launch="nam_a1_mfma_kernel"),
    "a1_p4_launch": dict(model="synth_a1_feather_relu", family="a1", mode="launch", kernel="il", ragged="nam_a1_p2_kernel", launch="nam_a1_p4_kernel"),
    "a1_bank_session": dict(model="bank_a1", family="a1", mode="session", session="nam_a1_q_kernel", ragged="nam_a1_p2_kernel",
                            launch="nam_a1_q_kernel"),
    "a2_kq_session": dict(model="A2", family="a2", mode="session", session="nam_kq_kernel", ragged="nam_kt_mfma_kernel", launch="nam_kq_kernel"),
    "a2_kq_launch": dict(model="A2", family="a2", mode="launch", ragged="nam_kt_mfma_kernel", launch="nam_kq_kernel"),
    "a2_bank_session": dict(model="bank_a2", family="a2", mode="session", session="nam_kq_kernel", ragged="nam_kt_mfma_kernel",
                            launch="nam_kq_kernel"),
    # (every ragged length: the register kernel shifts its history down by the call's frames)
    "wn_reg_session": dict(model="wavenet_a2_max", family="wn_reg", mode="session", r=range(1, rp.BLOCK), session="nam_wn_reg_kernel",
                           ragged="nam_wn_reg_kernel", launch="nam_wn_reg_kernel"),
}


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    """the banks' members: the committed fixture and two seeded models of its topology (tests/bank_models.py)"""
    d = tmp_path_factory.mktemp("ring_phase_members")
    a1 = [model_path("wavenet_a1_standard")]
    a2 = [model_path("A2")]
    for seed in (101, 102):
        a1.append(str(d / f"standard_{seed}.nam"))
        write_standard(a1[-1], seed)
    for seed in (401, 402):
        a2.append(str(d / f"a2_{seed}.nam"))
        write_a2(a2[-1], seed)
    return {"bank_a1": a1, "bank_a2": a2}


@pytest.fixture(scope="module")
def renderings():
    """oracle renderings, shared by the cases with the same model, tanh and signal (never modified): (path, fast_tanh, stream, frames) -> y"""
    return {}


def _oracle(oracle, renderings, paths, fast_tanh, x):
    """x [streams, N] through the oracle of each stream's model, 64-frame blocks"""
    def one(s):
        ref = oracle.get_dsp(paths[s], fast_tanh=fast_tanh)
        ref.Reset(48000.0, rp.BLOCK)
        y = ref.process_stream(x[s], rp.BLOCK)[0]
        y.setflags(write=False)
        return y

    keys = [(paths[s], fast_tanh, s, x.shape[1]) for s in range(x.shape[0])]
    todo = [s for s in range(x.shape[0]) if keys[s] not in renderings]
    with ThreadPoolExecutor(max_workers=max(len(todo), 1)) as pool:  # (the C side runs without the interpreter's lock)
        for s, y in zip(todo, pool.map(one, todo)):
            renderings[keys[s]] = y
    return [renderings[k] for k in keys]


@pytest.mark.parametrize("case", list(CASES))
def test_ring_phase_sweep(nam_lib, oracle, members, renderings, case):
    torch = pytest.importorskip("torch")
    nam = nam_lib
    c = CASES[case]
    fast_tanh = c.get("fast_tanh", True)
    session = c["mode"] == "session"
    paths = members[c["model"]] if c["model"] in members else [model_path(c["model"])] * N_STREAMS
    rings = rp.ring_lengths(c["family"], paths[0])
    calls = rp.schedule(rings, c["mode"], r=c["r"]) if "r" in c else rp.schedule(rings, c["mode"])
    off = rp.offsets(calls)
    N = int(off[-1])
    x = stream_bank(N_STREAMS, N, seed=SEED)

    models = [nam.get_dsp(p, fast_tanh=fast_tanh) for p in dict.fromkeys(paths)]
    max_frames = rp.BLOCK if session else 3 * rp.BLOCK
    if c["model"] in members:
        bank = nam.ModelBank(models)
        b = bank.batch(N_STREAMS, max_frames, stream_model=list(range(N_STREAMS)))
        assert [b.stream_model(s) for s in range(N_STREAMS)] == list(range(N_STREAMS))
    else:
        b = models[0].batch(N_STREAMS, max_frames)
    if c.get("kernel") == "il":
        b.set_kernel(nam.KERNEL_A1_IL)
    if session:
        assert b.set_persistent(True)
    # what has gone through the rings when the signal starts: the prewarm's silence, whole buffers of max_frames
    pre = models[0].GetPrewarmSamples()
    frames_before = (pre + max_frames - 1) // max_frames * max_frames

    def names():
        got = {"ragged": b.kernel_name(1), "launch": {b.kernel_name(2 * rp.BLOCK + r) for r in (1, 33, 63)}}
        want = {"ragged": c["ragged"], "launch": {c["launch"]}}
        if session:
            got["session"], want["session"] = b.kernel_name(), c["session"]
        return got, want

    b.Reset(prewarm=True)
    xd = torch.from_numpy(x[:, None, :]).cuda()
    yd = torch.zeros_like(xd)
    torch.cuda.synchronize()
    got, want = names()
    assert got == want, f"{case}: before the sweep"
    t0 = time.perf_counter()
    heads = [i for i, k in enumerate(calls) if k[0] != "session"]  # a cycle starts with its ragged call (launch mode: is one launch)
    cycle, mid = -1, len(heads) // 2
    for i, (kind, n) in enumerate(calls):
        if kind != "session":
            cycle += 1
            in_burst = 0
        b.process_device(xd.data_ptr() + int(off[i]) * 4, yd.data_ptr() + int(off[i]) * 4, n, N)
        if kind == "session":
            in_burst += 1
        if cycle % 64 == 63 and in_burst == (3 if session else 0):
            b.flush()  # the host waits in mid-burst; the session goes on
            if not session:
                b.synchronize()
        if cycle == mid and (i + 1 == len(calls) or calls[i + 1][0] != "session"):
            got, want = names()
            assert got == want, f"{case}: in mid-sweep (cycle {cycle})"
    b.flush()
    b.synchronize()
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    got, want = names()
    assert got == want, f"{case}: after the sweep"
    y = yd.cpu().numpy()[:, 0, :]
    b.close()
    assert np.isfinite(y).all()

    t0 = time.perf_counter()
    refs = _oracle(oracle, renderings, paths, fast_tanh, x)
    t_cpu = time.perf_counter() - t0
    tol = 5e-5 if fast_tanh else 1e-4
    worst = []
    for s in range(N_STREAMS):
        d = np.abs(refs[s] - y[s])
        worst.append((float(d.max()), tol * max(1.0, float(np.max(np.abs(refs[s]))))))
    print(f"{case}: {len(calls)} calls in {len(heads)} cycles, {N} frames ({N / 48000.0:.2f} s of audio), {frames_before} frames of prewarm; "
          f"device {t_gpu:.2f} s, oracle {t_cpu:.2f} s; max |y - oracle| per stream "
          + ", ".join(f"{e:.3e} (bound {bnd:.1e})" for e, bnd in worst))
    for s in range(N_STREAMS):
        d = np.abs(refs[s] - y[s])
        bound = worst[s][1]
        bad = np.flatnonzero(d > bound)
        if bad.size:
            cyc = np.unique(rp.cycles_of(calls, bad))
            print(f"{case}: stream {s}: bad frames in cycles {cyc.tolist()}")
            raise AssertionError(
                f"{case}: stream {s} differs from its oracle in {bad.size} frames of {cyc.size} cycles (the first: {cyc[:16].tolist()}); max error "
                f"{float(d.max()):.3e} at frame {int(d.argmax())}, bound {bound:.1e}; first bad frame {int(bad[0])}, error {float(d[bad[0]]):.3e}\n"
                + rp.describe(rings, calls, frames_before, int(bad[0]), taps=c["family"] == "a1"))
