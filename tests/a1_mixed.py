"""What tests/test_a1_mixed_loader.py, tests/test_gpu_a1_mixed.py and tools/a1_mixed_bench.py share: a SlimmableContainer of the
official WaveNet topology's tiers — feather 8 / 4, lite 12 / 6, standard 16 / 8, ordered by max_value — as ONE batch whose streams
are at mixed sizes, in persistent mode: one session of nam_a1_q_kernel through the kernels' bank path, every stream's rings in the
standard submodel's rows. The document is assembled from the three fixtures (the format: NAM/container.cpp, as
tests/linear_container.py writes it for Linear models); nothing is added to tests/golden.

Run as a program it is the child process of a test, in the pattern of tests/a2_mixed.py (whose drivers, tests/session_lengths.py's,
it uses): NAM_HIP_SESSION_STATS is read once per process, so every scenario that reads the `nam_hip session:` line runs in a process
of its own, does its bit-for-bit comparisons there, leaves its signals and outputs in .npy files for the oracle checks and prints
one JSON line."""
import json
import os
import sys

import numpy as np

import session_lengths as sl

ROOT = sl.ROOT
BLOCK = 64
FEATHER, LITE, STANDARD = 0, 1, 2  # the submodels' indices: ascending max_value
FIXTURES = ("synth_a1_feather", "synth_a1_lite", "wavenet_a1_standard")
MAX_VALUES = (0.25, 0.5, 1.0)
# ModelSpec::container_index (NAM/container.cpp:85-97): the first submodel whose max_value exceeds the ratio, else the last
RATIO = {FEATHER: 0.1, LITE: 0.4, STANDARD: 1.0}
TIERS = [STANDARD, LITE, FEATHER, LITE, STANDARD, FEATHER]  # each tier twice, the first and the last stream differ
Q, P4, P2 = "nam_a1_q_kernel", "nam_a1_p4_kernel", "nam_a1_p2_kernel"
SIDE = 20  # 64-frame buffers on each side of a transition: 1,280 frames, more than the longest ring (2 x 512 + 64 rows)
ODD = 37  # a call in front: control calls and row copies land at odd ring positions


def fixture_doc(name):
    with open(sl.model_file(name)) as f:
        return json.load(f)


def container_doc(names=FIXTURES, max_values=MAX_VALUES):
    """the container of the fixtures `names` in this order"""
    return {"version": "0.5.4", "architecture": "SlimmableContainer", "weights": [], "sample_rate": 48000,
            "config": {"submodels": [{"max_value": float(v), "model": fixture_doc(n)} for v, n in zip(max_values, names)]}}


def four_tier_doc():
    """... with the nano tier (4 / 2 channels) below feather: outside the family, the container has no residency"""
    return container_doc(("synth_a1_nano",) + FIXTURES, (0.1, 0.25, 0.5, 1.0))


def relu_doc():
    """... with feather's ReLU sibling in feather's place: another activation"""
    return container_doc(("synth_a1_feather_relu",) + FIXTURES[1:])


def load(nam, doc=None, fast_tanh=True):
    return nam.get_dsp_json(json.dumps(doc or container_doc()), fast_tanh=fast_tanh)


def assign(b, tiers, ratio=RATIO):
    """stream s of a batch whose streams are all on the last submodel to submodel tiers[s]"""
    for w in sorted(set(tiers)):
        ids = [s for s, v in enumerate(tiers) if v == w]
        if ids and w != STANDARD:
            b.SetSlimmableSize(ratio[w], ids)


def make(nam, tiers, persistent=True, model=None):
    """a batch of len(tiers) streams after Reset(prewarm), stream s on submodel tiers[s]; persistent mode is asked for last, of the
    batch as it then is"""
    b = (model or load(nam)).batch(len(tiers), BLOCK)
    b.Reset(prewarm=True)
    assign(b, tiers)
    if persistent:
        assert b.set_persistent(True), "set_persistent answered 0 on the batch at these sizes"
    return b


def make_bank(nam, tiers, persistent=True):
    """the same assignment as a bank batch: ModelBank([feather, lite, standard]), member = submodel index"""
    bank = nam.ModelBank([nam.get_dsp(sl.model_file(n), fast_tanh=True) for n in FIXTURES])
    b = bank.batch(len(tiers), BLOCK, stream_model=list(tiers))
    b.Reset(prewarm=True)
    if persistent:
        assert b.set_persistent(True)
    return b


def signal(n, T, seed):
    from signals import stream_bank
    return stream_bank(n, T, seed=seed)[:, None, :]


def _differ(a, b, streams=None):
    return [s for s in (range(a.shape[0]) if streams is None else streams) if not np.array_equal(a[s], b[s])]


def child(what, tmp):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import neuralampmodelercore_amd as nam
    nam.load_library()
    ans = {"what": what, "order": []}
    save = lambda name, a: np.save(os.path.join(tmp, name + ".npy"), a)  # noqa: E731
    n = len(TIERS)
    if what == "session":
        # the odd call (no session yet: a plain launch), then SIDE whole buffers through the mixed batch: one start, a command each
        lens = [ODD] + [BLOCK] * SIDE
        x = signal(n, sum(lens), 881)
        b = load(nam).batch(n, BLOCK)
        b.Reset(prewarm=True)
        assign(b, TIERS)
        ans["persistent"] = bool(b.set_persistent(True))
        ans["kernel"], ans["kernel_1024"] = b.kernel_name(), b.kernel_name(1024)
        y = sl.walk(b, x, lens, True)
        b.close()
        ans["order"].append("mixed")
        d = make_bank(nam, TIERS)
        ans["kernel_bank"], ans["kernel_bank_1024"] = d.kernel_name(), d.kernel_name(1024)
        yb = sl.walk(d, x, lens, True)
        d.close()
        ans["order"].append("bank")
        ans["differ_from_bank"] = _differ(y, yb)
        # the four-tier container at mixed sizes: no residency, no session — as before
        four = load(nam, four_tier_doc())
        b4 = four.batch(n, BLOCK)  # (no Reset: the answer does not depend on the state, and nothing is processed)
        b4.SetSlimmableSize(0.05, [1])
        b4.SetSlimmableSize(0.4, [2, 3])
        ans["persistent_four_tier"] = bool(b4.set_persistent(True))
        b4.close()
        ans["commands"] = SIDE
        save("x", x), save("y", y)
    elif what in ("tickets", "blocking"):
        T = 24 * BLOCK + BLOCK if what == "tickets" else SIDE * BLOCK
        x = signal(n, T, 882)
        run = (lambda b: sl.tickets(b, x, BLOCK, 8, BLOCK)) if what == "tickets" else (lambda b: sl.blocking(b, x, BLOCK))
        b = make(nam, TIERS)
        ans["kernel"] = b.kernel_name()
        y = run(b)
        ans["kernel_end"] = b.kernel_name()
        b.close()
        d = make_bank(nam, TIERS)
        ans["kernel_bank"] = d.kernel_name()
        yb = run(d)
        ans["kernel_bank_end"] = d.kernel_name()
        d.close()
        ans["order"] += ["mixed", "bank"]
        ans["differ_from_bank"] = _differ(y, yb)
        ans["commands"] = T // BLOCK
        save("x", x), save("y", y)
    elif what == "transitions":
        # [ODD, SIDE buffers] A [SIDE] B [SIDE] C [SIDE]; A: stream 1 lite -> standard; B: every lite and feather stream -> standard
        # (the batch is at one size); C: stream 0 -> feather (mixed again)
        lens = [ODD] + [BLOCK] * (4 * SIDE)
        k_a, k_b, k_c = 1 + SIDE, 1 + 2 * SIDE, 1 + 3 * SIDE
        cut = {k: ODD + (k - 1) * BLOCK for k in (k_a, k_b, k_c)}
        x = signal(n, sum(lens), 883)
        seen = {}
        narrow = [s for s, t in enumerate(TIERS) if t != STANDARD]

        def moves(b, k):
            if k == k_a:
                seen["kernel_before_a"] = b.kernel_name()
                b.SetSlimmableSize(RATIO[STANDARD], [1])
                seen["kernel_after_a"] = b.kernel_name()
            if k == k_b:
                b.SetSlimmableSize(RATIO[STANDARD], narrow)
                seen["kernel_after_b"] = b.kernel_name()
            if k == k_c:
                b.SetSlimmableSize(RATIO[FEATHER], [0])
                seen["kernel_after_c"] = b.kernel_name()

        b = make(nam, TIERS)
        y = sl.walk(b, x, lens, True, hook=moves)
        b.close()
        b = make(nam, TIERS)
        twin = sl.walk(b, x, lens, True)  # nothing happens
        b.close()
        ans.update(seen)
        # a stream equals the undisturbed twin up to the first call that names it: 1 up to A, the other narrow ones up to B, 0 up to C, 4 throughout
        T = sum(lens)
        until = {s: T for s in range(n)}
        until[1] = cut[k_a]
        for s in narrow:
            until[s] = min(until[s], cut[k_b])
        until[0] = cut[k_c]
        ans["until"] = until
        ans["differ_from_twin"] = [s for s in range(n) if not np.array_equal(y[s, :, :until[s]], twin[s, :, :until[s]])]
        # ... and a fresh stream of its new size from there on: the same streams in a fresh batch at the sizes behind the call
        fresh = {}
        tiers = list(TIERS)
        # (B names stream 1 too, which is at that size already: no move, it goes on as the standard stream A made it)
        for name, k, moved, to in (("a", k_a, [1], STANDARD), ("b", k_b, [s for s in narrow if s != 1], STANDARD), ("c", k_c, [0], FEATHER)):
            for s in moved:
                tiers[s] = to
            f = make(nam, tiers)
            ans["kernel_fresh_" + name] = f.kernel_name()
            yf = sl.walk(f, np.ascontiguousarray(x[:, :, cut[k]:]), lens[k:], True)
            f.close()
            fresh[name] = {"moved": moved, "differ": [s for s in moved if not np.array_equal(y[s, :, cut[k]:], yf[s, :, :])]}
        ans["fresh"] = fresh
        ans["order"] += ["moves", "twin", "fresh_a", "fresh_b", "fresh_c"]
        save("x", x), save("y", y)
        ans["cuts"] = [cut[k_a], cut[k_b], cut[k_c]]
    elif what == "slots":
        lens1, two, lens2 = [ODD] + [BLOCK] * SIDE, [BLOCK] * 2, [BLOCK] * SIDE
        cut = sum(lens1)
        x = signal(n, cut + sum(lens2), 884)
        x1, x2 = np.ascontiguousarray(x[:, :, :cut]), np.ascontiguousarray(x[:, :, cut:])
        # (a) restart_streams([2]) between two calls of the resident batch: nobody else notices
        b = make(nam, TIERS)
        plain = sl.walk(b, x, lens1 + lens2, True)
        b.close()
        seen = {}

        def restart(b, k):
            if k == len(lens1):
                b.restart_streams([2])
                seen["kernel_after_restart"] = b.kernel_name()

        b = make(nam, TIERS)
        yr = sl.walk(b, x, lens1 + lens2, True, hook=restart)
        b.close()
        ans["restart"] = {"who": [2], "cut": cut, "differ": _differ(plain, yr, [s for s in range(n) if s != 2]),
                          "named_before_equal": bool(np.array_equal(plain[2, :, :cut], yr[2, :, :cut])), **seen}
        save("x", x), save("y_restart", yr)
        # (b) get_stream_state(3), two buffers, set_stream_state(3, blob): the same two buffers give the same bits again
        src = 3
        assert TIERS[src] == LITE
        b = make(nam, TIERS)
        ans["kernel"] = b.kernel_name()
        sl.walk(b, x1, lens1, True)
        blob = b.get_stream_state(src)
        ans["kernel_after_get"] = b.kernel_name()
        x_two = np.ascontiguousarray(x2[:, :, :2 * BLOCK])
        first = sl.walk(b, x_two, two, True)
        b.set_stream_state(src, blob)
        ans["kernel_after_set"] = b.kernel_name()
        again = sl.walk(b, x_two, two, True)
        ans["rewind_repeats"] = bool(np.array_equal(first[src], again[src]))
        b.close()
        # (c) the blob of the resident stream against the same stream's with persistent mode off, at the same point
        b = make(nam, TIERS)
        sl.walk(b, x1, lens1, True)
        blob_on = b.get_stream_state(src)
        b.set_persistent(False)
        blob_off = b.get_stream_state(src)
        b.close()
        ans["blob_bytes"] = [len(blob_on), len(blob_off)]
        ans["blob_identical"] = blob_on == blob_off and blob_on == blob
        # (d) ... into an all-lite batch, which goes on with the source's bits (`plain` is the source, uninterrupted). A container
        # batch whose streams are all on ONE narrow size has no session, as ever; what its launches run depends on their length.
        # Launches of four buffers run nam_a1_q_kernel, the kernel the source's session runs: bit for bit. Launches of one buffer
        # run nam_a1_mfma_kernel under AUTO (another summation order: last bits differ, measured 6.0e-8): within the oracle bound.
        xd = signal(4, sum(lens2), 885)
        xd[2] = x2[src]
        for how, frames in (("q", 4 * BLOCK), ("mfma", BLOCK)):
            d = make(nam, [LITE] * 4, persistent=False)
            ans["kernel_dst_" + how] = d.kernel_name(frames)
            ans["blob_bytes_all_lite"] = len(d.get_stream_state(2))
            d.set_stream_state(2, blob_on)
            yd = sl.walk(d, xd, [frames] * (sum(lens2) // frames), False)
            d.close()
            ans["dst_continues_source_" + how] = bool(np.array_equal(yd[2], plain[src, :, cut:]))
            ans["dst_max_diff_" + how] = float(np.max(np.abs(yd[2] - plain[src, :, cut:])))
            save("y_dst_" + how, yd[2])
        ans["order"] += ["plain", "restart", "rewind", "blobs", "dst"]
    elif what == "guard":
        # a 32-frame call between whole buffers ends the session, runs as ONE plain launch of the bank form over every stream, and
        # the next whole buffer starts the session again
        lens = [64, 64, 32, 64, 64]
        x = signal(n, sum(lens), 886)
        b = make(nam, TIERS)
        ans["kernel"], ans["kernel_32"] = b.kernel_name(), b.kernel_name(32)
        y = sl.walk(b, x, lens, True)
        b.close()
        d = make_bank(nam, TIERS)
        ans["kernel_bank_32"] = d.kernel_name(32)
        d.close()
        ans["order"].append("guard")
        ans["commands"] = 4
        save("x", x), save("y", y)
    else:
        raise SystemExit("a1_mixed.py: unknown scenario " + what)
    print("a1_mixed: " + json.dumps(ans))


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
