"""The child processes of tests/test_gpu_session_completion.py: NAM_HIP_SESSION_STATS is read once per process, and the
`nam_hip session:` line is said when a batch is destroyed, so every case runs here, in a process of its own, on the cases of
tests/session_lengths.py (imported, not copied). One process feeds one case every host pattern — blocking calls of 64 and of 32
frames, three ticket feeds —, each on a fresh batch after Reset(prewarm) and each from the start of ONE signal, so the parent
holds every run against one oracle rendering by prefix; then the same feeds with persistent mode off and through device-window
sessions for the bit-for-bit comparisons, done here. It prints one JSON line; the runs' outputs go to .npy files."""
import json
import os
import sys
import time

import numpy as np

import session_lengths as sl

BLOCK = sl.BLOCK
N_BLOCKING = 40
# (name, [call lengths], depth): 48 buffers of 64 frames four deep; 48 of 48 frames sixteen deep; a 480-frame ticket between 64-frame ones
TICKET_FEEDS = [("t64", [64] * 48, 4), ("t48", [48] * 48, 16), ("t480", [64] * 8 + [480] + [64] * 8, 4)]
T_SIGNAL = max([N_BLOCKING * 64] + [sum(lens) for _, lens, _ in TICKET_FEEDS])


def make_case(nam, name, tmp, streams):
    c = sl.Case(nam, name, tmp)
    if streams:  # (another stream count than the shared case's: one stream = one workgroup, the first through a command is the last)
        c.n = streams
        c.ratio_of = [c.ratio_of[s % len(c.ratio_of)] for s in range(streams)]
        c.member_of = [c.member_of[s % len(c.member_of)] for s in range(streams)]
    return c


def blocking(b, x, frames):
    """40 blocking process() calls back to back; a foreign device-wide synchronize after call 20 (timed), one 2 ms pause after call 24"""
    import torch
    ys, t_sync = [], None
    for k in range(N_BLOCKING):
        ys.append(b.process(x[:, :, k * frames:(k + 1) * frames]))
        if k + 1 == 20:
            t0 = time.perf_counter()
            torch.cuda.synchronize()  # (a launch that lingers for the next call holds the device for the linger at most)
            t_sync = time.perf_counter() - t0
        if k + 1 == 24:
            time.sleep(0.002)  # (the launch gives up and leaves; the next call starts one again)
    return np.concatenate(ys, axis=2), t_sync


def tickets(b, x, lens, depth, hook=None):
    """the calls of `lens` as tickets, `depth` in flight; hook(b, k): before ticket k is submitted"""
    ys, inflight, at = [], [], 0
    for k, m in enumerate(lens):
        if hook:
            hook(b, k)
        if len(inflight) == depth:
            ys.append(b.wait(inflight.pop(0)))
        inflight.append(b.submit(x[:, :, at:at + m]))
        at += m
    while inflight:
        ys.append(b.wait(inflight.pop(0)))
    return np.concatenate(ys, axis=2)


def differ(a, b):
    return [s for s in range(a.shape[0]) if not np.array_equal(a[s], b[s])]


def child_host_paths(nam, name, tmp, streams, plain_too):
    """ans["order"]: the batches in the order of their `nam_hip session:` lines"""
    c = make_case(nam, name, tmp, streams)
    x = c.signal(seed=981, T=T_SIGNAL)
    np.save(os.path.join(tmp, "x.npy"), x)
    ans = {"case": name, "streams": c.n, "order": [], "paths": c.paths, "member_of": c.member_of, "ratio_of": c.ratio_of, "runs": {}}

    def run(tag, persistent, drive):
        b = c.make(persistent)
        y = drive(b)
        b.close()
        extra = None
        if isinstance(y, tuple):
            y, extra = y
        if persistent:
            ans["order"].append(tag)
        return y, extra

    ys = {}
    for frames in (64, 32):
        tag = f"b{frames}"
        ys[tag], t_sync = run(tag, True, lambda b: blocking(b, x, frames))
        ans["runs"][tag] = {"commands": N_BLOCKING, "calls": N_BLOCKING, "frames": N_BLOCKING * frames, "t_sync": t_sync}
    for tag, lens, depth in TICKET_FEEDS:
        ys[tag], _ = run(tag, True, lambda b: tickets(b, x, lens, depth))
        ans["runs"][tag] = {"commands": sl.commands(lens), "calls": len(lens), "frames": sum(lens)}
    for tag, y in ys.items():
        np.save(os.path.join(tmp, f"y_{tag}.npy"), y)
        ans["runs"][tag].update(finite=bool(np.isfinite(y).all()), peak=float(np.abs(y).max()))
    # the ticket runs against device-window sessions of the same batch fed the same call lengths: the same wavefront form (the
    # parent pins NAM_HIP_MAX_STAGES for the whole process), so the same bits
    for tag, lens, _ in TICKET_FEEDS:
        w, _ = run(tag + "_window", True, lambda b: sl.walk(b, np.ascontiguousarray(x[:, :, :sum(lens)]), lens, True))
        ans["runs"][tag]["differ_from_window"] = differ(ys[tag], w)
    if plain_too:  # the forms that are bit-equal to persistent mode off (profiles/session_lengths/README.md)
        for frames in (64, 32):
            p, _ = run("", False, lambda b: blocking(b, x, frames))
            ans["runs"][f"b{frames}"]["differ_from_plain"] = differ(ys[f"b{frames}"], p)
        for tag, lens, depth in TICKET_FEEDS:
            p, _ = run("", False, lambda b: tickets(b, x, lens, depth))
            ans["runs"][tag]["differ_from_plain"] = differ(ys[tag], p)
    return ans


def child_turns(nam, name, tmp, streams):
    """more streams than the chip holds at once in the form the launch takes: tickets four deep for twelve buffers"""
    c = make_case(nam, name, tmp, streams)
    lens = [64] * 12
    x = c.signal(seed=982, T=sum(lens))
    b = c.make(True)
    y = tickets(b, x, lens, 4)
    b.close()
    np.save(os.path.join(tmp, "x.npy"), x)
    np.save(os.path.join(tmp, "y_turns.npy"), y)
    return {"case": name, "streams": c.n, "order": ["turns"], "paths": c.paths, "member_of": c.member_of, "ratio_of": c.ratio_of,
            "runs": {"turns": {"commands": 12, "calls": 12, "finite": bool(np.isfinite(y).all()), "peak": float(np.abs(y).max())}}}


def child_control(nam, name, tmp):
    """Reset, restart_streams([3]) and set_stream_state with three tickets in flight: the tickets complete, their outputs stay
    waitable and equal the undisturbed run's; what follows the call is what the call makes of the batch"""
    c = make_case(nam, name, tmp, 0)
    lens = [64] * 10
    x = c.signal(seed=983, T=sum(lens))
    depth, at_k = 3, 6  # the call comes before ticket 6 is submitted: tickets 3, 4, 5 are in flight
    plain = tickets(c.make(True), x, lens, depth)
    ans = {"case": name, "streams": c.n, "calls": {}}
    blob = {}

    def hook_of(what):
        def hook(b, k):
            if k == 0:
                blob["state"] = b.get_stream_state(3)
            if k == at_k:
                if what == "reset":
                    b.Reset(prewarm=True)
                elif what == "restart":
                    b.restart_streams([3])
                else:
                    b.set_stream_state(7, blob["state"])
        return hook

    upto = at_k * 64
    for what in ("reset", "restart", "set_state"):
        b = c.make(True)
        y = tickets(b, x, lens, depth, hook=hook_of(what))
        b.close()
        touched = {"reset": list(range(c.n)), "restart": [3], "set_state": [7]}[what]
        ans["calls"][what] = {
            "finite": bool(np.isfinite(y).all()),
            "before_differ": differ(y[:, :, :upto], plain[:, :, :upto]),  # every ticket up to the call, the three in flight included
            "after_untouched_differ": [s for s in differ(y[:, :, upto:], plain[:, :, upto:]) if s not in touched],
            "after_touched_same": [s for s in touched if np.array_equal(y[s, :, upto:], plain[s, :, upto:])],
        }
    return ans


def main(what, name, tmp, streams, plain_too):
    sys.path[:0] = [os.path.join(sl.ROOT, "tests"), sl.ROOT]
    import neuralampmodelercore_amd as nam
    nam.load_library()
    if what == "host_paths":
        ans = child_host_paths(nam, name, tmp, streams, plain_too)
    elif what == "turns":
        ans = child_turns(nam, name, tmp, streams)
    else:
        ans = child_control(nam, name, tmp)
    ans["what"] = what
    print("session_completion: " + json.dumps(ans))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5] == "1")
