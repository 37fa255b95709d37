"""What tests/test_gpu_a2_mixed.py and tools/a2_mixed_bench.py share: A2.nam (A2-Lite below ratio 0.5, A2-Full from there) as ONE
batch whose streams are at mixed sizes, in persistent mode — one session of nam_kq_kernel, the Lite streams zero-padded next to the
Full ones. Run as a program it is the child process of a test, in the pattern of tests/session_lengths.py (whose
drivers it uses): NAM_HIP_SESSION_STATS is read once per process, so every scenario that reads the `nam_hip session:` line runs in a
process of its own, does its bit-for-bit comparisons there, leaves its signals and outputs in .npy files for the oracle checks
and prints one JSON line."""
import json
import os
import sys

import numpy as np

import session_lengths as sl

ROOT = sl.ROOT
MODEL = sl.model_file("A2")
BLOCK = 64
RATIOS = [1.0, 0.0, 0.4, 0.7, 0.2, 0.9]  # test_gpu_parity.py: test_container_mixed_submodels_per_stream
LITE, FULL = 0.0, 1.0
KQ, WR = "nam_kq_kernel", "nam_wn_reg_kernel"
SIDE = 38  # 64-frame buffers on each side of a transition: 2,432 frames, twice the longest reach (5 x 239) and a buffer more
ODD = 17  # a call in front of a transition: the control call lands at odd ring positions
EPISODE = 40  # buffers a stream stays at its other size in the long variant


def is_lite(ratio):
    return ratio < 0.5


def make(nam, ratios, persistent=True, order="sizes_first"):
    """a batch of len(ratios) streams after Reset(prewarm), stream s at ratios[s]; `order`: whether the mode is switched on after
    the sizes are set (the batch is mixed when it is asked) or before (the size changes mix a persistent batch)"""
    model = nam.get_dsp(MODEL, fast_tanh=True)
    b = model.batch(len(ratios), BLOCK)
    if persistent and order == "mode_first":
        assert b.set_persistent(True)
    b.Reset(prewarm=True)
    for r in sorted(set(ratios)):
        b.SetSlimmableSize(r, [s for s, v in enumerate(ratios) if v == r])
    if persistent and order == "sizes_first":
        assert b.set_persistent(True), "set_persistent answered 0 on the batch at these sizes"
    return b


def signal(n, T, seed):
    from signals import stream_bank
    return stream_bank(n, T, seed=seed)[:, None, :]


def _same(a, b):
    return [s for s in range(a.shape[0]) if not np.array_equal(a[s], b[s])]


def child(what, tmp):
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import neuralampmodelercore_amd as nam
    nam.load_library()
    ans = {"what": what, "order": []}
    save = lambda name, a: np.save(os.path.join(tmp, name + ".npy"), a)  # noqa: E731
    n = len(RATIOS)
    if what == "session":
        # 2 x SIDE whole buffers through the mixed batch: one start, one command per buffer
        lens = [BLOCK] * (2 * SIDE)
        x = signal(n, sum(lens), 991)
        b = make(nam, RATIOS)
        ans["persistent"] = True  # (make asserted set_persistent's answer)
        ans["kernel"], ans["kernel_1024"] = b.kernel_name(), b.kernel_name(1024)
        y = sl.walk(b, x, lens, True)
        b.close()
        ans["order"].append("session")
        ans["commands"] = len(lens)
        save("x", x), save("y", y)
    elif what == "continuity":
        all_lite = [LITE] * n
        named = 2
        lens = [BLOCK] * SIDE + [ODD] + [BLOCK] * SIDE
        cut = SIDE * BLOCK + ODD
        x = signal(n, SIDE * BLOCK + ODD + EPISODE * BLOCK + ODD + SIDE * BLOCK, 992)
        xa = np.ascontiguousarray(x[:, :, :sum(lens)])
        # run A: all-Lite, nothing happens
        b = make(nam, all_lite, order="mode_first")
        ans["kernel_all_lite"] = b.kernel_name()
        ya = sl.walk(b, xa, lens, True)
        b.close()
        # run B: between two calls stream `named` goes to Full and back, no process call in between
        seen = {}

        def there_and_back(b, k):
            if k == SIDE + 1:
                b.SetSlimmableSize(FULL, [named])
                seen["kernel_mixed"] = b.kernel_name()
                b.SetSlimmableSize(LITE, [named])
                seen["kernel_after"] = b.kernel_name()

        b = make(nam, all_lite, order="mode_first")
        yb = sl.walk(b, xa, lens, True, hook=there_and_back)
        b.close()
        ans["there_and_back"] = {"differ": [s for s in _same(ya, yb) if s != named], "named_before_equal": bool(np.array_equal(ya[named, :, :cut], yb[named, :, :cut])),
                                 "named_after_differs": not np.array_equal(ya[named, :, cut:], yb[named, :, cut:]), **seen}
        # run C: the episode spans EPISODE buffers (and ends behind another odd call, which the mixed session hands to a plain launch)
        lens_c = [BLOCK] * SIDE + [ODD] + [BLOCK] * EPISODE + [ODD] + [BLOCK] * SIDE
        k_in, k_out = SIDE + 1, SIDE + 1 + EPISODE + 1
        seen_c = {}

        def episode(b, k):
            if k == k_in:
                b.SetSlimmableSize(FULL, [named])
                seen_c["kernel_in"] = b.kernel_name()
            if k == k_out:
                seen_c["kernel_episode_end"] = b.kernel_name()
                b.SetSlimmableSize(LITE, [named])
                seen_c["kernel_out"] = b.kernel_name()

        b = make(nam, all_lite, order="mode_first")
        yc = sl.walk(b, x, lens_c, True, hook=episode)
        b.close()
        ans["episode"] = {"cuts": [cut, cut + EPISODE * BLOCK + ODD], "named": named, **seen_c}
        ans["order"] += ["all_lite", "there_and_back", "episode"]
        save("x", x), save("ya", ya), save("yb", yb), save("yc", yc)
    elif what == "slots":
        lens1, lens2 = [BLOCK] * SIDE + [ODD], [BLOCK] * SIDE
        cut = sum(lens1)
        x = signal(n, cut + sum(lens2), 993)
        src = 1  # a Lite stream, living padded
        assert is_lite(RATIOS[src])
        # (a) its state out of the mixed batch ...
        b = make(nam, RATIOS)
        ans["kernel"] = b.kernel_name()
        y1 = sl.walk(b, np.ascontiguousarray(x[:, :, :cut]), lens1, True)
        blob = b.get_stream_state(src)
        ans["blob_bytes_mixed"] = len(blob)
        y2 = sl.walk(b, np.ascontiguousarray(x[:, :, cut:]), lens2, True)  # (the source itself goes on undisturbed)
        b.close()
        save("x", x), save("y_src", np.concatenate([y1, y2], axis=2))
        # ... into all-Lite batches of another stream count, at two different slots: that batch's own kernel goes on from it
        outs = []
        for slot in (2, 0):
            d = make(nam, [LITE] * 4, order="mode_first")
            ans["kernel_dst"] = d.kernel_name()
            ans["blob_bytes_all_lite"] = d.stream_state_size(slot) if hasattr(d, "stream_state_size") else len(d.get_stream_state(slot))
            d.set_stream_state(slot, blob)
            xd = signal(4, sum(lens2), 994)
            xd[slot] = x[src, :, cut:]
            outs.append(sl.walk(d, xd, lens2, True)[slot])
            # and a blob taken from the all-Lite batch goes back into a padded slot of a mixed one (checked by the parent: continuity)
            d.close()
        ans["dst_slots_equal"] = bool(np.array_equal(outs[0], outs[1]))
        save("y_dst", outs[0])
        # (b) restart_streams while the batch is mixed: a Lite and a Full stream; everybody else does not notice
        who = [1, 3]
        b = make(nam, RATIOS)
        plain = sl.walk(b, x, lens1 + lens2, True)
        b.close()
        seen = {}

        def restart(b, k):
            if k == len(lens1):
                b.restart_streams(who)
                seen["kernel_after_restart"] = b.kernel_name()

        b = make(nam, RATIOS)
        yr = sl.walk(b, x, lens1 + lens2, True, hook=restart)
        b.close()
        ans["restart"] = {"who": who, "cut": cut, "differ": [s for s in _same(plain, yr) if s not in who],
                          "named_before_equal": all(bool(np.array_equal(plain[s, :, :cut], yr[s, :, :cut])) for s in who), **seen}
        save("y_restart", yr)
        # (c) a Lite blob from an all-Lite batch into a padded slot of the mixed batch (set transcodes on the way in)
        a = make(nam, [LITE] * 4, order="mode_first")
        xa = signal(4, cut, 995)
        sl.walk(a, xa, lens1, True)
        blob_a = a.get_stream_state(3)
        a.close()
        b = make(nam, RATIOS)
        b.set_stream_state(4, blob_a)  # stream 4 is Lite in RATIOS
        ans["kernel_after_set"] = b.kernel_name()
        xb = signal(n, sum(lens2), 996)
        ys = sl.walk(b, xb, lens2, True)
        b.close()
        save("x_set", np.concatenate([xa[3], xb[4]], axis=1)), save("y_set", ys[4])
        ans["set_cut"] = cut
        ans["order"] += ["src", "dst2", "dst0", "plain", "restart", "all_lite", "set"]
    elif what in ("tickets", "blocking"):
        T = 24 * BLOCK + BLOCK if what == "tickets" else 40 * BLOCK
        x = signal(n, T, 997)
        b = make(nam, RATIOS)
        ans["kernel"] = b.kernel_name()
        y = sl.tickets(b, x, BLOCK, 8, BLOCK) if what == "tickets" else sl.blocking(b, x, BLOCK)
        ans["kernel_end"] = b.kernel_name()
        b.close()
        ans["order"].append(what)
        ans["commands"] = T // BLOCK
        save("x", x), save("y", y)
    else:
        raise SystemExit("a2_mixed.py: unknown scenario " + what)
    print("a2_mixed: " + json.dumps(ans))


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
