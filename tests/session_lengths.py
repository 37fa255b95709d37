"""What tests/test_gpu_session_lengths.py and tools/session_lengths_bench.py share: the cases (a batch of a fixture, a bank or a
mixed-width batch on one of the session kernels that take a frame count per command), the fixed schedule of call lengths, and the
drivers that feed it — calls walking one device window, every call on one buffer with a flush in between, blocking host calls,
tickets. Run as a program it is the child process of a test: NAM_HIP_SESSION_STATS is read once per process, so every case that
reads the `nam_hip session:` line runs in a process of its own, does its bit-for-bit comparisons there, leaves the persistent
run's output in an .npy for the oracle check and prints one JSON line."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
BLOCK = 64

# partial commands first, last and between whole ones; calls below and above 64 in both directions; the sum (1,375) is odd, so
# every repetition starts at other ring positions
LENS = [64, 1, 63, 17, 47, 32, 32, 48, 96, 120, 480, 5, 64, 59, 240, 7]
MAX_FRAMES = max(LENS)

WR, ROW, WIDE = "nam_wn_reg_kernel", "nam_lstm_row_kernel", "nam_lstm_wide_kernel"
# name: (kernel, streams). 13 LSTM streams: the row kernel's last wavefront holds one stream of four
CASES = {
    "nano": (WR, 12),
    "a2_max": (WR, 12),
    "slimmable_two_widths": (WR, 12),
    "nano_bank3": (WR, 12),
    "lstm_row": (ROW, 13),
    "lstm_wide": (WIDE, 12),
    "lstm_bank2": (ROW, 12),
}
SLIM_RATIOS = (0.0, 1.0)  # stream s runs SLIM_RATIOS[s % 2]


def commands(lens):
    """session commands of a list of calls: ceil(n / 64) each"""
    return sum((n + BLOCK - 1) // BLOCK for n in lens)


def model_file(name):
    return os.path.join(MODELS, name + ".nam")


def longest_ring(path):
    """(K - 1) * dilation + 64 of the layer that looks back furthest (0 for a model without dilations: an LSTM)"""
    def walk(node):
        best = 0
        if isinstance(node, dict):
            if "dilations" in node:
                k = node.get("kernel_size", 1)
                ks = k if isinstance(k, list) else [k] * len(node["dilations"])
                best = max([(kk - 1) * d + BLOCK for kk, d in zip(ks, node["dilations"])] + [0])
            for v in node.values():
                best = max(best, walk(v))
        elif isinstance(node, list):
            for v in node:
                best = max(best, walk(v))
        return best
    with open(path) as f:
        return walk(json.load(f))


def schedule(ring):
    """LENS repeated until the total exceeds twice the longest history ring"""
    lens = list(LENS)
    while sum(lens) <= 2 * ring:
        lens += LENS
    return lens


class Case:
    """paths: the member files; member_of / ratio_of: per stream (ratio None = not slimmable); make(): a fresh batch"""

    def __init__(self, nam, name, tmp):
        from bank_models import write_lstm
        from bank_wr_models import NANO_SEEDS, write_nano
        self.name, (self.kernel, self.n) = name, CASES[name]
        self.ratio_of = [None] * self.n
        self.member_of = [0] * self.n
        if name in ("nano", "a2_max", "lstm_row", "lstm_wide", "slimmable_two_widths"):
            fixture = {"nano": "synth_a1_nano", "a2_max": "wavenet_a2_max", "lstm_row": "lstm", "lstm_wide": "synth_lstm_h18x2",
                       "slimmable_two_widths": "slimmable_wavenet"}[name]
            self.paths = [model_file(fixture)]
            if name == "slimmable_two_widths":
                self.ratio_of = [SLIM_RATIOS[s % 2] for s in range(self.n)]
        elif name == "nano_bank3":
            self.paths = [os.path.join(tmp, f"nano_{seed}.nam") for seed in NANO_SEEDS[:3]]
            for p, seed in zip(self.paths, NANO_SEEDS[:3]):
                write_nano(p, seed)
            self.member_of = [s % 3 for s in range(self.n)]
        else:
            self.paths = [model_file("lstm"), os.path.join(tmp, "lstm_771.nam")]
            write_lstm(self.paths[1], 771, num_layers=1, input_size=1, hidden=3, out_channels=1)
            self.member_of = [s % 2 for s in range(self.n)]
        self.models = [nam.get_dsp(p, fast_tanh=True) for p in self.paths]
        self.bank = nam.ModelBank(self.models) if len(self.models) > 1 else None
        self.lens = schedule(max(longest_ring(p) for p in self.paths))
        self.T = sum(self.lens)

    def signal(self, seed=977, T=None):
        from signals import stream_bank
        return stream_bank(self.n, T or self.T, seed=seed)[:, None, :]

    def make(self, persistent, max_frames=MAX_FRAMES):
        if self.bank:
            b = self.bank.batch(self.n, max_frames, stream_model=self.member_of)
        else:
            b = self.models[0].batch(self.n, max_frames)
        if persistent:
            assert b.set_persistent(True), "the case is one of a session kernel"
            assert b.kernel_name() == self.kernel, b.kernel_name()
        b.Reset(prewarm=True)
        if self.ratio_of[0] is not None:
            for r in SLIM_RATIOS:
                b.SetSlimmableSize(r, [s for s in range(self.n) if self.ratio_of[s] == r])
        return b


def walk(b, x, lens, persistent, hook=None):
    """the calls of `lens` walking one device window contiguously (offsets of any alignment), one flush at the end;
    hook(b, k): before call k"""
    import torch
    n, _, T = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.zeros((n, b.model.NumOutputChannels(), T), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    at = 0
    for k, m in enumerate(lens):
        if hook:
            hook(b, k)
        b.process_device(xd.data_ptr() + at * 4, yd.data_ptr() + at * 4, m, T)
        at += m
    if persistent:
        b.flush()
    b.synchronize()
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def plugin(b, x, lens, persistent):
    """every call on the same buffer at offset 0, a flush between calls: the plugin pattern"""
    import torch
    n, ic, T = x.shape
    oc = b.model.NumOutputChannels()
    xd = torch.zeros((n, ic, MAX_FRAMES), dtype=torch.float32, device="cuda")
    yd = torch.zeros((n, oc, MAX_FRAMES), dtype=torch.float32, device="cuda")
    xs = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.zeros((n, oc, T), dtype=torch.float32, device="cuda")
    at = 0
    for m in lens:
        xd[:, :, :m] = xs[:, :, at:at + m]
        torch.cuda.synchronize()
        b.process_device(xd.data_ptr(), yd.data_ptr(), m, MAX_FRAMES)
        if persistent:
            b.flush()  # (not synchronize(): that ends the session)
        else:
            b.synchronize()
        torch.cuda.synchronize()
        out[:, :, at:at + m] = yd[:, :, :m]
        at += m
    torch.cuda.synchronize()
    return out.cpu().numpy()


def blocking(b, x, frames):
    """blocking process() calls of `frames` back to back"""
    return np.concatenate([b.process(x[:, :, k:k + frames]) for k in range(0, x.shape[2], frames)], axis=2)


def tickets(b, x, frames, depth, last):
    """tickets of `frames` with `depth` in flight, then one ticket of the `last` frames of x"""
    T = x.shape[2] - last
    ys, inflight = [], []
    for k in range(0, T, frames):
        if len(inflight) == depth:
            ys.append(b.wait(inflight.pop(0)))
        inflight.append(b.submit(x[:, :, k:k + frames]))
    while inflight:
        ys.append(b.wait(inflight.pop(0)))
    ys.append(b.wait(b.submit(x[:, :, T:])))
    return np.concatenate(ys, axis=2)


def session_lines(stderr):
    """[(starts, launches, commands)] of the `nam_hip session:` lines, in order (one per batch that ran a session, said when the
    batch is destroyed)"""
    out = []
    for ln in stderr.splitlines():
        m = re.match(r"nam_hip session: (\d+) starts, (\d+) launches \(\d+ from a wait / flush\), (\d+) commands stored by the host, (\d+) through the stream", ln)
        if m:
            out.append((int(m.group(1)), int(m.group(2)), int(m.group(3)) + int(m.group(4))))
    return out


def _equal_streams(a, b):
    return [s for s in range(a.shape[0]) if not np.array_equal(a[s], b[s])]


def child(what, name, tmp):
    """One process: `what` in persistent mode (its batches say their `nam_hip session:` lines on stderr, in the order listed in
    the answer's "order") and the same calls with persistent mode off; prints one JSON line."""
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import neuralampmodelercore_amd as nam
    nam.load_library()
    ans = {"what": what, "case": name, "order": []}
    if what == "schedule":
        c = Case(nam, name, tmp)
        x = c.signal()
        for how, drive in (("walk", walk), ("plugin", plugin)):
            b = c.make(True)
            y = drive(b, x, c.lens, True)
            b.close()
            ans["order"].append(how)
            b = c.make(False)
            want = drive(b, x, c.lens, False)
            b.close()
            ans[how] = {"differ": _equal_streams(y, want), "finite": bool(np.isfinite(y).all()), "peak": float(np.abs(y).max())}
            if how == "plugin":
                np.save(os.path.join(tmp, "y_plugin.npy"), y)
                ans[how]["differ_from_walk"] = _equal_streams(y, y_walk)  # (the same session form, other offsets and flushes)
            if how == "walk":
                y_walk = y
                np.save(os.path.join(tmp, "y_walk.npy"), y)
                np.save(os.path.join(tmp, "x.npy"), x)
        # the same signal through a session in whole 64-frame commands (and the remainder): lane = frame in nam_wn_reg_kernel and a
        # step per frame in the LSTM kernels, so where a call ends changes no frame's arithmetic — whatever form the session runs in
        lens64 = [BLOCK] * (c.T // BLOCK) + ([c.T % BLOCK] if c.T % BLOCK else [])
        b = c.make(True)
        y64 = walk(b, x, lens64, True)
        b.close()
        ans["order"].append("walk64")
        ans["walk64"] = {"differ": _equal_streams(y_walk, y64), "commands": len(lens64)}
        ans["commands"] = commands(c.lens)
        ans["frames"] = c.T
        ans.update(paths=c.paths, member_of=c.member_of, ratio_of=c.ratio_of, streams=c.n)
    elif what in ("blocking", "tickets"):
        c = Case(nam, name, tmp)
        T = 40 * 32 if what == "blocking" else 24 * 48 + 480
        x = c.signal(T=T)
        run = (lambda b: blocking(b, x, 32)) if what == "blocking" else (lambda b: tickets(b, x, 48, 8, 480))
        b = c.make(True)
        y = run(b)
        b.close()
        ans["order"].append(what)
        b = c.make(False)
        want = run(b)
        b.close()
        ans[what] = {"differ": _equal_streams(y, want), "finite": bool(np.isfinite(y).all()), "peak": float(np.abs(y).max())}
        ans["commands"] = 40 if what == "blocking" else 24 + 8
    elif what == "guard":
        # the pipeline kernels keep the multiple-of-64 rule: a 32-frame call between whole buffers ends the session, runs as a plain
        # launch, and the next whole buffer starts the session again
        from signals import stream_bank
        lens = [64, 64, 32, 64, 64]
        model = nam.get_dsp(model_file(name), fast_tanh=True)
        x = stream_bank(12, sum(lens), seed=978)[:, None, :]
        ys = []
        for persistent in (True, False):
            b = model.batch(12, BLOCK)
            if persistent:
                assert b.set_persistent(True)
                ans["kernel"] = b.kernel_name()
            b.Reset(prewarm=True)
            ys.append(walk(b, x, lens, persistent))
            b.close()
        ans["order"].append("guard")
        np.save(os.path.join(tmp, "y_guard.npy"), ys[0])
        np.save(os.path.join(tmp, "x.npy"), x)
        ans["guard"] = {"differ": _equal_streams(ys[0], ys[1]), "finite": bool(np.isfinite(ys[0]).all()), "peak": float(np.abs(ys[0]).max())}
        ans["commands"] = 4
    print("session_lengths: " + json.dumps(ans))


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2], sys.argv[3])
