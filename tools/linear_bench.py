"""Linear models (impulse responses) on nam_linear_kernel: time per 64-frame call and per rendered second, next to the floor.

    python tools/linear_bench.py [--out FILE.json] [--quick]

Device-resident audio, nam_hip_batch_process_device, a host clock around a window of calls that ends in a synchronise of the batch
and of the device; every shape is warmed up first and the window is sized to at least `--window-ms` of work, three windows per case
(the median is reported, all three are kept). Per case one JSON line:

    us_per_call      one 64-frame call = append + nam_linear_kernel + reduce (three launches), all streams
    x_realtime       streams x 64 frames / 48 kHz / time per call
    floor_us         max(HBM bytes moved / 6.3 TB/s, 2 * 64 * R * columns flops / 155 TFLOP/s): the history rows the call reads
                     (R + 63 frames x columns x 4 bytes), the input and output once, and the partial sums written and read once
    floor_frac       floor / measured
    launch_only_us   the same three launches at R = 1 (one tap): what dispatch alone costs; the share of it in a small-R call is
                     launch_only_us / us_per_call

and one 10-second render (nam_hip_batch_process_device over 480,000 frames: the host cuts it into pieces) at 256 streams, R = 8,192.
For orientation only, f32_strict of tests/linear_oracle.py on one CPU core for one stream of the same length.

    python tools/linear_bench.py --container 512,2048,8192 [--streams 256] [--out FILE.json] [--quick]

measures a SlimmableContainer of Linear models of those tap counts (nam_linear_pairs_kernel: per-stream impulse responses) instead,
each case as a 64-frame call and as a 10-second render, in one session on one device:

    (a) every stream on the largest size, next to a one-model batch of that impulse response (nam_linear_kernel): the difference
        is what the work list's indirection costs
    (b) sizes sorted by stream next to sizes interleaved (every 32-stream tile carries every size): the work-list sizes
        (pairs, K-split slabs) are reported beside the times
    (c) what a host does without the container — one one-model batch per size, streams split evenly, called in turn — next to
        the one container batch with the same (sorted) assignment
    launch_only_us: the container's three launches with one-tap submodels, and the one-model batch's at R = 1
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
F32_MATRIX_FLOPS = 155e12
SR = 48000.0


def floor_us(R, columns, frames=64):
    hist = (R + frames - 1) * columns * 4
    io = 2 * frames * columns * 4
    return 1e6 * max((hist + io) / HBM_BYTES_PER_S, 2.0 * frames * R * columns / F32_MATRIX_FLOPS), hist + io


def time_calls(batch, xd, yd, frames, total, window_ms):
    """us per call of `frames` frames walking a resident window of `total` frames."""
    import torch
    calls_per_pass = total // frames

    def one_pass():
        for k in range(calls_per_pass):
            off = k * frames * 4
            batch.process_device(xd.data_ptr() + off, yd.data_ptr() + off, frames, total, torch.cuda.current_stream().cuda_stream)

    def timed(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass()
        batch.synchronize()  # (the launches run on the batch's own stream when torch's current stream is the default one)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    timed(1)  # warm-up: code objects, clocks
    passes = max(3, int(window_ms * 1e-3 / max(timed(1), 1e-6)) + 1)
    best = [timed(passes) * 1e6 / (passes * calls_per_pass) for _ in range(3)]
    return float(np.median(best)), [float(v) for v in best]


def container_cases(args, sizes, window, emit):
    import torch
    import neuralampmodelercore_amd as nam
    import linear_oracle as lo
    W, streams = len(sizes), args.streams
    seconds = 1 if args.quick else 10

    def doc_of(rs):
        subs = [{"max_value": (i + 1) / len(rs), "model": lo.linear_doc(R, True, seed=R)} for i, R in enumerate(rs)]
        return {"version": "0.5.4", "architecture": "SlimmableContainer", "weights": [], "sample_rate": 48000, "config": {"submodels": subs}}

    ratios = [(i + 0.5) / W for i in range(W - 1)] + [1.0]
    xd64 = (torch.rand((streams, 1, 64 * 32), device="cuda") - 0.5).contiguous()
    total = int(seconds * SR)
    xdr = (torch.rand((streams, 1, total), device="cuda") - 0.5).contiguous()

    def measure(batches, rows):
        """`batches` called in turn, batch i on the rows rows[i] (a slice of streams): (us per 64-frame call, us per render)."""
        out = []
        for xd, frames, win in ((xd64, 64, window), (xdr, total, 0.0)):
            parts = [xd[r].contiguous() for r in rows]
            outs = [torch.zeros_like(p_) for p_ in parts]
            n_total = xd.shape[2]

            class Turn:  # time_calls drives one object: the batches in turn
                def process_device(self, d_in, d_out, n, stride, stream):
                    off = d_in - parts[0].data_ptr()
                    for b, p_, o in zip(batches, parts, outs):
                        b.process_device(p_.data_ptr() + off, o.data_ptr() + off, n, stride, stream)

                def synchronize(self):
                    for b in batches:
                        b.synchronize()
            us, reps = time_calls(Turn(), parts[0], outs[0], frames, n_total, win)
            out.append((us, reps))
        return out

    def report(case, what, batches, rows, extra):
        (us, reps), (usr, repsr) = measure(batches, rows)
        emit(dict({"case": case, "what": what, "streams": streams, "sizes": sizes, "us_per_call": round(us, 3), "reps_us": [round(v, 3) for v in reps],
                   "x_realtime": round(streams * 64 / SR / (us * 1e-6), 1), "render_seconds": seconds, "ms_per_render": round(usr * 1e-3, 3),
                   "reps_ms": [round(v * 1e-3, 3) for v in repsr], "render_x_realtime": round(streams * seconds / (usr * 1e-6), 1),
                   "render_us_per_64_frames": round(usr / (total / 64), 3), "kernel": batches[0].kernel_name()}, **extra))

    def worklist(assign):
        tiles = (streams + 31) // 32
        pairs = sum(len(set(assign[32 * t:32 * t + 32])) for t in range(tiles))
        return {"tiles": tiles, "pairs": pairs}

    def container(rs, assign):
        b = nam.get_dsp_json(json.dumps(doc_of(rs))).batch(streams, 64)
        for w in range(W - 1):
            ids = [s for s, v in enumerate(assign) if v == w]
            if ids:
                b.SetSlimmableSize(ratios[w], ids)
        return b

    everyone = [slice(0, streams)]
    sorted_assign = [s * W // streams for s in range(streams)]
    mixed_assign = [s % W for s in range(streams)]
    # launch only: one-tap submodels, interleaved; the one-model batch at R = 1
    b = container([1] * W, mixed_assign)
    report("launch_only", "container of one-tap submodels, interleaved", [b], everyone, worklist(mixed_assign))
    b.close()
    b = nam.get_dsp_json(json.dumps(lo.linear_doc(1, True, seed=1))).batch(streams, 64)
    report("launch_only", "one-model batch, one tap", [b], everyone, {})
    b.close()
    # (a)
    b = container(sizes, [W - 1] * streams)
    report("a", "container, every stream on the largest size", [b], everyone, worklist([W - 1] * streams))
    b.close()
    b = nam.get_dsp_json(json.dumps(lo.linear_doc(sizes[-1], True, seed=sizes[-1]))).batch(streams, 64)
    report("a", "one-model batch of the largest size", [b], everyone, {})
    b.close()
    # (b)
    for what, assign in (("container, sizes sorted by stream", sorted_assign), ("container, sizes interleaved", mixed_assign)):
        b = container(sizes, assign)
        report("b", what, [b], everyone, worklist(assign))
        b.close()
    # (c)
    bounds = [next((s for s, v in enumerate(sorted_assign) if v == w), streams) for w in range(W)] + [streams]
    rows = [slice(bounds[w], bounds[w + 1]) for w in range(W)]
    batches = [nam.get_dsp_json(json.dumps(lo.linear_doc(R, True, seed=R))).batch(bounds[w + 1] - bounds[w], 64) for w, R in enumerate(sizes)]
    report("c", "one one-model batch per size, called in turn", batches, rows, {"streams_per_batch": [r.stop - r.start for r in rows]})
    for b in batches:
        b.close()
    b = container(sizes, sorted_assign)
    report("c", "the one container batch, same assignment", [b], everyone, worklist(sorted_assign))
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="short windows and a 1-second render (a rehearsal)")
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--container", default=None, metavar="R1,R2,...", help="measure a SlimmableContainer of Linear models of these tap counts instead")
    ap.add_argument("--streams", type=int, default=256, help="streams of the --container cases")
    args = ap.parse_args()
    import torch
    import neuralampmodelercore_amd as nam
    import linear_oracle as lo
    if not torch.cuda.is_available():
        raise SystemExit("linear_bench.py: no GPU (a measurement path does not fall back)")
    window = 30.0 if args.quick else args.window_ms
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def write_out():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for d in lines:
                    f.write(json.dumps(d) + "\n")

    if args.container:
        container_cases(args, [int(v) for v in args.container.split(",")], window, emit)
        write_out()
        return
    cases = [(256, 1), (256, 256), (256, 2048), (256, 8192), (256, 32768), (1024, 8192)]
    launch_only = {}
    for streams, R in cases:
        m = nam.get_dsp_json(json.dumps(lo.linear_doc(R, True, seed=R)))
        b = m.batch(streams, 64)
        total = 64 * 32
        xd = (torch.rand((streams, 1, total), device="cuda") - 0.5).contiguous()
        yd = torch.zeros_like(xd)
        us, reps = time_calls(b, xd, yd, 64, total, window)
        b.close()
        if R == 1:
            launch_only[streams] = us
        fl, nbytes = floor_us(R, streams)
        emit({"case": "call64", "streams": streams, "R": R, "us_per_call": round(us, 3), "reps_us": [round(v, 3) for v in reps],
              "x_realtime": round(streams * 64 / SR / (us * 1e-6), 1), "floor_us": round(fl, 3), "floor_frac": round(fl / us, 4),
              "floor_bytes": nbytes, "launch_only_us": round(launch_only.get(256, float("nan")), 3), "describe": m.describe()})
    # the render
    streams, R, seconds = 256, 8192, 1 if args.quick else 10
    m = nam.get_dsp_json(json.dumps(lo.linear_doc(R, True, seed=R)))
    b = m.batch(streams, 64)
    total = int(seconds * SR)
    xd = (torch.rand((streams, 1, total), device="cuda") - 0.5).contiguous()
    yd = torch.zeros_like(xd)
    us, reps = time_calls(b, xd, yd, total, total, 0.0)
    b.close()
    fl, _ = floor_us(R, streams)
    emit({"case": "render", "streams": streams, "R": R, "seconds": seconds, "ms_per_render": round(us * 1e-3, 3),
          "reps_ms": [round(v * 1e-3, 3) for v in reps], "x_realtime": round(streams * seconds / (us * 1e-6), 1),
          "us_per_64_frames": round(us / (total / 64), 3), "floor_us_per_64_frames": round(fl, 3), "floor_frac": round(fl / (us / (total / 64)), 4)})
    # orientation: the strict float32 restatement on one CPU core, one stream
    n = 4096
    h, bias = lo.taps_and_bias(lo.linear_doc(R, True, seed=R))
    x = np.random.default_rng(0).uniform(-0.5, 0.5, size=(1, n)).astype(np.float32)
    t0 = time.perf_counter()
    lo.f32_strict(h, bias, x, "oldest")
    dt = time.perf_counter() - t0
    emit({"case": "cpu_f32_strict_numpy", "streams": 1, "R": R, "frames": n, "x_realtime": round(n / SR / dt, 2)})
    write_out()


if __name__ == "__main__":
    main()
