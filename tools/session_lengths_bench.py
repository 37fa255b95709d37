"""What a persistent session costs per call at buffer sizes that are not multiples of 64 frames (not bench.py: that measures the
64-frame headline) — 32 and 48 frames (low-latency hosts), 96, and 120 / 240 / 480 (2.5 / 5 / 10 ms network packets at 48 kHz).

bench.py's configs 3, 4 and 5 at their stream counts (lstm.nam x 1,024: nam_lstm_row_kernel; wavenet_a2_max.nam x 512 and
slimmable_wavenet.nam x 768 at mixed widths: nam_wn_reg_kernel), device-resident buffers in persistent mode: regions of 20 calls
walking one window, a flush and a device synchronize behind each region (bank_bench.py's protocol). Per row: us per call (median,
min, max over --runs timings of --regions regions), xRT, and — from a second, untimed pass of ONE region per length with
NAM_HIP_SESSION_STATS=1 — the session starts / launches / commands of that region. 64 frames is in the list: the whole-buffer path,
whose run-to-run spread (us_min .. us_max) is the margin for "level" when two commits are compared. Then the blocking host call
(process()) at 32, 48 and 64 frames, 200 calls back to back, and tickets (submit / wait, 16 in flight) at 64 and 256 frames, 200 per
timing (--frames / --host-frames / --ticket-frames choose other lengths; "" = none).

Run the same file on two checkouts to compare them; every (config, pass) is a process of its own (the statistics switch is read
once per process), one JSON line per row.

    python tools/session_lengths_bench.py [--configs 3,4,5] [--runs 7] [--regions 10]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # bench.py: CONFIGS
    3: dict(model="lstm", streams=1024, slim_mix=False),
    4: dict(model="wavenet_a2_max", streams=512, slim_mix=False),
    5: dict(model="slimmable_wavenet", streams=768, slim_mix=True),
}
SLIM_RATIOS = (0.0, 0.34, 0.67, 1.0)
FRAMES = (32, 48, 64, 96, 120, 240, 480)
HOST_FRAMES = (32, 48, 64)
REGION = 20  # calls between flushes
TICKET_FRAMES = (64, 256)
TICKET_DEPTH = 16  # tickets in flight (NAM_HIP_PIPE_SLOTS)
TICKET_REGION = 200  # tickets per timing
MAX_FRAMES = 480


def xrt(n_streams, frames, us_per_call):
    return n_streams * frames / 48000.0 / (us_per_call * 1e-6)


def make_batch(nam, model, cfg):
    b = model.batch(cfg["streams"], MAX_FRAMES)
    assert b.set_persistent(True)
    b.Reset(prewarm=True)
    if cfg["slim_mix"]:
        for i, r in enumerate(SLIM_RATIOS):
            b.SetSlimmableSize(r, [s for s in range(cfg["streams"]) if s % 4 == i])
    return b


def child(config, stats, runs, regions, frames_list, host_frames_list, ticket_frames_list):
    import torch
    import neuralampmodelercore_amd as nam
    cfg = CONFIGS[config]
    n = cfg["streams"]
    model = nam.get_dsp(os.path.join(ROOT, "tests", "golden", "models", cfg["model"] + ".nam"), fast_tanh=True)
    ic = model.NumInputChannels()
    for frames in frames_list:
        T = frames * REGION
        xd = (0.2 * torch.randn(n, ic, T, device="cuda")).contiguous()
        yd = torch.zeros(n, model.NumOutputChannels(), T, device="cuda")
        b = make_batch(nam, model, cfg)

        def one_region():
            for k in range(REGION):
                b.process_device(xd.data_ptr() + k * frames * 4, yd.data_ptr() + k * frames * 4, frames, T)
            b.flush()
            torch.cuda.synchronize()

        row = dict(config=config, model=cfg["model"], streams=n, frames=frames, kernel=b.kernel_name())
        if stats:
            one_region()
            row["stats_region_calls"] = REGION
        else:
            for _ in range(3):
                one_region()
            per_call = []
            for _ in range(runs):
                t0 = time.perf_counter()
                for _ in range(regions):
                    one_region()
                per_call.append((time.perf_counter() - t0) * 1e6 / (regions * REGION))
            med = statistics.median(per_call)
            row.update(us_per_call_median=round(med, 3), us_min=round(min(per_call), 3), us_max=round(max(per_call), 3),
                       xrt=round(xrt(n, frames, med)), runs=runs)
        assert bool(torch.isfinite(yd).all())
        b.close()  # (says its `nam_hip session:` line when the statistics are on and a session ran)
        print("row-end", file=sys.stderr, flush=True)
        print("row: " + json.dumps(row), flush=True)
    for frames in host_frames_list:
        b = make_batch(nam, model, cfg)
        x = (0.2 * np.random.default_rng(1).standard_normal((n, ic, frames))).astype(np.float32)
        row = dict(config=config, model=cfg["model"], streams=n, frames=frames, path="blocking host call", kernel=b.kernel_name())
        if stats:
            for _ in range(REGION):
                b.process(x)
            row["stats_region_calls"] = REGION
        else:
            for _ in range(20):
                b.process(x)
            per_call = []
            for _ in range(runs):
                t0 = time.perf_counter()
                for _ in range(200):
                    b.process(x)
                per_call.append((time.perf_counter() - t0) * 1e6 / 200)
            med = statistics.median(per_call)
            row.update(us_per_call_median=round(med, 3), us_min=round(min(per_call), 3), us_max=round(max(per_call), 3),
                       xrt=round(xrt(n, frames, med)), runs=runs)
        b.close()
        print("row-end", file=sys.stderr, flush=True)
        print("row: " + json.dumps(row), flush=True)
    for frames in ticket_frames_list:
        b = make_batch(nam, model, cfg)
        x = (0.2 * np.random.default_rng(2).standard_normal((n, ic, frames))).astype(np.float32)
        out = np.empty((n, model.NumOutputChannels(), frames), dtype=np.float32)
        row = dict(config=config, model=cfg["model"], streams=n, frames=frames, path=f"tickets, {TICKET_DEPTH} in flight", kernel=b.kernel_name())

        def feed(n_tickets):
            inflight = []
            for _ in range(n_tickets):
                if len(inflight) == TICKET_DEPTH:
                    b.wait(inflight.pop(0), out)
                inflight.append(b.submit(x))
            while inflight:
                b.wait(inflight.pop(0), out)

        if stats:
            feed(TICKET_REGION)
            row["stats_region_calls"] = TICKET_REGION
        else:
            feed(TICKET_REGION)
            per_call = []
            for _ in range(runs):
                t0 = time.perf_counter()
                feed(TICKET_REGION)
                per_call.append((time.perf_counter() - t0) * 1e6 / TICKET_REGION)
            med = statistics.median(per_call)
            row.update(us_per_call_median=round(med, 3), us_min=round(min(per_call), 3), us_max=round(max(per_call), 3),
                       xrt=round(xrt(n, frames, med)), runs=runs)
        b.close()
        print("row-end", file=sys.stderr, flush=True)
        print("row: " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4,5")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--frames", default=",".join(map(str, FRAMES)), help="device-resident call lengths")
    ap.add_argument("--host-frames", default=",".join(map(str, HOST_FRAMES)), help="blocking host call lengths")
    ap.add_argument("--ticket-frames", default=",".join(map(str, TICKET_FRAMES)), help="ticket lengths (submit / wait, 16 in flight)")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--stats", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.stats, args.runs, args.regions, [int(f) for f in args.frames.split(",") if f],
                     [int(f) for f in args.host_frames.split(",") if f], [int(f) for f in args.ticket_frames.split(",") if f])
    for config in [int(c) for c in args.configs.split(",")]:
        rows = {}
        for stats in (False, True):
            env = {k: v for k, v in os.environ.items() if k != "NAM_HIP_SESSION_STATS"}
            if stats:
                env["NAM_HIP_SESSION_STATS"] = "1"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(config), "--runs", str(args.runs), "--regions", str(args.regions),
                                "--frames", args.frames, "--host-frames", args.host_frames, "--ticket-frames", args.ticket_frames]
                               + (["--stats"] if stats else []), env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"config {config}: the {'statistics' if stats else 'timing'} pass failed ({r.returncode})")
            got = [json.loads(ln[5:]) for ln in r.stdout.splitlines() if ln.startswith("row: ")]
            if not stats:
                rows = {(g["frames"], g.get("path", "")): g for g in got}
                continue
            # a batch says its line when it is closed, and none when no call of it entered a session: "row-end" separates the batches
            pat = r"nam_hip session: (\d+) starts, (\d+) launches \(\d+ from a wait / flush\), (\d+) commands stored by the host, (\d+) through the stream"
            chunks = r.stderr.split("row-end\n")
            for g, chunk in zip(got, chunks):
                m = re.search(pat, chunk)
                rows[(g["frames"], g.get("path", ""))].update(
                    region_calls=g["stats_region_calls"], session_starts=int(m.group(1)) if m else 0, session_launches=int(m.group(2)) if m else 0,
                    session_commands=int(m.group(3)) + int(m.group(4)) if m else 0)
        for row in rows.values():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
