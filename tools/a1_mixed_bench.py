"""A container of the official WaveNet topology's tiers (feather 8 / 4, lite 12 / 6, standard 16 / 8) with its streams at mixed
sizes (not bench.py: that measures the all-standard headline) — what persistent mode delivers when the tiers share a batch, and
what the size changes that mix and un-mix a batch cost. The container is assembled from the three fixtures, as tests/a1_mixed.py
does.

256 streams, 64-frame device-resident calls, persistent mode asked for (`persistent`: what set_persistent answered): regions of 20
calls walking one window, a flush and a device synchronize behind each region (a2_mixed_bench.py's protocol). Per case --runs
timings of --regions regions each, behind three warm-up regions: us per call as median, min and max (the spread is the margin for
"level" between two cases or two commits), xRT.

    mixed         86 standard, 85 lite, 85 feather streams (stream s on tier s % 3)
    standard, lite, feather
                  every stream at one size: the paths this feature must leave alone
    control       an all-lite batch: stream 0 to standard (the batch mixes: 255 streams' rows are copied next to it) and back (it
                  un-mixes: they are copied back), 64 frames in between; ms per call as the host sees it, and —
                  NAM_HIP_SESSION_STATS=1 — the library's own count of nam_state_rows_copy_kernel launches, stream states moved
                  and us spent in them; get_stream_state of a resident lite stream

The file runs on any commit that loads the fixtures: where a mixed batch has no session it says persistent=false and measures the
plain launches, one per size. Every case is a process of its own; one JSON line per row.

    python tools/a1_mixed_bench.py [--cases mixed,standard,lite,feather,control] [--runs 5] [--regions 10] [--streams 256]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = os.path.join(ROOT, "tests", "golden", "models")
FIXTURES = ("synth_a1_feather", "synth_a1_lite", "wavenet_a1_standard")  # ascending max_value
MAX_VALUES = (0.25, 0.5, 1.0)
RATIO = (0.1, 0.4, 1.0)  # selects submodel 0, 1, 2
FEATHER, LITE, STANDARD = 0, 1, 2
FRAMES, REGION = 64, 20
CASES = ("mixed", "standard", "lite", "feather", "control")


def container_text():
    subs = []
    for v, name in zip(MAX_VALUES, FIXTURES):
        with open(os.path.join(MODELS, name + ".nam")) as f:
            subs.append({"max_value": v, "model": json.load(f)})
    return json.dumps({"version": "0.5.4", "architecture": "SlimmableContainer", "weights": [], "sample_rate": 48000, "config": {"submodels": subs}})


def tiers(case, n):
    if case == "mixed":
        return [(STANDARD, LITE, FEATHER)[s % 3] for s in range(n)]
    return [dict(standard=STANDARD, lite=LITE, feather=FEATHER, control=LITE)[case]] * n


def child(case, n, runs, regions):
    import torch
    import neuralampmodelercore_amd as nam
    model = nam.get_dsp_json(container_text(), fast_tanh=True)
    ts = tiers(case, n)
    b = model.batch(n, FRAMES)
    b.Reset(prewarm=True)
    for w in sorted(set(ts)):
        if w != STANDARD:
            b.SetSlimmableSize(RATIO[w], [s for s, v in enumerate(ts) if v == w])
    persistent = bool(b.set_persistent(True))
    T = FRAMES * REGION
    xd = (0.2 * torch.randn(n, 1, T, device="cuda")).contiguous()
    yd = torch.zeros(n, 1, T, device="cuda")

    def one_region(calls=REGION):
        for k in range(calls):
            b.process_device(xd.data_ptr() + k * FRAMES * 4, yd.data_ptr() + k * FRAMES * 4, FRAMES, T)
        b.flush()
        torch.cuda.synchronize()

    row = dict(case=case, streams=n, per_tier=[ts.count(w) for w in (FEATHER, LITE, STANDARD)], frames=FRAMES, persistent=persistent,
               kernel=b.kernel_name())
    if case != "control":
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
                   xrt=round(n * FRAMES / 48000.0 / (med * 1e-6)), runs=runs)
    else:
        t_mix, t_unmix, t_get = [], [], []
        for _ in range(max(runs, 5)):
            one_region(1)
            t0 = time.perf_counter()
            b.SetSlimmableSize(RATIO[STANDARD], [0])
            t_mix.append((time.perf_counter() - t0) * 1e3)
            row["kernel_mixed"] = b.kernel_name()
            one_region(1)
            t0 = time.perf_counter()
            b.get_stream_state(1)
            t_get.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            b.SetSlimmableSize(RATIO[LITE], [0])
            t_unmix.append((time.perf_counter() - t0) * 1e3)
        med = lambda v: round(statistics.median(v), 3)  # noqa: E731
        row.update(ms_mix_median=med(t_mix), ms_mix_max=round(max(t_mix), 3), ms_unmix_median=med(t_unmix), ms_unmix_max=round(max(t_unmix), 3),
                   ms_get_stream_state_median=med(t_get), control_calls_each=len(t_mix))
    assert bool(torch.isfinite(yd).all())
    b.close()
    print("row: " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.streams, args.runs, args.regions)
    for case in [c for c in args.cases.split(",") if c]:
        assert case in CASES, case
        env = {k: v for k, v in os.environ.items() if k != "NAM_HIP_SESSION_STATS"}
        if case == "control":
            env["NAM_HIP_SESSION_STATS"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--runs", str(args.runs), "--regions", str(args.regions),
                            "--streams", str(args.streams)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"case {case} failed ({r.returncode})")
        row = [json.loads(ln[5:]) for ln in r.stdout.splitlines() if ln.startswith("row: ")][0]
        m = re.search(r"nam_hip A1 mixed sizes: (\d+) launches of nam_state_rows_copy_kernel moved (\d+) stream states, ([0-9.]+) us", r.stderr)
        if m:
            row.update(copy_launches=int(m.group(1)), stream_states_moved=int(m.group(2)), copy_us_total=float(m.group(3)),
                       copy_us_per_launch=round(float(m.group(3)) / max(int(m.group(1)), 1), 1))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
