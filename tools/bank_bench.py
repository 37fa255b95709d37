"""What a model bank costs, and what it is for (not bench.py: that measures the one-model headline).

256-stream persistent sessions on one GPU in bench.py's two shapes — regions of 20 commands between device synchronizes, and
regions of 500 commands — for
  (a) a one-model batch (wavenet_a1_standard; --family a2: A2.nam),
  (b) a bank batch with every stream on member 0,
  (c) a bank of 256 distinct members (standard-topology models with seeded weights, tests/bank_models.py; --family a2:
      A2-topology models with seeded weights, head_scale and LeakyReLU slope, tests/bank_models_a2.py), one per stream;
and the case a bank replaces: N captures as N one-stream batches called in turn with blocking 64-frame calls (N = 16 by
default: enough to extrapolate per-capture cost, and it keeps memory and session count small).
Every figure is the median of --runs repetitions (each a fresh timing of --regions regions); one JSON line per case.

    python tools/bank_bench.py [--family a1|a2] [--streams 256] [--runs 7] [--singles 16]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCK = 64


def time_session(batch, n_streams, region, regions, runs):
    """us per 64-frame step, median over `runs` (and the spread), for regions of `region` commands"""
    import torch
    T = BLOCK * region
    xd = (0.2 * torch.randn(n_streams, 1, T, device="cuda")).contiguous()
    yd = torch.zeros_like(xd)
    assert batch.set_persistent(True)
    batch.Reset(prewarm=True)

    def one_region():
        for k in range(region):
            batch.process_device(xd.data_ptr() + k * BLOCK * 4, yd.data_ptr() + k * BLOCK * 4, BLOCK, T)
        batch.flush()
        torch.cuda.synchronize()

    for _ in range(3):
        one_region()
    per_step = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(regions):
            one_region()
        per_step.append((time.perf_counter() - t0) * 1e6 / (regions * region))
    assert bool(torch.isfinite(yd).all())
    return statistics.median(per_step), min(per_step), max(per_step)


def xrt(n_streams, us_per_step):
    return n_streams * BLOCK / 48000.0 / (us_per_step * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--singles", type=int, default=16)
    ap.add_argument("--family", choices=["a1", "a2"], default="a1",
                    help="a1: the official topology (nam_a1_q_kernel); a2: the A2 topology (nam_kq_kernel)")
    args = ap.parse_args()
    import neuralampmodelercore_amd as nam
    if args.family == "a2":
        from bank_models_a2 import write_a2 as write_standard
    else:
        from bank_models import write_standard
    n = args.streams
    std_path = os.path.join(ROOT, "tests", "golden", "models", ("A2" if args.family == "a2" else "wavenet_a1_standard") + ".nam")
    std = nam.get_dsp(std_path, fast_tanh=True)
    with tempfile.TemporaryDirectory() as d:
        members = []
        for i in range(n):
            p = os.path.join(d, f"m{i}.nam")
            write_standard(p, 1000 + i)
            members.append(nam.get_dsp(p, fast_tanh=True))
    cases = {
        "a_one_model": lambda: std.batch(n, BLOCK),
        "b_bank_all_member_0": lambda: nam.ModelBank([std] + members[:7]).batch(n, BLOCK),
        "c_bank_distinct_members": lambda: nam.ModelBank(members).batch(n, BLOCK, stream_model=list(range(n))),
    }
    for region, regions in ((20, 50), (500, 4)):
        for name, make in cases.items():
            b = make()
            med, lo, hi = time_session(b, n, region, regions, args.runs)
            kernel = b.kernel_name()
            b.close()
            print(json.dumps(dict(case=name, streams=n, region_commands=region, us_per_step_median=round(med, 3), us_min=round(lo, 3),
                                  us_max=round(hi, 3), xrt=round(xrt(n, med)), kernel=kernel, runs=args.runs)), flush=True)
    # the case a bank replaces: one batch per capture, blocking 64-frame calls in turn
    k = args.singles
    batches = []
    for i in range(k):
        b = members[i].batch(1, BLOCK)
        b.set_persistent(True)
        b.Reset(prewarm=True)
        batches.append(b)
    x = (0.2 * np.random.default_rng(1).standard_normal((1, 1, BLOCK))).astype(np.float32)
    for _ in range(20):
        for b in batches:
            b.process(x)
    per_round = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        for _ in range(200):
            for b in batches:
                b.process(x)
        per_round.append((time.perf_counter() - t0) * 1e6 / 200)
    med = statistics.median(per_round)
    print(json.dumps(dict(case="d_one_stream_batches_in_turn", captures=k, us_per_round_median=round(med, 2), us_per_call=round(med / k, 2),
                          us_min=round(min(per_round), 2), us_max=round(max(per_round), 2), xrt=round(xrt(k, med)),
                          kernel=batches[0].kernel_name(), runs=args.runs,
                          note="per-capture cost is serial on the host: N captures cost N x us_per_call per 64 frames")), flush=True)
    for b in batches:
        b.close()


if __name__ == "__main__":
    main()
