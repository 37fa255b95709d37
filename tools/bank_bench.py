"""What a model bank costs, and what it is for (not bench.py: that measures the one-model headline).

256-stream persistent sessions on one GPU in bench.py's two shapes — regions of 20 commands between device synchronizes, and
regions of 500 commands — for
  (a) a one-model batch (wavenet_a1_standard; --family a2: A2.nam),
  (b) a bank batch with every stream on member 0,
  (c) a bank of 256 distinct members (standard-topology models with seeded weights, tests/bank_models.py; --family a2:
      A2-topology models with seeded weights, head_scale and LeakyReLU slope), one per stream;
and the case a bank replaces: N captures as N one-stream batches called in turn with blocking 64-frame calls (N = 16 by
default: enough to extrapolate per-capture cost, and it keeps memory and session count small).
Every figure is the median of --runs repetitions (each a fresh timing of --regions regions); one JSON line per case.

    python tools/bank_bench.py [--family a1|a2|nano] [--streams 256] [--runs 7] [--singles 16]

--family nano: the nam_wn_reg_kernel family on the official nano size (synth_a1_nano.nam; members from tests/bank_wr_models.py with
the fixture's head_scale, so every member's per-model code object is the fixture's: one compile, found by hash afterwards).

--family lstm: the LSTM family's two kernels in their bench shapes — one layer of 3 units at 1,024 streams (config 3's shape:
nam_lstm_row_kernel, four streams per wavefront) and one layer of 24 units at 256 streams (nam_lstm_wide_kernel, one stream
per wavefront); members from tests/bank_models.py, (a) is member 0 as a one-model batch. The three cases are INTERLEAVED:
run r times (a), (b), (c) one after the other before run r + 1 starts, so that a drift of the box lands on all three.

    python tools/bank_bench.py --family lstm [--runs 7] [--singles 16]
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


def time_sessions_interleaved(batches, n_streams, in_ch, region, regions, runs):
    """time_session for several batches of one shape at once: {name: (median, min, max)}, run r of every batch before run r + 1"""
    import torch
    T = BLOCK * region
    xd = (0.2 * torch.randn(n_streams, in_ch, T, device="cuda")).contiguous()
    yd = torch.zeros(n_streams, 1, T, device="cuda")

    def one_region(batch):
        for k in range(region):
            batch.process_device(xd.data_ptr() + k * BLOCK * 4, yd.data_ptr() + k * BLOCK * 4, BLOCK, T)
        batch.flush()
        torch.cuda.synchronize()

    for batch in batches.values():
        assert batch.set_persistent(True)
        batch.Reset(prewarm=True)
        for _ in range(3):
            one_region(batch)
    per_step = {name: [] for name in batches}
    for _ in range(runs):
        for name, batch in batches.items():
            t0 = time.perf_counter()
            for _ in range(regions):
                one_region(batch)
            per_step[name].append((time.perf_counter() - t0) * 1e6 / (regions * region))
    assert bool(torch.isfinite(yd).all())
    return {name: (statistics.median(v), min(v), max(v)) for name, v in per_step.items()}


def main_lstm(args, nam):
    from bank_models import write_lstm
    for shape, hidden, n in (("row_1x3", 3, 1024), ("wide_1x24", 24, 256)):
        with tempfile.TemporaryDirectory() as d:
            members = []
            for i in range(n):
                p = os.path.join(d, f"m{i}.nam")
                write_lstm(p, 2000 + i, num_layers=1, input_size=1, hidden=hidden, out_channels=1)
                members.append(nam.get_dsp(p, fast_tanh=True))
        for region, regions in ((20, 50), (500, 4)):
            batches = {
                "a_one_model": members[0].batch(n, BLOCK),
                "b_bank_all_member_0": nam.ModelBank(members[:8]).batch(n, BLOCK),
                "c_bank_distinct_members": nam.ModelBank(members).batch(n, BLOCK, stream_model=list(range(n))),
            }
            res = time_sessions_interleaved(batches, n, 1, region, regions, args.runs)
            for name, (med, lo, hi) in res.items():
                print(json.dumps(dict(case=name, shape=shape, streams=n, region_commands=region, us_per_step_median=round(med, 3),
                                      us_min=round(lo, 3), us_max=round(hi, 3), xrt=round(xrt(n, med)), kernel=batches[name].kernel_name(),
                                      runs=args.runs, interleaved=True)), flush=True)
            for b in batches.values():
                b.close()
        singles_in_turn(args, members, shape)


def xrt(n_streams, us_per_step):
    return n_streams * BLOCK / 48000.0 / (us_per_step * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--singles", type=int, default=16)
    ap.add_argument("--family", choices=["a1", "a2", "nano", "lstm"], default="a1",
                    help="a1: the official topology (nam_a1_q_kernel); a2: the A2 topology (nam_kq_kernel); "
                         "nano: the official nano size (nam_wn_reg_kernel); "
                         "lstm: nam_lstm_row_kernel / nam_lstm_wide_kernel in their own shapes (--streams is not read)")
    args = ap.parse_args()
    import neuralampmodelercore_amd as nam
    if args.family == "lstm":
        return main_lstm(args, nam)
    if args.family == "a2":
        from bank_models import write_a2 as write_standard
    elif args.family == "nano":
        from bank_wr_models import write_nano as write_standard
    else:
        from bank_models import write_standard
    n = args.streams
    std_path = os.path.join(ROOT, "tests", "golden", "models", dict(a2="A2", nano="synth_a1_nano").get(args.family, "wavenet_a1_standard") + ".nam")
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
    singles_in_turn(args, members)


def singles_in_turn(args, members, shape=None):
    """the case a bank replaces: one batch per capture, blocking 64-frame calls in turn"""
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
                          kernel=batches[0].kernel_name(), runs=args.runs, **(dict(shape=shape) if shape else {}),
                          note="per-capture cost is serial on the host: N captures cost N x us_per_call per 64 frames")), flush=True)
    for b in batches:
        b.close()


if __name__ == "__main__":
    main()
