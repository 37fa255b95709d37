"""Ring phases: where a call pattern puts the write position of every convolution-history ring (no GPU, no kernel: integers).

Every WaveNet kernel keeps a layer's input history in a ring of R rows — R = 2 d + 64 for the official topology (csrc/aq_table.h),
R = (K - 1) d + 64 for the A2 topology (csrc/kp_table.h) — and a call of n frames moves every ring's write position on by n, modulo
its own R. What a kernel does at a position depends on the position (kernel_a1_q.hip: store_rows' second store in a ring's first 15
rows and over its end, far_load's and the append's wrap when sixteen rows run over the end of an HBM ring; kernel_kq.hip: the
windows' tails), and a session of 64-frame buffers only ever reaches the positions 64 k mod R. This module makes call patterns that
reach ALL of them and says, for a frame of such a pattern, where every ring stood: tests/test_ring_phase_schedule.py checks the
coverage, tests/test_gpu_ring_phase.py drives the kernels through the patterns.

ring_lengths(family)      the rings of a family, read from the headers (a host program compiled against them) or, for a model
                          that runs nam_wn_reg_kernel, the bound (K - 1) d + 64 per layer from the .nam file
schedule(rings, mode)     a list of calls (kind, n_frames): "session" — cycles of one ragged call and a burst of 64-frame session
                          commands —, "launch" — plain launches of 128 + r frames, r in 1 .. 63
starts(rings, calls, f0)  every ring's write position at the start of every call
describe(...)             the rings' positions and classes around one frame, for an assertion message"""
import functools
import json
import os
import shutil
import subprocess
import tempfile
from collections import namedtuple
from math import gcd

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuralampmodelercore_amd", "csrc")

BLOCK = 64  # frames per session command (aq::kBlockF)
SUB = 16  # rows per sub-block of the big stages of nam_a1_q_kernel
MIN_BURST = 5  # three bursts of at most four buffers in a row switch a session to nam_a1_p4_kernel (include/nam_hip.h)

# name: as the family's header counts it; resident: the whole ring lives in LDS while a launch runs; mirrored: a resident ring
# followed by a copy of its first `mirror` rows (aq::mirror_rows)
Ring = namedtuple("Ring", "name R resident mirror")

_PROGRAMS = {
    "a1": r"""
#include <cstdio>
#include "aq_table.h"
using namespace namhip::aq;
int main()
{
  for (int j = 0; j < kJobs; j++)
    if (has_ring(j))
      std::printf("ring%d %d %d %d\n", ring_id(j), ring_len(j), (int)res(j), mirror_rows(j));
  return 0;
}
""",
    # resident: the job's whole history (K - 1) d stands in its LDS window (kernel_kq.hip: at most kWinMax = 3 * 64 rows)
    "a2": r"""
#include <cstdio>
#include "kp_table.h"
using namespace namhip::kp;
int main()
{
  for (int j = 0; j < kJobs; j++)
    std::printf("job%d %d %d 0\n", j, ring_len(j), (int)(ring_len(j) - 64 <= 3 * 64));
  return 0;
}
""",
}


@functools.lru_cache(maxsize=None)
def _header_rings(family):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        raise RuntimeError("no host C++ compiler to evaluate the ring tables")
    with tempfile.TemporaryDirectory(prefix="ring_phase_") as d:
        src, exe = os.path.join(d, "rings.cpp"), os.path.join(d, "rings")
        with open(src, "w") as f:
            f.write(_PROGRAMS[family])
        subprocess.check_call([cxx, "-std=c++17", "-I", CSRC, "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    rings = []
    for line in out.splitlines():
        name, R, res, mirror = line.split()
        rings.append(Ring(name, int(R), bool(int(res)), int(mirror)))
    return tuple(rings)


def _nam_rings(config, prefix=""):
    rings = []
    if config.get("condition_dsp") is not None:
        rings += _nam_rings(config["condition_dsp"]["config"], prefix + "cond.")
    for a, lc in enumerate(config["layers"]):
        ks = lc["kernel_sizes"] if "kernel_sizes" in lc else [lc["kernel_size"]] * len(lc["dilations"])
        for l, (K, d) in enumerate(zip(ks, lc["dilations"])):
            rings.append(Ring(f"{prefix}array{a}.layer{l}", (int(K) - 1) * int(d) + BLOCK, True, 0))
    return rings


def ring_lengths(family, nam_path=None):
    """The rings of "a1" (the official topology: nam_a1_q / p4 / p2 / mfma kernels; 20 rings) or "a2" (nam_kq / nam_kt_mfma
    kernels; 24 jobs) from the headers; "wn_reg": the bound (K - 1) d + 64 of every layer of the WaveNet in `nam_path` (its
    condition_dsp's layers included) — nam_wn_reg_kernel's own ring sizes are internal."""
    if family in _PROGRAMS:
        return list(_header_rings(family))
    if family != "wn_reg" or nam_path is None:
        raise ValueError(f"ring_lengths: family {family!r}" + (" needs a .nam path" if family == "wn_reg" else ""))
    with open(nam_path) as f:
        return _nam_rings(json.load(f)["config"])


def _lengths(rings):
    return sorted({r.R for r in rings})


def schedule(rings, mode, r=1, B=7):
    """Calls (kind, n_frames) that put every ring of `rings` at every position.
    "session": cycles of ("ragged", r) and B x ("session", 64). With one r the advance per cycle r + 64 B must be coprime to every
    ring length (1 + 64 * 7 = 449, a prime, is): as many cycles as the longest ring has rows then start a burst at every position
    of every ring. Of several r values each cycle takes one (greedily, as below), and the cycles go on until every ring has started a burst at
    every position and every r has occurred.
    "launch": ("launch", 128 + r), r in 1 .. 63 — three blocks, the last one ragged —, each r chosen (greedily: the r that puts
    the most rings where they have not started a launch yet, the least used among equals) until every RESIDENT ring has started a
    launch at every position and every r has occurred."""
    Rs = _lengths(rings)
    if mode == "session":
        if B < MIN_BURST:
            raise ValueError(f"schedule: bursts of {B} buffers would move the session to the low-latency kernel")
        rs = [int(r)] if np.isscalar(r) else [int(v) for v in r]
        if any(v <= 0 or v >= BLOCK for v in rs):
            raise ValueError("schedule: a ragged call has 1 .. 63 frames")
        if len(rs) == 1:
            adv = rs[0] + BLOCK * B
            bad = [R for R in Rs if gcd(adv, R) != 1]
            if bad:
                raise ValueError(f"schedule: the advance per cycle {adv} is not coprime to the ring lengths {bad}")
        seen = {R: np.zeros(R, dtype=bool) for R in Rs}
        used = {v: 0 for v in rs}
        calls, at, c = [], 0, 0
        while True:
            # (several r: the one that starts the burst where the most rings have not started one yet, the least used among equals)
            v = max(rs, key=lambda v: (sum(0 if seen[R][(at + v) % R] else 1 for R in Rs), -used[v], -v))
            used[v] += 1
            calls.append(("ragged", v))
            at += v
            for R in Rs:
                seen[R][at % R] = True
            calls += [("session", BLOCK)] * B
            at += BLOCK * B
            c += 1
            if c >= max(Rs) and all(s.all() for s in seen.values()) and all(used.values()):
                return calls
            if c > 64 * max(Rs):
                raise RuntimeError("schedule: the session pattern does not reach every position")
    if mode == "launch":
        Rs = _lengths([x for x in rings if x.resident])
        seen = {R: np.zeros(R, dtype=bool) for R in Rs}
        used = np.zeros(BLOCK, dtype=int)
        calls, at = [], 0
        while not (all(s.all() for s in seen.values()) and used[1:].all()):
            for R in Rs:
                seen[R][at % R] = True
            # the launch after this one starts at + 128 + r: how many rings does that put at a new position?
            gain = [sum(0 if seen[R][(at + 2 * BLOCK + v) % R] else 1 for R in Rs) for v in range(1, BLOCK)]
            best = max(range(1, BLOCK), key=lambda v: (gain[v - 1], -used[v], -v))
            used[best] += 1
            calls.append(("launch", 2 * BLOCK + best))
            at += 2 * BLOCK + best
            if len(calls) > 64 * max(Rs):
                raise RuntimeError("schedule: the launch pattern does not reach every position")
        return calls
    raise ValueError(f"schedule: mode {mode!r}")


def offsets(calls):
    """frame offset of every call (and, last, the total)"""
    return np.concatenate([[0], np.cumsum([n for _, n in calls], dtype=np.int64)])


def starts(rings, calls, frames_before=0):
    """[n_rings, n_calls]: every ring's write position when a call starts; `frames_before`: what went through the rings since
    their Reset (the prewarm's silence)."""
    off = offsets(calls)[:-1] + int(frames_before)
    return np.stack([off % r.R for r in rings])


def store_class(ring, so):
    """sixteen rows from `so` on in a mirrored ring (kernel_a1_q.hip: store_rows): "head" — some of them are mirrored rows, the
    second store goes R rows up —, "overrun" — they run over the ring's end, the second store goes R rows down —, else "plain"."""
    if ring.mirror and so < ring.mirror:
        return "head"
    if ring.mirror and so > ring.R - SUB:
        return "overrun"
    return "plain"


def wraps(ring, t, rows=SUB):
    """`rows` rows from t on run over the ring's end (an HBM ring: far_load's and the append's fallback to a per-lane wrap)"""
    return t + rows > ring.R


def tap_positions(ring, so):
    """the two older taps' first rows for the sixteen frames at `so` (official topology: R = 2 d + 64, taps d and 2 d back)"""
    d = (ring.R - BLOCK) // 2
    return [(so - 2 * d) % ring.R, (so - d) % ring.R]


def sub_blocks(ring, wp):
    """ring positions of the four sixteen-frame sub-blocks of a 64-frame buffer written at wp"""
    return [(wp + SUB * i) % ring.R for i in range(BLOCK // SUB)]


def _classes(ring, wp, n_frames, taps):
    """the classes the sub-blocks of a call of n_frames at wp fall in"""
    tags = set()
    for k in range(0, n_frames, SUB):
        so = (wp + k) % ring.R
        if ring.mirror:
            tags.add(store_class(ring, so))
            if taps and any(t + SUB > ring.R for t in tap_positions(ring, so)):
                tags.add("tap window in the mirror")
        elif not ring.resident:
            if wraps(ring, so) or (taps and any(wraps(ring, t) for t in tap_positions(ring, so))):
                tags.add("HBM fallback")
        elif so + SUB > ring.R:
            tags.add("wraps")
    tags.discard("plain")
    return "/".join(sorted(tags))


def cycles_of(calls, frames):
    """the cycle (a ragged call or a launch, and the session commands behind it) every frame of `frames` lies in"""
    off = offsets(calls)
    heads = np.array([int(off[k]) for k, c in enumerate(calls) if c[0] != "session"], dtype=np.int64)
    return np.maximum(np.searchsorted(heads, np.asarray(frames), side="right") - 1, 0)


def describe(rings, calls, frames_before, frame, taps=True):
    """Where the rings stood around `frame` of the signal `calls` cut up: the call it lies in, the cycle (a ragged call and the
    burst behind it; in launch mode a cycle is one launch) and, for every ring, the position at which the cycle's burst started
    and the position of the call itself, each with the classes its sub-blocks fall in. `taps`: the rings are the official
    topology's (taps d and 2 d back)."""
    off = offsets(calls)
    i = int(np.searchsorted(off, frame, side="right")) - 1
    first = i
    while first > 0 and calls[first][0] == "session" and calls[first - 1][0] == "session":
        first -= 1  # the burst's first command
    ragged = [k for k, c in enumerate(calls[:first + 1]) if c[0] != "session"]
    cycle = len(ragged) - 1 if ragged else 0
    burst_frames = 0
    for k in range(first, len(calls)):
        if calls[k][0] != calls[first][0] or (k > first and calls[k][0] != "session"):
            break
        burst_frames += calls[k][1]
    lines = [f"frame {frame} lies in call {i} ({calls[i][0]}, {calls[i][1]} frames, from frame {int(off[i])}) of cycle {cycle}, "
             f"whose {'burst' if calls[first][0] == 'session' else calls[first][0]} starts at frame {int(off[first])}"]
    for r in rings:
        p0 = int((off[first] + frames_before) % r.R)
        p1 = int((off[i] + frames_before) % r.R)
        c0, c1 = _classes(r, p0, burst_frames, taps), _classes(r, p1, calls[i][1], taps)
        kind = "mirrored" if r.mirror else "resident" if r.resident else "HBM"
        lines.append(f"  {r.name} (R = {r.R}, {kind}): cycle starts at position {p0}{' [' + c0 + ']' if c0 else ''}, "
                     f"this call at position {p1}{' [' + c1 + ']' if c1 else ''}")
    return "\n".join(lines)
