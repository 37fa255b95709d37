"""The call patterns of tests/ring_phase.py reach what tests/test_gpu_ring_phase.py is there for — no GPU: plain integer arithmetic
on the schedules, with the ring lengths read from csrc/aq_table.h and csrc/kp_table.h by a host program. These are conditions
on the schedule, not measurements: a change of a table (another ring length, another resident set, a longer mirror) that the
patterns no longer cover fails here, on any machine."""
import numpy as np
import pytest

import ring_phase as rp
from conftest import model_path

FAMILIES = ("a1", "a2")


@pytest.fixture(scope="module", params=FAMILIES)
def family(request):
    rings = rp.ring_lengths(request.param)
    return request.param, rings, rp.schedule(rings, "session"), rp.schedule(rings, "launch")


def _burst_starts(calls):
    """indices of the first command of every burst"""
    return [i for i, c in enumerate(calls) if c[0] == "session" and (i == 0 or calls[i - 1][0] != "session")]


def test_ring_lengths_come_from_the_headers():
    a1, a2 = rp.ring_lengths("a1"), rp.ring_lengths("a2")
    assert len(a1) == 20 and len(a2) == 24
    # (the topologies as the headers' own comments state them: R = 2 d + 64, d = 1 .. 512, twice; (K - 1) d + 64)
    assert [r.R for r in a1] == [2 * (1 << k) + 64 for k in range(10)] * 2
    assert min(r.R for r in a2) == 69 and max(r.R for r in a2) == 1259
    assert [r.name for r in a1 if r.mirror] == [f"ring{k}" for k in range(7)] and all(r.mirror == 15 for r in a1[:7])
    assert all(r.resident for r in a1 if r.mirror) and [r.name for r in a1 if not r.resident] == ["ring7", "ring8", "ring9", "ring18", "ring19"]
    wn = rp.ring_lengths("wn_reg", model_path("wavenet_a2_max"))
    assert wn and all(r.R > rp.BLOCK and r.resident for r in wn)
    assert [r.R for r in wn if r.name.startswith("array0")] == [3 * 1 + 64, 3 * 2 + 64]


def test_session_schedule_shape(family):
    name, rings, calls, _ = family
    total = int(rp.offsets(calls)[-1])
    longest = max(r.R for r in rings)
    print(f"{name}: session schedule {len(calls)} calls, {total} frames = {total / 48000.0:.2f} s of audio; longest ring {longest}")
    bursts = _burst_starts(calls)
    assert len(bursts) == longest  # as many cycles as the longest ring has rows
    assert total == longest * 449  # one ragged frame + seven buffers per cycle: about 10 s for the official topology
    for i in bursts:
        assert calls[i - 1][0] == "ragged" and 0 < calls[i - 1][1] < rp.BLOCK
        n = 0
        while i + n < len(calls) and calls[i + n][0] == "session":
            assert calls[i + n][1] == rp.BLOCK
            n += 1
        assert n >= rp.MIN_BURST  # (shorter bursts, three in a row, would move the session to nam_a1_p4_kernel)


def test_session_bursts_start_at_every_position_of_every_ring(family):
    _, rings, calls, _ = family
    for frames_before in (0, 4096):  # (what a prewarm leaves: a translation, which coverage of ALL positions does not depend on)
        at = rp.starts(rings, calls, frames_before)[:, _burst_starts(calls)]
        for r, pos in zip(rings, at):
            assert np.array_equal(np.unique(pos), np.arange(r.R)), r


def test_session_sub_blocks_reach_every_class_of_the_mirrored_rings():
    rings = rp.ring_lengths("a1")
    calls = rp.schedule(rings, "session")
    mirrored = [r for r in rings if r.mirror]
    assert len(mirrored) == 7
    idx = [i for i, c in enumerate(calls) if c[0] == "session"]
    at = rp.starts(rings, calls)[:, idx]
    for r, pos in zip(rings, at):
        if not r.mirror:
            continue
        so = np.unique((pos[:, None] + rp.SUB * np.arange(rp.BLOCK // rp.SUB)[None, :]) % r.R)
        classes = {int(s): rp.store_class(r, int(s)) for s in so}
        head = [s for s, c in classes.items() if c == "head"]
        over = [s for s, c in classes.items() if c == "overrun"]
        assert all(s < 15 for s in head) and {0, 1, 14} <= set(head), (r, head)
        assert all(s > r.R - 16 for s in over) and {r.R - 15, r.R - 1} <= set(over), (r, over)
        assert "plain" in classes.values() and classes[15] == "plain" and classes[r.R - 16] == "plain", r
        # ... and a tap window that ends exactly on the mirror's last row, R + 14, and one that ends on the ring's last row
        taps = {t for s in so for t in rp.tap_positions(r, int(s))}
        assert {r.R - 1, r.R - 16, 0} <= taps, r


def test_session_reaches_the_fallbacks_of_the_hbm_rings():
    rings = rp.ring_lengths("a1")
    calls = rp.schedule(rings, "session")
    idx = [i for i, c in enumerate(calls) if c[0] == "session"]
    at = rp.starts(rings, calls)[:, idx]
    hbm = [r for r in rings if not r.resident]
    assert len(hbm) == 5
    for r, pos in zip(rings, at):
        if r.resident:
            continue
        so = np.unique((pos[:, None] + rp.SUB * np.arange(rp.BLOCK // rp.SUB)[None, :]) % r.R)
        for what, ts in (("append", set(int(s) for s in so)), ("taps", {t for s in so for t in rp.tap_positions(r, int(s))})):
            assert any(t + 16 > r.R for t in ts) and any(t + 16 == r.R for t in ts) and any(t + 16 < r.R for t in ts), (r, what)
            assert {r.R - 15, r.R - 1} <= ts, (r, what)  # both edges of the fallback


def test_launches_start_at_every_position_of_every_resident_ring(family):
    name, rings, _, calls = family
    total = int(rp.offsets(calls)[-1])
    print(f"{name}: launch schedule {len(calls)} calls, {total} frames = {total / 48000.0:.2f} s of audio")
    assert all(c[0] == "launch" and 2 * rp.BLOCK < c[1] < 3 * rp.BLOCK for c in calls)
    assert {c[1] - 2 * rp.BLOCK for c in calls} == set(range(1, rp.BLOCK))  # every ragged tail 1 .. 63
    resident = [r for r in rings if r.resident]
    assert resident
    for frames_before in (0, 4096):
        at = rp.starts(rings, calls, frames_before)
        for r, pos in zip(rings, at):
            if r.resident:
                assert np.array_equal(np.unique(pos), np.arange(r.R)), r
    assert len(calls) <= 3 * max(r.R for r in resident)  # (the greedy choice stays near the lower bound of one launch per row)


def test_sweep_with_every_ragged_length_for_the_register_kernel():
    """nam_wn_reg_kernel shifts its history down by the call's frames: the sweep of its case takes every ragged length 1 .. 63"""
    rings = rp.ring_lengths("wn_reg", model_path("wavenet_a2_max"))
    calls = rp.schedule(rings, "session", r=range(1, rp.BLOCK))
    assert {c[1] for c in calls if c[0] == "ragged"} == set(range(1, rp.BLOCK))
    at = rp.starts(rings, calls)[:, _burst_starts(calls)]
    for r, pos in zip(rings, at):
        assert np.array_equal(np.unique(pos), np.arange(r.R)), r
    print(f"wn_reg: session schedule {len(calls)} calls, {int(rp.offsets(calls)[-1])} frames")


def test_schedule_refuses_what_would_not_sweep():
    rings = rp.ring_lengths("a1")
    with pytest.raises(ValueError):
        rp.schedule(rings, "session", r=1, B=4)  # short bursts: another kernel
    with pytest.raises(ValueError):
        rp.schedule(rings, "session", r=2, B=7)  # advance 450: not coprime to the even ring lengths
    with pytest.raises(ValueError):
        rp.schedule(rings, "session", r=64, B=7)


def test_describe_names_cycle_position_and_class():
    rings = rp.ring_lengths("a1")
    calls = rp.schedule(rings, "session")
    off = rp.offsets(calls)
    # cycle 3's burst starts after four ragged frames and three bursts: frame 4 + 3 * 448
    f0 = 4 + 3 * 448
    assert calls[3 * 8][0] == "ragged" and int(off[3 * 8 + 1]) == f0
    text = rp.describe(rings, calls, 0, f0 + 64 + 5)
    assert "of cycle 3" in text and f"starts at frame {f0}" in text
    assert f"ring0 (R = 66, mirrored): cycle starts at position {f0 % 66}" in text
    assert f"this call at position {(f0 + 64) % 66}" in text
    # a position in a mirrored ring's head names its class; so does an HBM ring's fallback
    r0 = rings[0]
    k = next(i for i in range(len(calls)) if calls[i][0] == "session" and calls[i - 1][0] == "ragged" and int(off[i]) % r0.R == 14)
    assert "position 14 [" in rp.describe(rings, calls, 0, int(off[k])) and "head" in rp.describe([r0], calls, 0, int(off[k]))
    r9 = rings[9]
    k = next(i for i in range(len(calls)) if calls[i][0] == "session" and calls[i - 1][0] == "ragged" and int(off[i]) % r9.R == r9.R - 15)
    assert "HBM fallback" in rp.describe([r9], calls, 0, int(off[k]))
