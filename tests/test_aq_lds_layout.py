"""The LDS layout of nam_a1_q_kernel (csrc/aq_table.h) — no GPU: the table is plain constexpr C++, so a host program prints it
and the checks are made here. What must hold: everything fits the 160 KB of a CDNA4 workgroup; the regions (weight block, words,
slots, every job's input area) follow each other without overlap; a big layer's resident ring is followed by the mirror of its
first 15 rows, which lies behind the ring's R live rows (the only rows that go back into the stream state) and inside the ring's
own plane, so that sixteen rows from any position p < R are addressable as p + n without a wrap."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuralampmodelercore_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "aq_table.h"
using namespace namhip::aq;
int main()
{
  std::printf("lds %d wb %d flags %d slots %d in0 %d mirror %d\n", kLdsBytes, kWB, kFlagB, kSlotB0, kInB0, kMirror);
  for (int b = 0; b < kNst - 1; b++)
    std::printf("slot %d %d %d\n", b, slot_b(b), slot_bytes(b));
  for (int j = 0; j < kJobs; j++)
    std::printf("job %d big %d small %d res %d ring_len %d mirror_rows %d in_rows %d plane_b %d in_b %d in_bytes %d chans %d\n", j, (int)is_big(j),
                (int)is_small(j), (int)res(j), has_ring(j) ? ring_len(j) : 0, mirror_rows(j), in_rows(j), plane_b(j), in_b(j), in_bytes(j), chans(j));
  return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to evaluate aq_table.h")
    d = tmp_path_factory.mktemp("aq_layout")
    src = d / "layout.cpp"
    src.write_text(PROGRAM)
    exe = d / "layout"
    subprocess.check_call([cxx, "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    head, slots, jobs = None, [], []
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        w = line.split()
        if w[0] == "lds":
            head = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
        elif w[0] == "slot":
            slots.append({"b": int(w[1]), "at": int(w[2]), "bytes": int(w[3])})
        else:
            jobs.append({w[i]: int(w[i + 1]) for i in range(0, len(w), 2)})
    return head, slots, jobs


def test_layout_fits_a_workgroup(layout):
    head, _, _ = layout
    assert head["lds"] <= 160 * 1024


def test_regions_follow_each_other(layout):
    head, slots, jobs = layout
    assert head["wb"] == 0 and head["flags"] > 0 and head["slots"] == head["flags"] + 256
    at = head["slots"]
    for s in slots:
        assert s["at"] == at and s["bytes"] > 0 and s["at"] % 16 == 0
        at += s["bytes"]
    assert head["in0"] >= at
    at = head["in0"]
    for j in jobs:
        assert j["in_b"] == at and j["in_b"] % 16 == 0
        assert j["in_bytes"] == j["plane_b"] * (j["chans"] // 4)
        assert j["plane_b"] >= j["in_rows"] * 16
        at += j["in_bytes"]
    assert at == head["lds"]


def test_mirrors_lie_behind_the_live_rows(layout):
    head, _, jobs = layout
    assert head["mirror"] == 15  # sixteen rows from any position: at most fifteen beyond the ring's end
    mirrored = [j for j in jobs if j["mirror_rows"]]
    assert [j["job"] for j in mirrored] == [j["job"] for j in jobs if j["big"] and j["res"]] and len(mirrored) == 7
    for j in mirrored:
        R = j["ring_len"]
        live = range(0, R)  # the rows ring_to_lds / lds_to_ring move: exactly R
        mirror = range(R, R + j["mirror_rows"])
        assert j["mirror_rows"] == head["mirror"] and j["in_rows"] == R + head["mirror"]
        assert mirror[0] == live[-1] + 1  # behind the live rows, not among them
        assert mirror[-1] * 16 + 16 <= j["plane_b"]  # inside the ring's own plane: never in the next plane's live rows
        assert R >= 16 + head["mirror"]  # a sixteen-row store touches the ring's head or its end, never both
        # sixteen rows from every position stay inside live rows + mirror
        assert all(p + 15 < R + j["mirror_rows"] for p in range(R))
    for j in jobs:
        if not j["mirror_rows"]:
            assert j["in_rows"] == (j["ring_len"] if j["res"] else j["in_rows"])  # small resident rings: R rows, no mirror
