#!/usr/bin/env python3
"""Developer tool: the instruction census of nam_a1_q_kernel<ACT_FASTTANH, false, true, false> (the session instantiation the
benchmark's flagship runs) by STAGE, from its gfx950 listing — no GPU needed.

    python tools/isa_census_a1q.py [--listing k.s] [--keep k.s] > profiles/valu_diet/census_after.txt

Without --listing the kernel file is compiled to a listing first (hipcc -S -DNAM_AQ_PROBE: that one instantiation only).
A stage is found by its steady loop: the innermost loop that holds matrix instructions (a big stage's 16-frame sub-block, which
runs four times per buffer; a small stage's buffer) together with the per-buffer loop around it. Per stage and buffer the tool
prints the instructions by class, splits the vector ones into math (fp32 arithmetic, |x| masks, reciprocals) and the rest, and
sums them per SIMD (a workgroup's sixteen stages share four SIMDs), which is what the counters SQ_INSTS_VALU - SQ_INSTS_MFMA
give per SIMD and step. The listing is static: a wait on a hand-over word counts as ONE look (the hardware counts every look),
and blocks that run for few sub-blocks only (a ring's second copy of mirrored rows, a far ring's rows across its end, a ragged
buffer, the exit token) are listed apart as `rare` and weighted by how often they run (see RARE below)."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "neuralampmodelercore_amd", "csrc", "kernel_a1_q.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-DNAM_AQ_PROBE", "--cuda-device-only", "-S"]
CLASSES = ["mfma", "trans", "valu_math", "valu_other", "lds", "vmem", "salu", "wait"]
TRANS = ("v_rcp", "v_exp", "v_log", "v_rsq", "v_sqrt", "v_sin", "v_cos")
MATH = re.compile(r"^v_(pk_)?(fma|fmac|fmaak|fmamk|mul|add|sub|mac|mad)_(legacy_)?f32")


def classify(text):
    op = text.split()[0]
    if op.startswith(("v_mfma", "v_smfma")):
        return "mfma"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_"):
        if MATH.match(op) or (op.startswith("v_and_b32") and "0x7fffffff" in text):
            return "valu_math"
        return "valu_other"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_setprio")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return None


def parse(lines):
    """[(line number, 'label' | 'inst', text)] of the kernel's body"""
    items = []
    for i, l in enumerate(lines, 1):
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            items.append((i, "label", m.group(1)))
            continue
        if not t or t.startswith((";", "//", ".")) or re.match(r"^\d+:$", t) or t.endswith(":"):
            continue
        if re.match(r"^[a-z_0-9]+$", t.split()[0]):
            items.append((i, "inst", t))
    return items


def blocks_of(items):
    """basic blocks [(first line, last line, label or None)]: a label or the instruction behind a branch starts one"""
    out, cur, lab = [], None, None
    for i, k, t in items:
        if k == "label":
            if cur:
                out.append((cur[0], cur[1], lab))
            cur, lab = None, t
            continue
        cur = (cur[0], i) if cur else (i, i)
        if re.match(r"^s_(cbranch|branch|endpgm)", t) and ".LBB" in t + ".LBB":
            out.append((cur[0], cur[1], lab))
            cur, lab = None, None
    if cur:
        out.append((cur[0], cur[1], lab))
    return out


def count(items, a, b, skip=()):
    c = dict.fromkeys(CLASSES, 0)
    for i, k, t in items:
        if k == "inst" and a <= i <= b and not any(x <= i <= y for x, y in skip):
            cl = classify(t)
            if cl:
                c[cl] += 1
    return c


def loops_of(items):
    label_line = {t: i for i, k, t in items if k == "label"}
    loops = set()
    for i, k, t in items:
        if k == "inst":
            m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
            if m and label_line.get(m.group(1), 1 << 30) < i:
                loops.add((label_line[m.group(1)], i))
    return sorted(loops)


# RARE: a forward-skipped block inside a steady loop that holds one of these runs for few sub-blocks only
def rare_ranges(items, a, b):
    """Line ranges inside [a, b] that a conditional FORWARD branch jumps over and that hold a per-lane wrap (v_min_u32 after an add:
    rows across a ring's end), a v_cndmask (the second copy of mirrored rows, a ragged buffer's row mask) — the steady path of a
    session has none of these — or that end the loop (the exit token: a block that leaves the loop)."""
    label_line = {t: i for i, k, t in items if k == "label"}
    out = []
    for i, k, t in items:
        if k != "inst" or not (a <= i <= b):
            continue
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)", t)
        if not m or m.group(1) not in label_line:
            continue
        tgt = label_line[m.group(1)]
        if not (i < tgt <= b) or tgt - i > 40:
            continue
        body = [x for j, kk, x in items if kk == "inst" and i < j < tgt]
        if any(x.startswith(("v_min_u32", "v_cndmask")) for x in body) and not any(x.startswith("v_mfma") for x in body):
            out.append((i + 1, tgt - 1))
    return out


def main():
    args = sys.argv[1:]
    listing = args[args.index("--listing") + 1] if "--listing" in args else None
    keep = args[args.index("--keep") + 1] if "--keep" in args else None
    if not listing:
        listing = keep or os.path.join(tempfile.mkdtemp(), "kernel_a1_q.s")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc] + FLAGS + ["-o", listing, SRC], stderr=subprocess.DEVNULL)
    lines = open(listing).read().splitlines()
    items = parse(lines)
    loops = loops_of(items)
    cnt = {l: count(items, *l) for l in loops}
    with_m = [l for l in loops if cnt[l]["mfma"] > 0 and cnt[l]["mfma"] <= 300]  # (the dispatch over the stages closes "loops" around everything)
    leaves = [l for l in with_m if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in with_m)]
    stages = []
    for leaf in leaves:
        # the per-buffer loop: the widest loop around the leaf that holds no other leaf
        outer = [o for o in with_m if o[0] <= leaf[0] and leaf[1] <= o[1] and not any(x != leaf and o[0] <= x[0] and x[1] <= o[1] for x in leaves)]
        per_buffer = min(outer, key=lambda o: (o[0], -o[1]))
        stages.append((leaf, per_buffer))
    # leaves of one per-buffer loop (the transition's and its layer's) are one stage
    by_buf = {}
    for leaf, pb in stages:
        by_buf.setdefault(pb, []).append(leaf)
    meta = {}
    for key in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".agpr_count"):
        for l in lines:
            m = re.match(r"^\s*" + re.escape(key) + r":\s*(\d+)", l)
            if m:
                meta[key] = int(m.group(1))
    print("nam_a1_q_kernel<ACT_FASTTANH, false, true, false> (gfx950): instructions per stage and 64-frame buffer, from the listing")
    print("code object: " + ", ".join(f"{k} {v}" for k, v in meta.items()))
    print("kind  lines            x/buf " + " ".join(f"{c:>10s}" for c in CLASSES) + "   rare(valu)")
    tot = dict.fromkeys(CLASSES, 0.0)
    tot_rare = 0.0
    n_big = n_small = 0
    for pb in sorted(by_buf):
        lv = sorted(by_buf[pb])
        big = len(lv) == 1 and cnt[lv[0]]["mfma"] == 16
        if big:
            leaf = lv[0]
            rare = rare_ranges(items, *pb)
            steady_leaf = count(items, *leaf, skip=rare)
            steady_pb = count(items, *pb, skip=rare)
            per = {c: 4 * steady_leaf[c] + (steady_pb[c] - steady_leaf[c]) for c in CLASSES}
            rv = sum(sum(count(items, x, y)[c] for c in ("valu_math", "valu_other", "trans")) for x, y in rare if leaf[0] <= x and y <= leaf[1])
            n_big += 1
            kind, rep = "big", 4
        else:
            rare = rare_ranges(items, *pb)
            per = count(items, *pb, skip=rare)
            rv = sum(sum(count(items, x, y)[c] for c in ("valu_math", "valu_other", "trans")) for x, y in rare)
            n_small += 1
            kind, rep = "small", 1
        for c in CLASSES:
            tot[c] += per[c]
        tot_rare += rv * rep
        print(f"{kind:5s} {pb[0]:6d}-{pb[1]:<6d}  {rep:5d} " + " ".join(f"{per[c]:10d}" for c in CLASSES) + f"   {rv:4d} x{rep} (static, not in the sums)")
    print(f"stages found: {n_big} big + {n_small} small (the kernel has 10 + 6)")
    print("sum   per workgroup and buffer " + " ".join(f"{tot[c]:10.0f}" for c in CLASSES))
    valu = tot["trans"] + tot["valu_math"] + tot["valu_other"]
    print(f"MFMA per workgroup and buffer: {tot['mfma']:.0f}  (the counters' SQ_INSTS_MFMA: 1336.2; the last layer's 1x1 is dead code: 10 x 64 + 5 x 128 + 56)")
    print(f"non-MFMA vector instructions per SIMD and buffer, steady path: {valu / 4:.1f}"
          f"  = math {(tot['trans'] + tot['valu_math']) / 4:.1f} + other {tot['valu_other'] / 4:.1f}")
    print(f"  rare blocks, if every one ran every time: + {tot_rare / 4:.1f} per SIMD and buffer")
    print("  (counters: SQ_INSTS_VALU - SQ_INSTS_MFMA per SIMD and step counts every look of a wait, the census one per wait)")


if __name__ == "__main__":
    main()
