"""Two `hipcc -S --cuda-device-only` listings of kernel_wn_reg.hip, kernel by kernel, as OPCODE sequences (operands dropped: a new
scalar in the prologue renumbers registers all the way down): how many instructions each form has, in how many places the two
sequences differ and where the first and last of them lie, and the net change by opcode.

    python profiles/bank_wn_reg/opcode_compare.py old/kernel_wn_reg.s new/kernel_wn_reg.s      (the ahead-of-time kernels)
    python profiles/bank_wn_reg/opcode_compare.py old/jit_nano.s new/jit_nano.s                (a per-model listing)"""
import collections
import difflib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w*nam_wn_reg\w*|nam_wn_reg_jit\w*):\s", line)
        if m:
            name, body = m.group(1), []
            continue
        if name:
            if line.strip().startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                body.append(t.split()[0])
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    for name, a in old.items():
        b = new[name]
        hunks = [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]
        rem, add = collections.Counter(), collections.Counter()
        for _, i1, i2, j1, j2 in hunks:
            rem.update(a[i1:i2])
            add.update(b[j1:j2])
        net = {k: add[k] - rem[k] for k in sorted(set(add) | set(rem)) if add[k] != rem[k]}
        where = f"first at instruction {hunks[0][1]}, last at {hunks[-1][1]}" if hunks else "-"
        print(f"{name}: {len(a)} -> {len(b)} instructions; {len(hunks)} differing places ({where}), {sum(rem.values())} removed / "
              f"{sum(add.values())} added; net by opcode: {net}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
