"""Are the one-model instantiations of the kernels that run model banks the same code before and after the BANK template
parameter? Compares two sets of `hipcc -S --cuda-device-only` listings (same flags as csrc/Makefile), kernel by kernel: the
body of every kernel of the OLD listing against the kernel of the NEW listing of the same name, or — where the new tree added
the parameter — whose name is the old one plus a trailing `false` template argument (BANK). Basic-block label numbers and the
kernel's own name are normalised; what remains different is printed. Under the summary line of every listing: one line per
kernel template (how many of the old instantiations are identical line for line, and the set of line pairs the others differ
in), and what the new listing adds.

    hipcc <flags> --cuda-device-only -S -o old/kernel_kq.s <old tree>/kernel_kq.hip     (and the others; then the new tree)
    python tools/isa_compare_instantiations.py old/ new/ [kernel_kq kernel_kt_mfma ...]

Without a list: the interleaved-frame kernels (kernel_a1_q, kernel_a1_p4, kernel_a1_p2: the A1 bank family), the A2 family's
(kernel_kq, kernel_kt_mfma) and the LSTM family's (kernel_lstm), as far as both directories hold their listings.
"""
import os
import re
import sys

DEFAULT = ("kernel_a1_q", "kernel_a1_p4", "kernel_a1_p2", "kernel_kq", "kernel_kt_mfma", "kernel_lstm")


def twin_of(name):
    """the mangled name with one more template argument `false`: ...<args> E E v <parameters> -> ...<args> Lb0E E E v ..."""
    i = name.index("EEvPK")
    return name[:i] + "Lb0E" + name[i:]


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and "_kernel" in m.group(1) and "nam_" in m.group(1):
            name, body = m.group(1), []
            continue
        if name:
            if line.strip().startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            text = line.split(";")[0].rstrip()
            if text.strip():
                body.append(text)
    return out


def base_name(mangled):
    """the kernel's plain name out of the mangled one: ...19nam_lstm_row_kernelILi1E... -> nam_lstm_row_kernel"""
    m = re.search(r"(\d+)nam_", mangled)  # (behind the namespaces' names, each with its length in front)
    return mangled[m.end(1):m.end(1) + int(m.group(1))]


def main(old_dir, new_dir, names=()):
    rc = 0
    for k in names or DEFAULT:
        if not names and not (os.path.exists(os.path.join(old_dir, k + ".s")) and os.path.exists(os.path.join(new_dir, k + ".s"))):
            continue
        old, new = kernels(os.path.join(old_dir, k + ".s")), kernels(os.path.join(new_dir, k + ".s"))
        norm = lambda l, n: re.sub(r"\.LBB\d+_", ".LBB_", l.replace(n, "K"))
        same, kernarg_only, other = 0, 0, []
        per = {}  # kernel template -> [instantiations, identical ones, the line pairs the others differ in]
        twins = set()
        for name, body in old.items():
            twin = name if name in new else twin_of(name)
            row = per.setdefault(base_name(name), [0, 0, set()])
            row[0] += 1
            twins.add(twin)
            if twin not in new:
                other.append((name, "no such kernel in the new listing"))
                continue
            a, b = [norm(l, name) for l in body], [norm(l, twin) for l in new[twin]]
            diffs = [(x, y) for x, y in zip(a, b) if x != y]
            if len(a) != len(b):
                other.append((name, f"{len(a)} vs {len(b)} lines"))
            elif not diffs:
                same += 1
                row[1] += 1
            elif all("amdhsa_kernarg_size" in x or re.match(r"\s*s_add_u32 s\d+, s\d+, 0x[0-9a-f]+$", x) for x, _ in diffs):
                row[2].update((x.strip(), y.strip()) for x, y in diffs)
                kernarg_only += 1  # the size of the argument block / the offset of the implicit arguments behind it
            else:
                other.append((name, diffs[:4]))
        print(f"{k}: {len(old)} one-model instantiations, {len(new) - len(old)} new (BANK) ones; identical {same}, "
              f"identical but for the kernel-argument size / the implicit arguments' offset {kernarg_only}, different {len(other)}")
        for base, (n, ident, pairs) in sorted(per.items()):
            print(f"  {base}: {n} instantiations in the old listing, {ident} identical line for line, "
                  f"{n - ident} differing only in: {sorted(pairs)}")
        added = {}
        for name in new:
            if name not in twins:
                added[base_name(name)] = added.get(base_name(name), 0) + 1
        print("  new: " + (", ".join(f"{c} of {b}" for b, c in sorted(added.items())) or "none"))
        for o in other:
            print("   ", o)
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
