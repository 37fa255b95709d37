"""Are the one-model instantiations of the kernels that run model banks the same code before and after the BANK template
parameter? Compares two sets of `hipcc -S --cuda-device-only` listings (same flags as csrc/Makefile), kernel by kernel: the
body of every kernel of the OLD listing against the kernel of the NEW listing of the same name, or — where the new tree added
the parameter — whose name is the old one plus a trailing `false` template argument (BANK). Basic-block label numbers and the
kernel's own name are normalised; what remains different is printed.

    hipcc <flags> --cuda-device-only -S -o old/kernel_kq.s <old tree>/kernel_kq.hip     (and the others; then the new tree)
    python tools/isa_compare_instantiations.py old/ new/ [kernel_kq kernel_kt_mfma ...]

Without a list: the interleaved-frame kernels (kernel_a1_q, kernel_a1_p4, kernel_a1_p2: the A1 bank family) and the A2 family's
(kernel_kq, kernel_kt_mfma), as far as both directories hold their listings.
"""
import os
import re
import sys

DEFAULT = ("kernel_a1_q", "kernel_a1_p4", "kernel_a1_p2", "kernel_kq", "kernel_kt_mfma")


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


def main(old_dir, new_dir, names=()):
    rc = 0
    for k in names or DEFAULT:
        if not names and not (os.path.exists(os.path.join(old_dir, k + ".s")) and os.path.exists(os.path.join(new_dir, k + ".s"))):
            continue
        old, new = kernels(os.path.join(old_dir, k + ".s")), kernels(os.path.join(new_dir, k + ".s"))
        norm = lambda l, n: re.sub(r"\.LBB\d+_", ".LBB_", l.replace(n, "K"))
        same, kernarg_only, other = 0, 0, []
        for name, body in old.items():
            twin = name if name in new else twin_of(name)
            if twin not in new:
                other.append((name, "no such kernel in the new listing"))
                continue
            a, b = [norm(l, name) for l in body], [norm(l, twin) for l in new[twin]]
            diffs = [(x, y) for x, y in zip(a, b) if x != y]
            if len(a) != len(b):
                other.append((name, f"{len(a)} vs {len(b)} lines"))
            elif not diffs:
                same += 1
            elif all("amdhsa_kernarg_size" in x or re.match(r"\s*s_add_u32 s\d+, s\d+, 0x[0-9a-f]+$", x) for x, _ in diffs):
                kernarg_only += 1  # the size of the argument block / the offset of the implicit arguments behind it
            else:
                other.append((name, diffs[:4]))
        print(f"{k}: {len(old)} one-model instantiations, {len(new) - len(old)} new (BANK) ones; identical {same}, "
              f"identical but for the kernel-argument size / the implicit arguments' offset {kernarg_only}, different {len(other)}")
        for o in other:
            print("   ", o)
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
