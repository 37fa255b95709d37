#!/usr/bin/env python3
"""Which kernels the plan compiler offers each model: name, info.has_a1_kernel and the a1_valu= ... a1_p2= flags of
describe(), one line per .nam under tests/golden/models (or the files / directories named on the command line).
Host-side only: runs without a GPU. Two builds offer the same kernels when their outputs are identical."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import neuralampmodelercore_amd as nam  # noqa: E402


def main(argv):
    paths = []
    for a in argv or [os.path.join(ROOT, "tests", "golden", "models")]:
        paths += sorted(glob.glob(os.path.join(a, "**", "*.nam"), recursive=True)) if os.path.isdir(a) else [a]
    for p in paths:
        name = os.path.splitext(os.path.basename(p))[0]
        try:
            m = nam.get_dsp(p)
        except Exception as e:  # a fixture that is meant not to load
            print(f"{name}: {type(e).__name__}")
            continue
        flags = " | ".join(f.group(0) for f in re.finditer(r"a1_valu=\S+.*?a1_p2=\S+", m.describe()))
        print(f"{name}: has_a1_kernel={m.info.has_a1_kernel} {flags}")


if __name__ == "__main__":
    main(sys.argv[1:])
