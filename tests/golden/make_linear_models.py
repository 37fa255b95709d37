"""Writes tests/golden/linear/linear_r65.nam: the Linear fixture of cpp/tools/linear_check's test, from the recipe of
tests/linear_oracle.py (linear_doc(65, bias=True, seed=65)). Run from anywhere: python tests/golden/make_linear_models.py

Not under tests/golden/models: tests/test_reference_build.py runs every *.nam there through the reference build of oracle/_ref,
which leaves NAM/linear.cpp out (it needs Eigen's FFT)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import linear_oracle  # noqa: E402

FIXTURES = {"linear_r65": dict(R=65, bias=True, seed=65)}

if __name__ == "__main__":
    for name, kw in FIXTURES.items():
        path = os.path.join(HERE, "linear", name + ".nam")
        with open(path, "w") as f:
            json.dump(linear_oracle.linear_doc(**kw), f)
            f.write("\n")
        print(path)
