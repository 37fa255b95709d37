"""Writes tests/golden/linear/linear_container_33_65_257_1025.nam: a SlimmableContainer of four Linear models, one impulse response
recipe at 33, 65, 257 and 1,025 taps (tests/linear_oracle.py: linear_doc(R, True, seed=R)) with max_values 0.25 / 0.5 / 0.75 / 1.0 —
the fixture of cpp/tools/linear_container_check. Run from anywhere: python tests/golden/make_linear_container.py

Not under tests/golden/models, like linear_r65.nam: see make_linear_models.py."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import linear_container  # noqa: E402

if __name__ == "__main__":
    with open(linear_container.FIXTURE, "w") as f:
        json.dump(linear_container.container_doc(), f)
        f.write("\n")
    print(linear_container.FIXTURE, os.path.getsize(linear_container.FIXTURE), "bytes")
