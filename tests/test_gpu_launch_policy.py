"""launch_wr hands the batch's own figures to csrc/launch_policy.h (tests/test_launch_policy.py checks the rule itself on the CPU):
the parity and bit-for-bit tests hold for any stage count, so a wrong field there would pass all of them. NAM_HIP_SESSION_STATS=1
makes launch_wr say what a multi-buffer launch of nam_wn_reg_kernel runs as; the switch is read once per process, so every case is a
process of its own. The lines are the parent commit's (profiles/launch_policy/README.md), and the first is the project's GPU record
for this model (profiles/bank_wn_reg/forms_by_stream_count.txt: nano, 12 streams, 4 stages, 104,176 bytes)."""
import os
import subprocess
import sys

import pytest

from bank_wr_models import NANO_SEEDS, write_nano
from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
         "import numpy as np\n"
         "import neuralampmodelercore_amd as nam\n"
         "from bank_harness import BLOCK, drive\n"
         "nam.load_library()\n"
         "b = nam.get_dsp(%r, fast_tanh=True).batch(12, 4 * BLOCK)\n"
         "b.Reset(prewarm=False)\n"
         "x = (0.3 * np.random.default_rng(941).standard_normal((12, 1, 4 * BLOCK))).astype(np.float32)\n"
         "y, name = drive(b, x, 'launch')\n"
         "b.close()\n"
         "assert name == 'nam_wn_reg_kernel' and np.isfinite(y).all() and np.abs(y).max() > 0, name\n"
         "print('launched')\n")


@pytest.mark.parametrize("max_stages,line", [
    (None, "12 workgroups as 4 wavefront(s) per stream, 104176 bytes of LDS each"),
    (2, "12 workgroups as 2 wavefront(s) per stream, 83568 bytes of LDS each"),
    (1, None)])
def test_launch_wr_reports_the_policys_shape(tmp_path, max_stages, line):
    """Twelve streams of member 0 of the nano set, one plain launch of 256 frames."""
    path = str(tmp_path / "nano.nam")
    write_nano(path, NANO_SEEDS[0])
    env = {k: v for k, v in os.environ.items() if k != "NAM_HIP_MAX_STAGES"}
    env["NAM_HIP_SESSION_STATS"] = "1"
    if max_stages:
        env["NAM_HIP_MAX_STAGES"] = str(max_stages)
    code = CHILD % (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle"), path)
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "launched" in r.stdout, r.stdout + r.stderr
    print(r.stderr)
    said = [ln for ln in r.stderr.splitlines() if ln.startswith("nam_hip nam_wn_reg_kernel:")]
    assert said == (["nam_hip nam_wn_reg_kernel: " + line] if line else []), r.stderr
