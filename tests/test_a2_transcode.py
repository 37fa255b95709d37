"""csrc/a2_transcode.h on the CPU: tests/src/a2_transcode_check.cpp built against csrc's loader and planner, once as it is and once
with AddressSanitizer + UBSan (an ordinary executable, nothing preloaded, no device), run on tests/golden/models/A2.nam — A2-Lite's
zero-padded plan equals A2-Full's layout field by field and is zero wherever it is padded; the transcode table between
nam_wn_reg_kernel's state and the padded rings covers both, carries a state there and back at odd ring positions exactly as
kernel_a2_transcode.hip walks it, and tables that name floats outside a state or twice are refused."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "neuralampmodelercore_amd", "csrc")
A2 = os.path.join(ROOT, "tests", "golden", "models", "A2.nam")


@pytest.mark.parametrize("sanitizers", [False, True], ids=["plain", "asan_ubsan"])
def test_a2_transcode_table_and_padded_plan(tmp_path, sanitizers):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "a2_transcode_check")
    sources = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f == "nam_loader.cpp" or re.fullmatch(r"plan.*\.cpp", f)]
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitizers else []
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + ["-I" + CSRC, "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "a2_transcode_check.cpp")] + sources, check=True, timeout=600)
    env = dict(os.environ)  # (the sanitizer runtime is linked into the executable: nothing is preloaded or removed)
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe, A2], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "a2_transcode_check: ok" in r.stdout and "24 rings" in r.stdout, r.stdout
