"""csrc/linear_worklist.h on the CPU: tests/src/linear_worklist_check.cpp built with AddressSanitizer + UBSan into an ordinary
executable (nothing preloaded, no device) — the (column tile, submodel) pairs of an all-Linear container's batch, the per-column pair
index, the grid extents and the partial-sum size for every kind of assignment at 1, 32, 33 and 70 streams, against what batch creation
allocates."""
import os
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_linear_worklist_under_sanitizers(tmp_path):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "linear_worklist_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "neuralampmodelercore_amd", "csrc"), "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "linear_worklist_check.cpp")], check=True, timeout=60)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "linear_worklist_check: ok" in r.stdout
