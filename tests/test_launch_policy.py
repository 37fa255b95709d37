"""csrc/launch_policy.h on the CPU: tests/src/launch_policy_check.cpp built with AddressSanitizer + UBSan into an ordinary executable
(nothing preloaded, no device) — nam_wn_reg_kernel's wavefronts per stream, dense forms and LDS at every stream count where the
answer changes (257, 513, 769, 1,025, 1,793 ... on 256 CUs: no GPU test runs that many streams), the occupancy rule and the stream
bound of pick_kernel / persist_kind."""
import os
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_launch_policy_table_under_sanitizers(tmp_path):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "launch_policy_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "neuralampmodelercore_amd", "csrc"), "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "launch_policy_check.cpp")], check=True, timeout=60)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "launch_policy_check: ok" in r.stdout
