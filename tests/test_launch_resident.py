"""csrc/launch_policy.h on the CPU: tests/src/launch_resident_check.cpp built with AddressSanitizer + UBSan into an ordinary
executable (nothing preloaded, no device) — launch_all_resident / wr_all_resident, the rule by which a session's launch of
nam_wn_reg_kernel, nam_lstm_row_kernel or nam_lstm_wide_kernel may linger for its next command: every workgroup on the chip at
once. The values at the documented bounds (1,024 / 1,025 one-wave workgroups on 256 CUs, the LDS steps of the occupancy rule, the
LSTM kernels' four per CU), monotone in the workgroup count, and agreement with wr_stream_bound and wr_launch_shape's turns."""
import os
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_launch_resident_rule_under_sanitizers(tmp_path):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "launch_resident_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "neuralampmodelercore_amd", "csrc"), "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "launch_resident_check.cpp")], check=True, timeout=60)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "launch_resident_check: ok" in r.stdout
