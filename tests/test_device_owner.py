"""csrc/device_owner.h on the CPU: tests/src/owner_check.cpp built with AddressSanitizer + UBSan into an ordinary executable
(nothing preloaded, no device) — the move-only rules every owner of the host runtime relies on, and leak detection over them."""
import os
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_owner_rules_under_sanitizers(tmp_path):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "owner_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "owner_check.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, timeout=60)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "owner_check: ok" in r.stdout
