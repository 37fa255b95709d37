"""csrc/session_command.h on the CPU: tests/src/session_command_check.cpp built into an ordinary executable, once plainly and once
with AddressSanitizer + UBSan (nothing preloaded, no device) — the session's command word for every frame count 1 .. 64, a whole
command bit for bit the word the pipeline kernels read, the split of a call of any length into commands, and the tag limit of
partial commands with what it means for the rebase mark."""
import os
import subprocess

import pytest

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_session_command_check(tmp_path, sanitize):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "session_command_check")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([CLANG, "-std=c++17", *flags, "-I" + os.path.join(ROOT, "neuralampmodelercore_amd", "csrc"), "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "session_command_check.cpp")], check=True, timeout=60)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "session_command_check: ok" in r.stdout
