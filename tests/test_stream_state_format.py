"""csrc/stream_state.h on the CPU: tests/src/stream_state_check.cpp built with AddressSanitizer + UBSan into an ordinary executable
(nothing preloaded, no device) — the blob of nam_hip_batch_get_stream_state / set_stream_state: the encode -> validate round trip,
every refusal with the field it names, truncation at every length (each on a heap block of exactly that length), flipped bytes, and
the Linear ring's rotation for every (source position, destination position) of a 7-row and of an 896-row ring against a plain
modular restatement."""
import os
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_stream_state_format_under_sanitizers(tmp_path):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    exe = str(tmp_path / "stream_state_check")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "neuralampmodelercore_amd", "csrc"), "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "src", "stream_state_check.cpp")], check=True, timeout=60)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream_state_check: ok" in r.stdout
