#!/bin/bash
# The host sources with AddressSanitizer + UBSan, linked with profiles/bank_families/bank_host_check.cpp into an ordinary
# executable (the kernels' objects come from the normal build: make -C neuralampmodelercore_amd/csrc first), run on the CPU:
# three members per family accepted, one set per family refused. Nothing is loaded into Python; no device is needed.
set -e
cd "$(dirname "$0")/../.."
OUT=${1:-build/bank_host_check}
mkdir -p "$OUT"
for f in nam_hip_api api_launch api_session api_host_io api_bank nam_loader plan plan_ops plan_a1 plan_wr wr_jit; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
    -x hip -c -o "$OUT/$f.o" neuralampmodelercore_amd/csrc/$f.cpp &
done
wait
/opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c -o "$OUT/main.o" profiles/bank_families/bank_host_check.cpp
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o "$OUT/bank_host_check" \
  "$OUT"/*.o neuralampmodelercore_amd/lib/obj/kernel_*.o
python - "$OUT" <<'PY'
import sys
sys.path.insert(0, "tests")
from bank_models import write_a2, write_lstm, write_standard
d = sys.argv[1]
write_a2(f"{d}/a2_a.nam", 401)
write_a2(f"{d}/a2_b.nam", 402)
write_lstm(f"{d}/lstm_a.nam", 511)
write_lstm(f"{d}/lstm_b.nam", 512)
write_lstm(f"{d}/lstm_h4.nam", 521, hidden=4)
write_standard(f"{d}/std_a.nam", 101)
PY
G=tests/golden/models
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/bank_host_check" \
  --accept $G/wavenet_a1_standard.nam $G/synth_a1_lite.nam $G/synth_a1_feather.nam "$OUT/std_a.nam" \
  --accept $G/A2.nam "$OUT/a2_a.nam" "$OUT/a2_b.nam" \
  --accept $G/lstm.nam "$OUT/lstm_a.nam" "$OUT/lstm_b.nam" \
  --refuse $G/wavenet_a1_standard.nam $G/synth_a1_lite.nam $G/lstm.nam \
  --refuse $G/A2.nam "$OUT/a2_a.nam" $G/wavenet_a1_standard.nam \
  --refuse $G/lstm.nam "$OUT/lstm_a.nam" "$OUT/lstm_h4.nam" \
  --refuse $G/synth_a1_nano.nam
echo "exit status $?"
