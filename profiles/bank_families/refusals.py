"""Every bank the three host-side test files (tests/test_bank_abi.py, test_bank_a2_abi.py, test_bank_lstm_abi.py) expect to be
refused, built against the checkout given as argument; prints the full nam_hip_last_error text of each. No device needed
(nam_hip_bank_create is host-only). The outputs of two checkouts are compared with diff.
    python profiles/bank_families/refusals.py CHECKOUT_ROOT"""
import importlib
import os
import sys
import tempfile

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import neuralampmodelercore_amd as nam  # noqa: E402


def writer(name, *modules):
    for m in modules:
        try:
            return getattr(importlib.import_module(m), name)
        except (ImportError, AttributeError):
            pass
    raise SystemExit(f"no {name}")


write_standard = writer("write_standard", "bank_models")
write_a2 = writer("write_a2", "bank_models_a2", "bank_models")
write_lstm = writer("write_lstm", "bank_models_lstm", "bank_models")
tmp = tempfile.mkdtemp()
count = [0]


def fx(name, fast_tanh=True, **kw):
    return nam.get_dsp(os.path.join(root, "tests", "golden", "models", name + ".nam"), fast_tanh=fast_tanh, **kw)


def seeded(write, seed, fast_tanh=True, luts=None, **kw):
    count[0] += 1
    p = os.path.join(tmp, f"m{count[0]}.nam")
    write(p, seed, **kw)
    return nam.get_dsp(p, fast_tanh=fast_tanh, luts=luts)


def refused(label, models):
    try:
        nam.ModelBank(models)
        print(f"{label}: ACCEPTED")
    except nam.NamHipError as e:
        print(f"{label}: [{e.code}] {e}")


std, a2, lstm = fx("wavenet_a1_standard"), fx("A2"), fx("lstm")
LUT = {"Tanh": (-5.0, 5.0, 1024)}
# tests/test_bank_abi.py
refused("a1 std+lstm", [std, lstm])
refused("a1 std+nano", [std, fx("synth_a1_nano")])
refused("a1 std+std+feather_relu", [std, std, fx("synth_a1_feather_relu")])
refused("a1 feather_relu+std", [fx("synth_a1_feather_relu"), std])
refused("a1 std+slimmable", [std, fx("slimmable_wavenet")])
refused("a1 std+A2", [std, a2])
refused("a1 std+seeded tanh", [std, seeded(write_standard, 103, fast_tanh=False)])
refused("a1 std tanh+lut", [fx("wavenet_a1_standard", False), fx("wavenet_a1_standard", False, luts=LUT)])
# tests/test_bank_a2_abi.py
s330 = seeded(write_a2, 330)
refused("a2 A2+std", [a2, std])
refused("a2 std+A2", [std, a2])
refused("a2 seeded+seeded+std", [s330, s330, std])
refused("a2 A2+lstm", [a2, lstm])
refused("a2 leaky+tanh", [s330, seeded(write_a2, 331, act="Tanh")])
refused("a2 tanh+leaky", [seeded(write_a2, 332, act="Tanh"), s330])
refused("a2 fasttanh+tanh", [seeded(write_a2, 333, act="Tanh"), seeded(write_a2, 334, fast_tanh=False, act="Tanh")])
refused("a2 leaky+relu", [s330, seeded(write_a2, 335, act="ReLU")])
refused("a2 A2+sigmoid", [a2, seeded(write_a2, 336, act="Sigmoid")])
refused("a2 sigmoid", [seeded(write_a2, 336, act="Sigmoid")])
lut = seeded(write_a2, 337, fast_tanh=False, luts=LUT, act="Tanh")
refused("a2 tanh+lut", [seeded(write_a2, 338, fast_tanh=False, act="Tanh"), lut])
refused("a2 lut", [lut])
refused("a2 A2+kt_c8", [a2, fx("synth_kt_c8")])
refused("a2 kt_c8+A2", [fx("synth_kt_c8"), a2])
refused("a2 A2+slimmable", [a2, fx("slimmable_wavenet")])
refused("a2 A2+nano", [a2, fx("synth_a1_nano")])
# tests/test_bank_lstm_abi.py
s520 = seeded(write_lstm, 520)
refused("lstm hidden 4", [lstm, s520, seeded(write_lstm, 521, hidden=4)])
refused("lstm 2 layers", [lstm, seeded(write_lstm, 522, num_layers=2)])
refused("lstm 18 vs 20", [fx("synth_lstm_h18x2"), seeded(write_lstm, 523, num_layers=2, hidden=20)])
refused("lstm fast+slow", [lstm, seeded(write_lstm, 524, fast_tanh=False)])
refused("lstm slow+fast", [fx("lstm", False), s520])
refused("lstm 44100", [lstm, seeded(write_lstm, 525, sample_rate=44100)])
refused("lstm +hidden 40", [lstm, seeded(write_lstm, 526, hidden=40)])
refused("lstm hidden 40", [seeded(write_lstm, 526, hidden=40)])
refused("lstm lstm+std", [lstm, std])
refused("lstm std+lstm", [std, lstm])
refused("lstm A2+lstm", [a2, lstm])
refused("lstm lstm+seeded+A2", [lstm, s520, a2])
# accepted sets, for contrast (the ABI tests' accepting cases in short)
for label, models in (("a1", [std, fx("synth_a1_lite"), fx("synth_a1_feather")]), ("a2", [a2, s330]), ("lstm", [lstm, s520])):
    print(f"accepted {label}: {len(nam.ModelBank(models))} members")
