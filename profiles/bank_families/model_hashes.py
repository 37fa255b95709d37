"""SHA-256 of every file the bank model writers produce for the (seed, keyword) combinations the tests and tools/bank_bench.py
use. Run with the tests directory of a checkout as argument; the outputs of two checkouts are compared with diff.
    python profiles/bank_families/model_hashes.py TESTS_DIR"""
import hashlib
import importlib
import os
import sys
import tempfile

sys.path.insert(0, sys.argv[1])


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

A1 = [(s, {}) for s in (101, 102, 103, 104, 105, 200, 201, 202)] + [(1000 + i, {}) for i in range(256)]
A2 = ([(s, {}) for s in (301, 302, 330, 340, 341, 342, 343, 401, 402, 403, 404, 405, 406, 407, 461, 462)]
      + [(s, dict(act="Tanh")) for s in (310, 311, 331, 332, 333, 334, 337, 338)] + [(s, dict(act="ReLU")) for s in (320, 321, 335)]
      + [(336, dict(act="Sigmoid"))]
      + [(450, kw) for kw in (dict(head_scale=0.05, slope=0.01), dict(head_scale=0.05, slope=0.2), dict(head_scale=0.07, slope=0.01))]
      + [(1000 + i, {}) for i in range(256)])
SHAPES = [dict(num_layers=1, input_size=1, hidden=3, out_channels=1), dict(num_layers=2, input_size=1, hidden=4, out_channels=1),
          dict(num_layers=2, input_size=1, hidden=18, out_channels=1), dict(num_layers=2, input_size=2, hidden=24, out_channels=2)]
LSTM = ([(700 + 10 * i + j, kw) for i, kw in enumerate(SHAPES) for j in (0, 1)]
        + [(s, dict(kw, **extra)) for kw in (SHAPES[0], SHAPES[2]) for s, extra in ((760, {}), (760, dict(state_seed=1)), (761, {}))]
        + [(s, {}) for s in (771, 772, 511, 512, 520, 524, 530, 531, 532, 533)]
        + [(513, dict(num_layers=2, hidden=18)), (521, dict(hidden=4)), (522, dict(num_layers=2)), (523, dict(num_layers=2, hidden=20)),
           (525, dict(sample_rate=44100)), (526, dict(hidden=40))]
        + [(2000 + i, dict(num_layers=1, input_size=1, hidden=3, out_channels=1)) for i in range(1024)]
        + [(2000 + i, dict(num_layers=1, input_size=1, hidden=24, out_channels=1)) for i in range(256)])

with tempfile.TemporaryDirectory() as d:
    p = os.path.join(d, "m.nam")
    for name, write, cases in (("write_standard", write_standard, A1), ("write_a2", write_a2, A2), ("write_lstm", write_lstm, LSTM)):
        every = hashlib.sha256()
        for seed, kw in cases:
            write(p, seed, **kw)
            h = hashlib.sha256(open(p, "rb").read()).hexdigest()
            every.update(h.encode())
            print(f"{name}({seed}{''.join(f', {k}={v}' for k, v in kw.items())}) {h}")
        print(f"{name}: {len(cases)} files, sha256 over their hashes {every.hexdigest()}")
