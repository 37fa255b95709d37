"""The planner's output, pinned byte for byte on the CPU: tests/src/plan_dump.cpp built with AddressSanitizer + UBSan against
csrc's loader and plan*.cpp (an ordinary executable, nothing preloaded, no device), run over every fixture, seeded generated models
and one hand-written model, and compared with profiles/plan_wr/parent_table.txt — per model the hash of what the same program
printed at the commit before plan_wr.cpp was restructured (profiles/plan_wr/README.md: how it was recorded). What
nam_wn_reg_kernel runs, the text of the per-model header (the code-object cache key) and the structure key of a bank are
functions of these bytes.

    python tests/test_plan_pin.py [--full] CSRC_DIR > table      # the table of another csrc; --full: every line (README.md)
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_synthetic_models as msm  # noqa: E402

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "neuralampmodelercore_amd", "csrc")
MODELS = os.path.join(ROOT, "tests", "golden", "models")
TABLE = os.path.join(ROOT, "profiles", "plan_wr", "parent_table.txt")
PIN = "pin_run_and_film.nam"
CUT2_MODELS = [PIN, "synth_a1_nano.nam", "wavenet_a2_max.nam"]


def write_pin_model(path):
    """One WR_RUN and one matrix-form FiLM layer in one program, the run long enough to be cut: the model whose table lines hold the
    difference between the two cost models of plan_wr.cpp (the sub-run cutter has no discount for matrix-form FiLM weights).
    condition_dsp: a plain ReLU stack, 4 channels, 16 layers, K = 3, head size 8; main array: one layer at condition size 8,
    channels 4, bottleneck 4, K = 4, head1x1 of 4, every FiLM slot active with shift."""
    rng = np.random.default_rng(4242)

    def model(arrays, scale, cond_dsp=None):
        w = (rng.standard_normal(msm.featured_weight_count(arrays)).astype(np.float32) * np.float32(0.3)).tolist()
        w[-1] = scale
        config = dict(layers=arrays, head=None, head_scale=scale)
        if cond_dsp is not None:
            config["condition_dsp"] = cond_dsp
        return dict(version="0.6.0", architecture="WaveNet", config=config, metadata=dict(name="planner pin model"), weights=w, sample_rate=48000)

    inner = model([dict(input_size=1, condition_size=1, head_size=8, channels=4, kernel_size=3, dilations=[1, 2, 4, 8] * 4,
                        activation="ReLU", gated=False, head_bias=False)], 0.5)
    main = dict(input_size=1, condition_size=8, head_size=1, head_bias=True, channels=4, bottleneck=4, kernel_size=4, dilations=[3],
                activation="Softsign", gating_mode="none", layer1x1=dict(active=True, groups=1),
                head1x1=dict(active=True, out_channels=4, groups=1))
    for key in msm.FILM_KEYS:
        main[key] = dict(active=True, shift=True, groups=1)
    with open(path, "w") as f:
        json.dump(model([main], 0.1, inner), f)


def write_narrow(tmp, idx):
    """A narrow stack drawn the way tools/fuzz_models.py: random_narrow draws one (1 .. 4 channels per array, odd dilations)."""
    rng = np.random.default_rng(2000 + idx)
    arrays = []
    for _ in range(int(rng.integers(1, 4))):
        C = int(rng.choice([1, 2, 3, 4]))
        dl = [int(rng.choice([1, 2, 3, 5, 7, 16, 31, 32, 33, 63, 64, 65, 100, 127, 128, 300, 512, 700])) for _ in range(int(rng.integers(1, 7)))]
        arrays.append((C, dl, ["Tanh", "ReLU", "Sigmoid"][int(rng.integers(3))], bool(rng.integers(2))))
    name = "narrow_%02d" % idx
    old = msm.HERE
    msm.HERE = tmp  # (build writes to HERE/models)
    try:
        msm.build(name, arrays, int(rng.integers(1 << 30)))
    finally:
        msm.HERE = old
    return os.path.join(tmp, "models", name + ".nam")


def generate_models(tmp):
    """The generated models, in table order: 64 feature-rich ones, 24 narrow stacks, the pin model."""
    os.makedirs(os.path.join(tmp, "models"), exist_ok=True)
    paths = []
    for seed in range(1000, 1064):
        p = os.path.join(tmp, "models", "featured_%d.nam" % seed)
        msm.write_featured(p, seed, wr_shapes=bool(seed % 2), post_head=bool((seed // 2) % 2))
        paths.append(p)
    paths += [write_narrow(tmp, i) for i in range(24)]
    pin = os.path.join(tmp, "models", PIN)
    write_pin_model(pin)
    return paths + [pin]


def build_dump(csrc, exe):
    assert os.path.exists(CLANG), "the ROCm toolchain that builds the library also builds this check"
    sources = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f == "nam_loader.cpp" or re.fullmatch(r"plan.*\.cpp", f)]
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + csrc, "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "src", "plan_dump.cpp")] + sources,
                   check=True, timeout=600)


def run_dump(exe, paths, **extra_env):
    env = dict(os.environ)  # (LD_PRELOAD neither set nor removed: the sanitizer runtime is linked into the executable)
    for k in ("NAM_HIP_WR_PROGRAM", "NAM_HIP_WR_CUT2"):
        env.pop(k, None)
    env.update(extra_env)
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    r = subprocess.run([exe] + paths, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def field(line, key, missing=None):
    m = re.search(r"(?:^| )%s=(\[[^\]]*\]|\S+)" % re.escape(key), line)
    assert m or missing is not None, (key, line)
    return m.group(1) if m else missing


def model_line(name, lines, coverage):
    """The table's line for one model in one section: the hash of everything plan_dump printed for it (the full output of the whole
    set is 750 KB: `--full` prints it), and — `coverage` — what its fast_tanh 0 plans reach, for test_table_covers_what_it_pins:
    planned / plans with shapes on offer (J) and without (B), the first refusal's reason of each, plans that needed run-time-flag
    layers (rt), with a head rechannel with taps, a post-stack head ring, a condition_dsp; compiled-in programs with a cut run, with
    a matrix-form FiLM layer, with both."""
    out = "m %s lines=%d dump=%s" % (name, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16])
    if not coverage:
        return out
    num = lambda l, k: int(field(l, k))  # noqa: E731
    assert not [l for l in lines if l.startswith("model ")], "a model that could not be loaded or planned pins nothing: " + lines[0]
    plans = [l for l in lines if l.startswith("plan ") and num(l, "ft") == 0]
    J = [l for l in plans if num(l, "shapes") == 1]
    B = [l for l in plans if num(l, "shapes") == 0]
    cut = set(field(l, "p") for l in lines if l.startswith("program ") and num(l, "ft") == 0
              and int(field(l, "ops_cut").split(":")[0]) > int(field(l, "ops").split(":")[0]))
    film = set(field(l, "program") for l in J if num(l, "jit") and num(l, "n_film_matrix"))
    why = lambda ls: ([field(l, "why") for l in ls if not num(l, "ok") and field(l, "why") != "[]"] + ["[]"])[0]  # noqa: E731
    out += " J=%d/%d B=%d/%d" % (sum(num(l, "ok") for l in J), len(J), sum(num(l, "ok") for l in B), len(B))
    counts = dict(rt=sum(num(l, "ok") and num(l, "has_rt_layers") for l in B), end_k=sum(num(l, "n_end_k") > 0 for l in J),
                  post_ring=sum(num(l, "n_post_ring") > 0 for l in J), set_cond=sum(num(l, "n_set_cond") > 0 for l in J), cut=len(cut),
                  film=len(film), both=len(cut & film))
    out += "".join(" %s=%d" % kv for kv in counts.items() if kv[1])  # (a count of 0 and an empty reason are not written)
    return out + "".join(" %s=%s" % kv for kv in (("whyJ", why(J)), ("whyB", why(B))) if kv[1] != "[]")


def make_table(csrc, tmp, full=False):
    """-> (the table's text, {(section, model): the lines plan_dump printed})"""
    exe = os.path.join(tmp, "plan_dump")
    build_dump(csrc, exe)
    generated = generate_models(tmp)
    fixtures = [os.path.join(MODELS, f) for f in sorted(os.listdir(MODELS)) if f.endswith(".nam")]
    everything = fixtures + generated
    out = ["# generated models (sha256, 64 bits)"]
    for p in generated:
        with open(p, "rb") as f:
            out.append("file %s %s" % (os.path.basename(p), hashlib.sha256(f.read()).hexdigest()[:16]))
    printed = {}
    for section, env, paths in (("default", {}, everything), ("NAM_HIP_WR_PROGRAM=0", dict(NAM_HIP_WR_PROGRAM="0"), everything),
                                ("NAM_HIP_WR_CUT2=3", dict(NAM_HIP_WR_CUT2="3"), [p for p in everything if os.path.basename(p) in CUT2_MODELS])):
        out.append("# section " + section)
        lines = run_dump(exe, paths, **env).splitlines()
        for p in paths:
            name = os.path.basename(p)
            mine = [l for l in lines if l.split()[1] == name]
            printed[(section, name)] = mine
            out += mine if full else [model_line(name, mine, section == "default")]
    return "\n".join(out) + "\n", printed


def test_table_covers_what_it_pins():
    """Conditions on the recorded table itself: a pin that no input reaches holds nothing."""
    with open(TABLE) as f:
        lines = f.read().splitlines()
    default = lines[lines.index("# section default") + 1:lines.index("# section NAM_HIP_WR_PROGRAM=0")]
    assert len(default) == 31 + 89 and all(l.startswith("m ") for l in default)
    pair = lambda l, k: [int(x) for x in field(l, k).split("/")]  # noqa: E731
    count = lambda k: sum(int(field(l, k, "0")) for l in default)  # noqa: E731
    # refusals, with their reasons. Shapes on offer and still refused: the per-model policy said no (its `why` is the one kept).
    # No shapes and refused: the run-time-flag policy said no. No shapes, planned, with run-time-flag layers: the exact-shapes
    # policy said no and the next one took the model.
    assert [l for l in default if field(l, "whyJ", "[]") != "[]"]
    assert [l for l in default if field(l, "whyB", "[]") != "[]"]
    assert count("rt") and count("end_k") and count("post_ring") and count("set_cond")
    assert count("cut") and count("film") and count("both")
    by_name = {l.split()[1]: l for l in default}
    assert pair(by_name["slimmable_wavenet.nam"], "J")[1] >= 3  # widths
    assert pair(by_name["slimmable_container.nam"], "J")[1] >= 2  # submodels
    assert int(field(by_name[PIN], "both", "0")) == 1
    generated = [l.split()[1] for l in lines if l.startswith("file ")]
    assert len(generated) == 89
    for name in generated:
        assert pair(by_name[name], "J")[0] >= 1, name  # every generated model is planned with a shape set on offer


def test_planner_output_is_the_recorded_table(tmp_path):
    with open(TABLE) as f:
        want = f.read().splitlines()
    text, printed = make_table(CSRC, str(tmp_path))
    got = text.splitlines()
    files_want = [l for l in want if l.startswith("file ")]
    files_got = [l for l in got if l.startswith("file ")]
    drift = [(a, b) for a, b in zip(files_want, files_got) if a != b]
    assert not drift and len(files_want) == len(files_got), \
        "the generator drifted (not the planner): the generated .nam files are not the recorded ones\n  recorded: %s\n  now:      %s" % (
            drift[0] if drift else (len(files_want), len(files_got)))
    section = None
    for i, (a, b) in enumerate(zip(want, got)):
        section = a[len("# section "):] if a.startswith("# section ") else section
        assert a == b, ("the planner's output changed, line %d\n  recorded: %s\n  now:      %s\nwhat plan_dump prints for it now (the "
                        "recorded side: profiles/plan_wr/README.md, --full):\n%s") % (i + 1, a, b, "\n".join(printed.get((section, b.split()[1]), [])))
    assert len(want) == len(got), "the planner's output has %d lines, the recorded table %d" % (len(got), len(want))


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        sys.stdout.write(make_table([a for a in sys.argv[1:] if a != "--full"][0], tmp, full="--full" in sys.argv)[0])
