"""Can a model notice that one of its weights is wrong? The census of a model's teeth, and the live feature-rich models.

census(document, fast_tanh, x): scale one weight at a time by 1 + 2^-k (rounded to float32 like every weight), run the strict
float32 oracle, and count the perturbations whose max error against the UNPERTURBED float64 truth stays within FACTOR x e32
(tests/accuracy.py) — the faults the float64 bound could not report on that model and input. A model where that share is large
tests nothing: a wrong history ring, tap, FiLM shift or gate path would not change its output either.

The 50 seeded feature-rich models of tests/test_gpu_breadth.py (make_synthetic_models.write_featured) are mostly such models
at gain 1: outputs of 0.004 .. 0.6 that hardly move. LIVE GAINS: every weight but the trailing head_scale of each WaveNet list
times one gain g per seed (make_synthetic_models.apply_gain; head_scale stays because it is compiled into the per-model code
object, so the gained model runs on the code object of the ungained one), g = the largest 2^(k/4), k = 0 .. 8, tried upwards,
at which the float64 output's swing over time stays <= 4 on the census input (chosen from the float64 oracle alone, on the CPU).

    python tests/model_teeth.py            # writes tests/golden/featured_live.json (tests/test_model_teeth.py recomputes it)
    python tests/model_teeth.py --report   # the figures of profiles/accuracy/README.md: the census before / after the gain
    python tests/model_teeth.py --rows OUT # the ACCURACY lines of a `pytest -s` run of the GPU cases as that README's table rows

A seed is LIVE when swing >= MIN_SWING and unnoticed / sampled <= MAX_SHARE; the others stay in the table with their figures
and run only in the flat-bound test they have always been in.
"""
import copy
import functools
import json
import os
import sys

import numpy as np

from conftest import ROOT  # (first: it puts the oracle on the path)
import accuracy
from signals import stream_bank

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_synthetic_models as msm  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "featured_live.json")
SEEDS = range(50)  # tests/test_gpu_breadth.py: FEATURED_SEEDS
GAINS = [2.0 ** (k / 4) for k in range(9)]
MAX_SWING = 4.0
MIN_SWING, MAX_SHARE, MAX_SHARE_OVERALL, MIN_LIVE = 0.1, 0.30, 0.20, 44
CENSUS_STREAMS, CENSUS_AMPLITUDE, CENSUS_K, CENSUS_SAMPLE = 2, 2.7, 6, 100
SMOOTH_ACTS = {"Tanh", "Sigmoid", "SiLU"}  # what fast_tanh / libm mode changes (and what wr_act1 evaluates in exp2 forms)


def fast_tanh_of(seed):
    return seed % 3 == 0  # as tests/test_gpu_breadth.py loads them


def featured(seed, gain=1.0, path=os.devnull):
    """The document of featured model `seed`, as test_featured_models_match_oracle_and_reference writes it, times `gain`."""
    return msm.write_featured(path, 7000 + seed, wr_shapes=bool(seed % 2), post_head=seed >= 40, gain=gain)


def in_channels(document):
    return int(document["config"].get("in_channels", 1)) if document["architecture"] == "WaveNet" else 1


@functools.lru_cache(maxsize=None)
def inputs(n_in, amplitude):
    """The input of the GPU cases: accuracy.inputs for one channel; [8, n_in, 768] of the same bank for more."""
    if n_in == 1:
        return accuracy.inputs(amplitude)
    x = stream_bank(accuracy.N_STREAMS * n_in, accuracy.N_FRAMES, seed=accuracy.SEED).reshape(accuracy.N_STREAMS, n_in, accuracy.N_FRAMES)
    x = np.ascontiguousarray(x * np.float32(amplitude), dtype=np.float32)
    x.setflags(write=False)
    return x


def census_input(document):
    """The first CENSUS_STREAMS streams of the GPU cases' input at amplitude 2.7."""
    return inputs(in_channels(document), CENSUS_AMPLITUDE)[:CENSUS_STREAMS]


def swing_of(truth):
    """The largest peak-to-peak excursion over time of any stream and output channel."""
    return float(np.max(truth.max(axis=-1) - truth.min(axis=-1)))


def census(document, fast_tanh, x, k=CENSUS_K, sample=CENSUS_SAMPLE, luts=None):
    """-> dict(peak, swing, e32, sampled, unnoticed, unnoticed_flat). At most `sample` weights per "weights" list (all of a
    shorter list; a fixed draw otherwise); a weight the factor does not move (a zero) is not counted."""
    truth = accuracy.run_oracle(document, fast_tanh, x, "f64", luts=luts)
    e32 = float(np.max(np.abs(accuracy.run_oracle(document, fast_tanh, x, "f32", luts=luts).astype(np.float64) - truth)))
    peak = float(np.max(np.abs(truth)))
    flat = accuracy.old_bound(fast_tanh, peak)
    j = copy.deepcopy(document)
    sampled = unnoticed = unnoticed_flat = 0
    for d in msm.weight_documents(j):
        w = d["weights"]
        idx = range(len(w)) if len(w) <= sample else np.sort(np.random.default_rng(1).choice(len(w), sample, replace=False))
        for i in idx:
            i = int(i)
            old = w[i]
            w[i] = float(np.float32(np.float32(old) * np.float32(1.0 + 2.0 ** -k)))
            if w[i] != old:
                err = float(np.max(np.abs(accuracy.run_oracle(j, fast_tanh, x, "f32", luts=luts).astype(np.float64) - truth)))
                sampled += 1
                unnoticed += err <= accuracy.FACTOR * e32
                unnoticed_flat += err <= flat
            w[i] = old
    return dict(peak=peak, swing=swing_of(truth), e32=e32, sampled=sampled, unnoticed=int(unnoticed), unnoticed_flat=int(unnoticed_flat))


def choose_gain(seed):
    """The largest gain of GAINS, tried upwards, at which the float64 output stays finite and swings by at most MAX_SWING."""
    best = GAINS[0]
    for g in GAINS:
        doc = featured(seed, g)
        t = accuracy.run_oracle(doc, fast_tanh_of(seed), census_input(doc), "f64")
        if not np.isfinite(t).all() or swing_of(t) > MAX_SWING:
            break
        best = g
    return best


def is_live(row):
    return row["swing"] >= MIN_SWING and row["sampled"] > 0 and row["unnoticed"] <= MAX_SHARE * row["sampled"]


def table_row(seed, gain=None):
    gain = choose_gain(seed) if gain is None else gain
    doc = featured(seed, gain)
    c = census(doc, fast_tanh_of(seed), census_input(doc))
    row = dict(seed=seed, gain=gain, swing=c["swing"], peak=c["peak"], e32=c["e32"], sampled=c["sampled"], unnoticed=c["unnoticed"])
    row["live"] = bool(is_live(row))
    return row


def compute_table(seeds=SEEDS):
    accuracy.nam_oracle.build()
    return [table_row(seed) for seed in seeds]


@functools.lru_cache(maxsize=None)
def _table_file():
    with open(TABLE) as f:
        return json.load(f)


def load_table():
    return _table_file()["models"]


def live_rows():
    return [r for r in load_table() if r["live"]]


# ---------------------------------------------------------------------------
# The fixtures the float64 bound did not hold yet (tests/test_gpu_accuracy_breadth.py), with the same census
# ---------------------------------------------------------------------------
# A fixture is DEAD when more than MAX_SHARE of its sampled weights go unnoticed, or when its output is a constant for all
# practical purposes: swing < MIN_RELATIVE_SWING x peak. (The absolute MIN_SWING is a condition on the gained models, whose gain
# is chosen to reach it; the A1 / K-tap fixtures have head scales of 0.05 and peak at 0.02 .. 0.25 with swings as large as
# their peaks, and miss 1 .. 10 of 60 perturbed weights.) A dead fixture stays in its flat-bound parity test only.
MIN_RELATIVE_SWING = 0.01
FIXTURE_SAMPLE = 60
POSTHEAD_LIVE = "synth_posthead_live"  # written at test time (write_fixture): the fixtures' directory is pinned by test_plan_pin.py
LUTS = {
    "lut_wavenet": ("wavenet", {"Tanh": (-5.0, 5.0, 1024)}),
    "lut_a1_standard": ("wavenet_a1_standard", {"Tanh": (-4.0, 4.0, 4096)}),
    "lut_a2_max": ("wavenet_a2_max", {"Sigmoid": (-8.0, 8.0, 1024), "SiLU": (-6.0, 6.0, 333)}),
}  # tests/test_gpu_parity.py: test_lookup_table_activations_match_oracle
SYNTH_A1 = ["synth_a1_13", "synth_a1_c12", "synth_a1_c8", "synth_a1_mixed", "synth_a1_lite", "synth_a1_c14"]
SYNTH_KT = ["synth_kt_c8", "synth_kt_c16", "synth_kt_c12", "synth_kt_c4"]
FIXTURES = (["wavenet_condition_dsp", "synth_multich", "synth_leakyhardtanh", "synth_posthead", POSTHEAD_LIVE] + SYNTH_A1 + SYNTH_KT
            + sorted(LUTS))


def write_fixture(name, path):
    """The one model of FIXTURES that is not a committed file: synth_posthead's topology drawn again (another seed, weights 2.8
    times larger), so that the post-stack head sees a signal that moves: swing 1.7 at peak 1.7, where synth_posthead swings by
    0.006 around a bias of 0.71."""
    assert name == POSTHEAD_LIVE
    msm.build_general(name, path=path, **dict(msm.GENERAL["synth_posthead"], seed=121, gain=2.5))
    return path


@functools.lru_cache(maxsize=None)
def fixture_document(name):
    """-> (parsed document, luts or None)"""
    if name == POSTHEAD_LIVE:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            return accuracy.nam_oracle.validate_nam_file(write_fixture(name, os.path.join(tmp, name + ".nam"))), None
    model, luts = LUTS.get(name, (name, None))
    return accuracy.nam_oracle.validate_nam_file(accuracy.model_path(model)), luts


def fixture_row(name):
    doc, luts = fixture_document(name)
    c = census(doc, True, census_input(doc), sample=FIXTURE_SAMPLE, luts=luts)
    row = dict(name=name, swing=c["swing"], peak=c["peak"], e32=c["e32"], sampled=c["sampled"], unnoticed=c["unnoticed"])
    row["dead"] = bool(row["unnoticed"] > MAX_SHARE * row["sampled"] or row["swing"] < MIN_RELATIVE_SWING * row["peak"])
    return row


def load_fixture_table():
    return {r["name"]: r for r in _table_file()["fixtures"]}


class Truth:
    """What accuracy.Yardstick is for a named fixture, for any document: truth, e32 and (lazily) e32_exp2 on input x."""

    def __init__(self, document, fast_tanh, x, luts=None):
        accuracy.nam_oracle.build()
        self._args = (document, fast_tanh, x)
        self._luts = luts
        self.truth = accuracy.run_oracle(document, fast_tanh, x, "f64", luts=luts)
        self.truth.setflags(write=False)
        self.peak = float(np.max(np.abs(self.truth)))
        self.e32 = self.error(accuracy.run_oracle(document, fast_tanh, x, "f32", luts=luts))
        self._e32_exp2 = None

    def error(self, y):
        assert y.shape == self.truth.shape, (y.shape, self.truth.shape)
        return float(np.max(np.abs(y.astype(np.float64) - self.truth)))

    @property
    def e32_exp2(self):
        if self._e32_exp2 is None:
            self._e32_exp2 = self.error(accuracy.run_oracle(*self._args, "f32x2", luts=self._luts))
        return self._e32_exp2


@functools.lru_cache(maxsize=None)
def live_document(seed):
    return featured(seed, next(r["gain"] for r in load_table() if r["seed"] == seed))


@functools.lru_cache(maxsize=None)
def live_truth(seed, fast_tanh, amplitude):
    doc = live_document(seed)
    return Truth(doc, fast_tanh, inputs(in_channels(doc), amplitude))


@functools.lru_cache(maxsize=None)
def fixture_truth(name, fast_tanh, amplitude):
    doc, luts = fixture_document(name)
    return Truth(doc, fast_tanh, inputs(in_channels(doc), amplitude), luts=luts)


# ---------------------------------------------------------------------------
# What a document exercises, read from its JSON
# ---------------------------------------------------------------------------
ACTIVATIONS = ["Tanh", "ReLU", "Sigmoid", "Hardtanh", "SiLU", "Softsign", "Hardswish", "LeakyReLU", "LeakyHardtanh", "Fasttanh", "PReLU"]
REQUIRED = (["gating:none", "gating:gated", "gating:blended"] + [f"{k}:{s}" for k in msm.FILM_KEYS for s in ("shift", "scale")]
            + ["groups_input", "groups_input_mixin", "groups_layer1x1", "groups_head1x1", "bottleneck", "condition_dsp", "post_head",
               "in_channels"] + ["act:" + a for a in ACTIVATIONS])


def _act_names(a):
    if a is None:
        return []
    if isinstance(a, list):
        return [n for v in a for n in _act_names(v)]
    return [a if isinstance(a, str) else a["type"]]


def activation_types(document):
    """Every activation type named anywhere in a WaveNet document (layers, secondaries, post-stack head, nested condition)."""
    if document["architecture"] != "WaveNet":
        return set()
    cfg = document["config"]
    names = set()
    for a in cfg["layers"]:
        names |= set(_act_names(a["activation"])) | set(_act_names(a.get("secondary_activation")))
        n = len(a["dilations"])
        modes = a["gating_mode"] if isinstance(a.get("gating_mode"), list) else [a.get("gating_mode", "gated" if a.get("gated") else "none")] * n
        if any(m != "none" for m in modes) and "secondary_activation" not in a:
            names.add("Sigmoid")  # the default secondary
    if cfg.get("head"):
        names |= set(_act_names(cfg["head"]["activation"]))
    if cfg.get("condition_dsp"):
        names |= activation_types(cfg["condition_dsp"])
    return {"LeakyHardtanh" if n == "LeakyHardTanh" else n for n in names}


def has_smooth_activation(document):
    return bool(activation_types(document) & SMOOTH_ACTS)


def features(document):
    """The members of REQUIRED this WaveNet document exercises."""
    cfg = document["config"]
    f = {"act:" + a for a in activation_types(document)}
    if cfg.get("condition_dsp"):
        f.add("condition_dsp")
        f |= features(cfg["condition_dsp"]) - {"in_channels"}
    if cfg.get("head"):
        f.add("post_head")
    if cfg.get("in_channels", 1) > 1:
        f.add("in_channels")
    for a in cfg["layers"]:
        C, B, n, ks, modes, h1, HO, l1, hs, hk, hb = msm._arr_dims(a)
        f |= {"gating:" + m for m in modes}
        if a.get("groups_input", 1) > 1:
            f.add("groups_input")
        if a.get("groups_input_mixin", 1) > 1:
            f.add("groups_input_mixin")
        if l1.get("active", True) and l1.get("groups", 1) > 1:
            f.add("groups_layer1x1")
        if HO and h1.get("groups", 1) > 1:
            f.add("groups_head1x1")
        if B != C:
            f.add("bottleneck")
        for key in msm.FILM_KEYS:
            film = a.get(key, False)
            if film is False or not film.get("active", True):
                continue
            if (key == "head1x1_post_film" and not HO) or (key == "layer1x1_post_film" and not l1.get("active", True)):
                continue
            f.add(f"{key}:{'shift' if film.get('shift', True) else 'scale'}")
    return f


# ---------------------------------------------------------------------------
def _report():
    accuracy.nam_oracle.build()
    for label, gain_of in (("gain 1", lambda s: 1.0), ("live gains", lambda s: None)):
        rows = []
        for s in SEEDS:
            gain = choose_gain(s) if gain_of(s) is None else gain_of(s)
            doc = featured(s, gain)
            r = dict(census(doc, fast_tanh_of(s), census_input(doc)), seed=s, gain=gain)
            r["live"] = is_live(r)
            rows.append(r)
            print(f"{label}: seed {r['seed']} gain {r['gain']:.3f} swing {r['swing']:.3g} peak {r['peak']:.3g} e32 {r['e32']:.2e} "
                  f"4 e32 / flat bound {accuracy.FACTOR * r['e32'] / accuracy.old_bound(fast_tanh_of(s), r['peak']):.5f} "
                  f"unnoticed {r['unnoticed']} / {r['sampled']} ({r['unnoticed'] / max(r['sampled'], 1):.2f}), by the flat bound "
                  f"{r['unnoticed_flat']} {'live' if r['live'] else 'DEAD'}")
        print(f"{label}: inside the flat bound {sum(r['unnoticed_flat'] for r in rows)} / {sum(r['sampled'] for r in rows)}")
        print(f"{label}: unnoticed {sum(r['unnoticed'] for r in rows)} / {sum(r['sampled'] for r in rows)}, "
              f"{sum(r['live'] for r in rows)} live; over the live ones {sum(r['unnoticed'] for r in rows if r['live'])} / "
              f"{sum(r['sampled'] for r in rows if r['live'])}")


CALLS = {"generic_calls": "11 x 64 + 37 + 27", "wn_reg_calls": "11 x 64 + 37 + 27", "wn_reg_launch": "512 + 256 in one launch each",
         "wn_reg_session": "session of 12 commands", "wn_reg_table_session": "table form (NAM_HIP_WR_PROGRAM=0), session of 12 commands",
         "a1_mfma_calls": "11 x 64 + 37 + 27", "q_session": "padded form, session of 12 commands", "kt_mfma_calls": "11 x 64 + 37 + 27",
         "a1_valu_calls": "11 x 64 + 37 + 27", "auto_calls": "AUTO, 11 x 64 + 37 + 27"}


def _rows(path):
    """The ACCURACY lines of a `pytest -s` run of tests/test_gpu_accuracy_breadth.py as the rows of profiles/accuracy/README.md."""
    import re
    print("| model | kernel, calls | tanh | amp | peak | e32 | e_gpu | e_gpu / e32 | yardstick | census (unnoticed / sampled) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    with open(path) as f:
        for m in re.finditer(r"ACCURACY (\S+) (\S+) (\S+) fast_tanh=(\d) amp=(\S+) yardstick=(\S+) peak=(\S+) e32=(\S+) e_gpu=(\S+) "
                             r"e_gpu/e32=(\S+) tanhf_e32=(\S+) census=(\S+)", f.read()):
            case, kname, model, ft, amp, yard, peak, e32, e_gpu, ratio, e32_tanhf, share = m.groups()
            note = "tanhf" if yard == "libm" else f"exp2 form (tanhf's: e32 {e32_tanhf}, ratio {float(e_gpu) / float(e32_tanhf):.2f})"
            print(f"| {model} | {kname}, {CALLS[case]} | {'fast' if ft == '1' else 'libm'} | {amp} | {peak} | {e32} | {e_gpu} | {ratio} | "
                  f"{note} | {share.replace('/', ' / ')} |")


def main():
    if "--report" in sys.argv:
        return _report()
    if "--rows" in sys.argv:
        return _rows(sys.argv[sys.argv.index("--rows") + 1])
    rows = compute_table()
    fixtures = [fixture_row(name) for name in FIXTURES]
    with open(TABLE, "w") as f:
        json.dump(dict(note="written by tests/model_teeth.py; recomputed by tests/test_model_teeth.py", k=CENSUS_K, sample=CENSUS_SAMPLE,
                       fixture_sample=FIXTURE_SAMPLE, streams=CENSUS_STREAMS, amplitude=CENSUS_AMPLITUDE, models=rows, fixtures=fixtures),
                  f, indent=1)
        f.write("\n")
    for r in fixtures:
        print(f"fixture {r['name']}: swing {r['swing']:.3g} peak {r['peak']:.3g} e32 {r['e32']:.2e} unnoticed {r['unnoticed']} / {r['sampled']}"
              f"{' DEAD' if r['dead'] else ''}")
    live = [r for r in rows if r["live"]]
    print(f"{len(live)} of {len(rows)} live; unnoticed over the live set {sum(r['unnoticed'] for r in live)} / {sum(r['sampled'] for r in live)}; "
          f"left out: {[r['seed'] for r in rows if not r['live']]}")


if __name__ == "__main__":
    main()
