"""The inputs of tests/test_gpu_accuracy_breadth.py checked on the CPU (tests/model_teeth.py): conditions on the models, not
measurements of the kernels.

1. The gain leaves the generator alone at gain 1 (the bytes of every seeded model are the recorded ones) and scales every weight
   but the trailing head_scale of each WaveNet list; the planner's shape-set header — the text nam_wn_reg_kernel's per-model
   code object is compiled from and found by — is the same with and without the gain.
2. tests/golden/featured_live.json is what tests/model_teeth.py computes: gains chosen from the float64 oracle, the census figures.
3. At least 44 of the 50 seeds are live (swing >= 0.1, at most 30 % of the sampled single-weight errors of 2^-6 unnoticed by
   4 e32), at most 20 % go unnoticed over the live set, and every feature of the op program appears in a live model that
   nam_wn_reg_kernel accepts and in one the interpreter runs.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import accuracy
import model_teeth as mt
import test_plan_pin

msm = mt.msm

# sha256 over the bytes write_featured(7000 + seed, wr_shapes = seed odd, post_head = seed >= 40) wrote for seeds 0 .. 49, in
# order, at the commit before it had a gain
FEATURED_BYTES = "6caa508c8729edfcd0fa4430bba4c3bf718b4064df9fac2f78f711db61cbfcbc"


def test_gain_one_writes_the_recorded_bytes(tmp_path):
    h = hashlib.sha256()
    for seed in mt.SEEDS:
        for kwargs in ({}, {"gain": 1.0}):
            p = str(tmp_path / "m.nam")
            msm.write_featured(p, 7000 + seed, wr_shapes=bool(seed % 2), post_head=seed >= 40, **kwargs)
            with open(p, "rb") as f:
                data = f.read()
            if kwargs:
                assert data == last
            last = data
        h.update(data)
    assert h.hexdigest() == FEATURED_BYTES


def test_gain_scales_every_weight_but_each_head_scale():
    seen_nested = seen_post_head = False
    for seed in (1, 7, 43, 47):  # nested conditions; 43, 47: with a post-stack head
        plain, gained = mt.featured(seed), mt.featured(seed, 2.0 ** 0.75)
        a, b = msm.weight_documents(plain), msm.weight_documents(gained)
        assert len(a) == len(b) >= 1 and a[0] is plain
        seen_nested |= len(a) > 1
        seen_post_head |= plain["config"]["head"] is not None
        for da, db in zip(a, b):
            wa, wb = np.asarray(da["weights"], dtype=np.float64), np.asarray(db["weights"], dtype=np.float64)
            assert da["config"]["head_scale"] == wa[-1] == wb[-1]
            want = (wa[:-1].astype(np.float32) * np.float32(2.0 ** 0.75)).astype(np.float64)
            np.testing.assert_array_equal(wb[:-1], want)
            assert np.all(wb[:-1][wa[:-1] != 0] != wa[:-1][wa[:-1] != 0])
        # nothing but weights differs
        for d in b:
            d["weights"] = None
        for d in a:
            d["weights"] = None
        assert plain == gained
    assert seen_nested and seen_post_head


def test_gain_leaves_the_code_object_header_alone(tmp_path):
    """WrShapeSet::header_text prints the shapes, the op programs with their offsets and each op's scale (head_scale, a nested
    condition's head_scale) — nothing else of the weights. tests/src/plan_dump.cpp prints its length and hash per shape set."""
    exe = str(tmp_path / "plan_dump")
    test_plan_pin.build_dump(test_plan_pin.CSRC, exe)
    paths = []
    for r in mt.load_table():
        for tag, gain in (("plain", 1.0), ("gained", r["gain"])):
            paths.append(str(tmp_path / f"{tag}_{r['seed']}.nam"))
            mt.featured(r["seed"], gain, paths[-1])
    lines = [l.split() for l in test_plan_pin.run_dump(exe, paths).splitlines() if l.startswith("shapes ")]
    by_file = {}
    for l in lines:
        by_file.setdefault(l[1], []).append(l[2:])
    assert len(by_file) == 2 * len(mt.load_table())  # every model, gained or not, has shape sets on offer
    for r in mt.load_table():
        plain, gained = by_file[f"plain_{r['seed']}.nam"], by_file[f"gained_{r['seed']}.nam"]
        assert plain == gained and any(f.startswith("header=") for f in plain[0]), r["seed"]


@pytest.fixture(scope="module")
def computed():
    accuracy.nam_oracle.build()
    return [mt.table_row(seed) for seed in mt.SEEDS], [mt.fixture_row(name) for name in mt.FIXTURES]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], float):
            assert a[k] == pytest.approx(b[k], rel=1e-9, abs=0.0), (k, a, b)
        else:
            assert a[k] == b[k], (k, a, b)


def test_committed_table_is_the_computed_one(computed):
    models, fixtures = computed
    with open(mt.TABLE) as f:
        t = json.load(f)
    assert (t["k"], t["sample"], t["fixture_sample"], t["streams"], t["amplitude"]) == (
        mt.CENSUS_K, mt.CENSUS_SAMPLE, mt.FIXTURE_SAMPLE, mt.CENSUS_STREAMS, mt.CENSUS_AMPLITUDE)
    assert len(t["models"]) == len(models) == 50 and len(t["fixtures"]) == len(fixtures)
    for a, b in zip(t["models"], models):
        _same(a, b)
    for a, b in zip(t["fixtures"], fixtures):
        _same(a, b)


def test_live_set_conditions(computed):
    models, fixtures = computed
    live = [r for r in models if r["live"]]
    for r in models:
        share = r["unnoticed"] / max(r["sampled"], 1)
        print(f"seed {r['seed']} gain {r['gain']:.3f} swing {r['swing']:.3g} peak {r['peak']:.3g} e32 {r['e32']:.2e} unnoticed "
              f"{r['unnoticed']} / {r['sampled']} = {share:.2f} {'live' if r['live'] else 'LEFT OUT'}")
        assert r["gain"] in mt.GAINS and r["sampled"] > 0
        assert r["live"] == (r["swing"] >= 0.1 and share <= 0.30)
    assert len(live) >= 44, [r["seed"] for r in models if not r["live"]]
    unnoticed, sampled = sum(r["unnoticed"] for r in live), sum(r["sampled"] for r in live)
    print(f"live set: {len(live)} seeds, unnoticed {unnoticed} / {sampled} = {unnoticed / sampled:.3f}")
    assert unnoticed <= 0.20 * sampled
    # the fixtures of the GPU cases: the dead ones are named, the others pass the same share
    assert [r["name"] for r in fixtures if r["dead"]] == ["synth_posthead"]
    for r in fixtures:
        assert r["dead"] or (r["unnoticed"] <= 0.30 * r["sampled"] and r["swing"] >= mt.MIN_RELATIVE_SWING * r["peak"]), r


def test_every_feature_is_in_a_live_model_on_each_kernel(nam_lib, tmp_path):
    """Read from the generated JSON. nam_generic_kernel (the interpreter) runs every model; nam_wn_reg_kernel those it accepts
    (loading a model needs no GPU). The GPU cases run each live model on both where both take it."""
    nam = nam_lib
    on_wn_reg, on_interpreter, interpreter_only = set(), set(), set()
    for r in mt.live_rows():
        path = str(tmp_path / f"live_{r['seed']}.nam")
        f = mt.features(mt.featured(r["seed"], r["gain"], path))
        assert f <= set(mt.REQUIRED), f - set(mt.REQUIRED)
        on_interpreter |= f
        if nam.get_dsp(path, fast_tanh=mt.fast_tanh_of(r["seed"])).info.has_a1_kernel & 16:
            on_wn_reg |= f
        else:
            interpreter_only |= f
    print("features on interpreter-only live models:", sorted(interpreter_only))
    assert set(mt.REQUIRED) - on_wn_reg == set(), sorted(set(mt.REQUIRED) - on_wn_reg)
    assert set(mt.REQUIRED) - on_interpreter == set(), sorted(set(mt.REQUIRED) - on_interpreter)
    # what _random_activation can draw is what REQUIRED lists
    rng, drawn = np.random.default_rng(0), set()
    for _ in range(400):
        a = msm._random_activation(rng, 3)
        drawn.add(a if isinstance(a, str) else a["type"])
    assert drawn == set(mt.ACTIVATIONS)


def test_census_counts_what_the_bound_cannot_see():
    """On a model with a dead weight the census says so: a weight behind a ReLU that never opens changes nothing."""
    doc = {"version": "0.5.4", "architecture": "WaveNet", "sample_rate": 48000,
           "config": {"layers": [dict(input_size=1, condition_size=1, head_size=1, channels=1, kernel_size=1, dilations=[1], activation="ReLU",
                                      gated=False, head_bias=True)], "head": None, "head_scale": 1.0},
           # rechannel, conv, conv bias (keeps the ReLU shut), mixin, 1x1, 1x1 bias, head, head bias, head_scale
           "weights": [1.0, 0.5, -10.0, 0.25, 1.0, 0.5, 1.0, 0.75, 1.0]}
    x = mt.inputs(1, 1.0)[:2]
    c = mt.census(doc, True, x, sample=100)
    # the ReLU's output is 0: only the head bias and head_scale reach the output
    assert (c["sampled"], c["unnoticed"]) == (9, 7) and c["swing"] == 0.0 and c["peak"] == 0.75
    doc["weights"][2] = 0.1
    c = mt.census(doc, True, x, sample=100)
    assert c["sampled"] == 9 and c["unnoticed"] <= 2 and c["swing"] > 0.1  # (the 1x1 feeds nothing behind the last layer)
    assert mt.census(doc, True, x, sample=4)["sampled"] == 4
