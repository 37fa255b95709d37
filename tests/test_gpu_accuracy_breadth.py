"""-m gpu: the breadth of the op program held to the float64 bound of tests/test_gpu_accuracy.py,

    max |gpu - truth| <= 4 x yardstick      8 streams x 768 frames of stream_bank x 2.7 and x 1.0, Reset(prewarm=True) on both sides

on models that can notice a fault: the LIVE feature-rich models (tests/model_teeth.py: the seeded models of test_gpu_breadth.py
times the gains of tests/golden/featured_live.json; tests/test_model_teeth.py holds the conditions on them), and the fixtures the
accuracy suite did not hold yet. Every model runs on every kernel that accepts it, each asserted by name:

    generic_calls    nam_generic_kernel, 11 x 64 frames, then 37 + 27
    wn_reg_calls     nam_wn_reg_kernel, the same calls
    wn_reg_launch    nam_wn_reg_kernel, one 512-frame launch (the forms with several wavefronts per stream), then the other 256
    wn_reg_session   nam_wn_reg_kernel, a persistent session of twelve 64-frame commands

The yardstick is e32, the strict float32 oracle's own error against the truth. One exception, fixed by what the kernel computes
(profiles/accuracy/README.md): nam_wn_reg_kernel in libm mode on a model with a Tanh, Sigmoid or SiLU evaluates them in the exp2 /
rcp forms (kernel_wn_reg.hip: wr_act1 -> device_common.h: mf::act_hw) and is held to e32_exp2, the float32 oracle built with
those forms. nam_generic_kernel calls tanhf / expf (d_act) and keeps e32. Every run prints an ACCURACY line with its ratio.
"""
import numpy as np
import pytest

import accuracy
import model_teeth as mt
from conftest import model_path

pytestmark = pytest.mark.gpu

RAGGED = [64] * 11 + [37, 27]
GENERIC, WN_REG = "nam_generic_kernel", "nam_wn_reg_kernel"
TABLE_FORM_SEEDS = [5, 7, 15, 33, 43]  # 5: three input channels; 7, 15, 33: gated, FiLMs with shift, a nested condition; 43: a post-stack head


def _host_calls(nam, model, x, kernel, kname, max_frames, plan):
    b = model.batch(accuracy.N_STREAMS, max_frames)
    b.set_kernel(kernel)
    for m in sorted(set(plan)):
        assert b.kernel_name(m) == kname, (m, b.kernel_name(m), kname)
    b.Reset(prewarm=True)
    parts, a = [], 0
    for m in plan:
        parts.append(b.process(x[..., a:a + m]))
        a += m
    b.close()
    assert a == x.shape[-1]
    return np.concatenate(parts, axis=-1)


def _session(nam, model, x, kname, kernel=None):
    """A persistent session of 64-frame commands over a device-resident window [streams][channels][frames], one flush."""
    import torch
    b = model.batch(accuracy.N_STREAMS, 64)
    if kernel is not None:
        b.set_kernel(kernel)
    b.Reset(prewarm=True)
    assert b.set_persistent(True) and b.kernel_name() == kname, b.kernel_name()
    x3 = x if x.ndim == 3 else x[:, None, :]
    assert x3.shape[1] == model.NumInputChannels()
    T = x3.shape[2]
    xd = torch.from_numpy(x3.copy()).cuda()
    yd = torch.zeros((x3.shape[0], model.NumOutputChannels(), T), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for k in range(T // 64):
        b.process_device(xd.data_ptr() + k * 64 * 4, yd.data_ptr() + k * 64 * 4, 64, T)
    b.flush()
    b.synchronize()
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    b.close()
    return y


def _op_program_runs(nam, model):
    """(label, kernel it must run on, how) for a model of the op program: the interpreter, and nam_wn_reg_kernel where it accepts it."""
    runs = [("generic_calls", GENERIC, lambda x: _host_calls(nam, model, x, nam.KERNEL_GENERIC, GENERIC, 64, RAGGED))]
    if model.info.has_a1_kernel & 16:
        runs += [("wn_reg_calls", WN_REG, lambda x: _host_calls(nam, model, x, nam.KERNEL_WN_REG, WN_REG, 64, RAGGED)),
                 ("wn_reg_launch", WN_REG, lambda x: _host_calls(nam, model, x, nam.KERNEL_WN_REG, WN_REG, 512, [512, 256])),
                 ("wn_reg_session", WN_REG, lambda x: _session(nam, model, x, WN_REG, nam.KERNEL_WN_REG))]
    return runs


def _hold(runs, label, t, x, fast_tanh, amplitude, exp2_kernels, census):
    """Runs every (case, kernel, how) on x, prints its ACCURACY line, and asserts all of them against 4 x their yardstick."""
    over = []
    for case, kname, how in runs:
        y = how(x)
        assert y.dtype == np.float32 and np.isfinite(y).all(), (label, case)
        exp2 = (not fast_tanh) and kname in exp2_kernels
        yard = t.e32_exp2 if exp2 else t.e32
        e_gpu = t.error(y.reshape(t.truth.shape))
        ratio = e_gpu / yard if yard > 0 else float("inf") if e_gpu > 0 else 0.0
        print(f"ACCURACY {case} {kname} {label} fast_tanh={int(fast_tanh)} amp={amplitude} yardstick={'exp2' if exp2 else 'libm'} "
              f"peak={t.peak:.3f} e32={yard:.3e} e_gpu={e_gpu:.3e} e_gpu/e32={ratio:.2f} tanhf_e32={t.e32:.3e} census={census}")
        if not e_gpu <= accuracy.FACTOR * yard:
            over.append((case, kname, e_gpu, yard, round(ratio, 2)))
    assert not over, (label, fast_tanh, amplitude, over)


def _census(row):
    return f"{row['unnoticed']}/{row['sampled']}"


# ---------------------------------------------------------------------------
# The live feature-rich models
# ---------------------------------------------------------------------------
def _live_params():
    out = []
    for r in mt.live_rows():
        seed = r["seed"]
        modes = [mt.fast_tanh_of(seed)] + ([not mt.fast_tanh_of(seed)] if mt.has_smooth_activation(mt.live_document(seed)) else [])
        out += [(seed, ft, amp) for ft in modes for amp in (2.7, 1.0)]
    return out


LIVE_PARAMS = _live_params()


def _load_live(nam, tmp_path, seed, fast_tanh):
    row = next(r for r in mt.live_rows() if r["seed"] == seed)
    path = str(tmp_path / f"featured_{seed}.nam")
    doc = mt.featured(seed, row["gain"], path)
    assert doc == mt.live_document(seed)
    return row, doc, nam.get_dsp(path, fast_tanh=fast_tanh)


@pytest.mark.parametrize("seed,fast_tanh,amplitude", LIVE_PARAMS, ids=[f"{s}-{'fast' if f else 'libm'}-x{a}" for s, f, a in LIVE_PARAMS])
def test_live_featured_model_within_four_e32_of_the_truth(nam_lib, tmp_path, seed, fast_tanh, amplitude):
    nam = nam_lib
    row, doc, model = _load_live(nam, tmp_path, seed, fast_tanh)
    if seed % 2:
        assert model.info.has_a1_kernel & 16 or model.wr_why(), "a model of instantiated shapes must say why it was refused"
    t = mt.live_truth(seed, fast_tanh, amplitude)
    x = mt.inputs(mt.in_channels(doc), amplitude)
    exp2_kernels = {WN_REG} if mt.has_smooth_activation(doc) else set()
    _hold(_op_program_runs(nam, model), f"featured_{seed}", t, x, fast_tanh, amplitude, exp2_kernels, _census(row))


_TABLE_FEATURES = set().union(*[mt.features(mt.live_document(s)) for s in TABLE_FORM_SEEDS])
assert {"gating:gated", "condition_dsp"} <= _TABLE_FEATURES and any(f.endswith(":shift") for f in _TABLE_FEATURES)
assert all(s in [r["seed"] for r in mt.live_rows()] for s in TABLE_FORM_SEEDS)


@pytest.mark.parametrize("amplitude", [2.7, 1.0])
@pytest.mark.parametrize("seed", TABLE_FORM_SEEDS)
def test_live_featured_model_on_the_table_form(nam_lib, tmp_path, monkeypatch, seed, amplitude):
    """nam_wn_reg_kernel without the compiled-in program (NAM_HIP_WR_PROGRAM=0: the ahead-of-time kernels walk the op table), in a
    session, as test_wn_reg_without_the_compiled_in_program runs it — on live models, against the float64 bound."""
    nam = nam_lib
    monkeypatch.setenv("NAM_HIP_WR_PROGRAM", "0")
    fast_tanh = mt.fast_tanh_of(seed)
    row, doc, model = _load_live(nam, tmp_path, seed, fast_tanh)
    assert model.info.has_a1_kernel & 16, model.wr_why()
    t = mt.live_truth(seed, fast_tanh, amplitude)
    x = mt.inputs(mt.in_channels(doc), amplitude)
    runs = [("wn_reg_table_session", WN_REG, lambda x: _session(nam, model, x, WN_REG, nam.KERNEL_WN_REG))]
    _hold(runs, f"featured_{seed}", t, x, fast_tanh, amplitude, {WN_REG} if mt.has_smooth_activation(doc) else set(), _census(row))


# ---------------------------------------------------------------------------
# The fixtures the accuracy suite did not hold yet, each on the kernels its parity test names
# ---------------------------------------------------------------------------
def _a1_mfma(nam, model):
    return [("a1_mfma_calls", "nam_a1_mfma_kernel", lambda x: _host_calls(nam, model, x, nam.KERNEL_A1_MFMA, "nam_a1_mfma_kernel", 64, RAGGED))]


def _a1_mfma_and_q(nam, model):
    return _a1_mfma(nam, model) + [("q_session", "nam_a1_q_kernel", lambda x: _session(nam, model, x, "nam_a1_q_kernel"))]


def _ktap(nam, model):
    return [("kt_mfma_calls", "nam_kt_mfma_kernel", lambda x: _host_calls(nam, model, x, nam.KERNEL_A1_MFMA, "nam_kt_mfma_kernel", 64, RAGGED)),
            ("a1_valu_calls", "nam_a1_kernel", lambda x: _host_calls(nam, model, x, nam.KERNEL_A1, "nam_a1_kernel", 64, RAGGED))]


def _lut(nam, model):
    """test_lookup_table_activations_match_oracle runs what AUTO picks; a table is read by the interpreter alone (device_common.h: d_lut)."""
    return [("auto_calls", GENERIC, lambda x: _host_calls(nam, model, x, nam.KERNEL_AUTO, GENERIC, 64, RAGGED))]


FIXTURE_RUNS = dict([(n, _op_program_runs) for n in ("wavenet_condition_dsp", "synth_multich", "synth_leakyhardtanh", mt.POSTHEAD_LIVE)]
                    + [(n, _a1_mfma_and_q if n == "synth_a1_lite" else _a1_mfma) for n in mt.SYNTH_A1]
                    + [(n, _ktap) for n in mt.SYNTH_KT] + [(n, _lut) for n in mt.LUTS])
DEAD_FIXTURES = sorted(n for n, r in mt.load_fixture_table().items() if r["dead"])  # they stay in their flat-bound parity tests
assert DEAD_FIXTURES == ["synth_posthead"], DEAD_FIXTURES


def _fixture_params():
    out = []
    for name in FIXTURE_RUNS:
        doc, luts = mt.fixture_document(name)
        smooth = mt.has_smooth_activation(doc)
        # a lookup table replaces the function that fast_tanh would: one mode says it all — but for "wavenet", whose parity
        # test runs both to show that the table wins
        modes = (True, False) if (smooth and not luts) or name == "lut_wavenet" else (False,) if luts else (True,)
        out += [(name, ft, amp) for ft in modes for amp in (2.7, 1.0)]
    return out


FIXTURE_PARAMS = _fixture_params()


@pytest.mark.parametrize("name,fast_tanh,amplitude", FIXTURE_PARAMS, ids=[f"{n}-{'fast' if f else 'libm'}-x{a}" for n, f, a in FIXTURE_PARAMS])
def test_fixture_within_four_e32_of_the_truth(nam_lib, tmp_path, name, fast_tanh, amplitude):
    nam = nam_lib
    doc, luts = mt.fixture_document(name)
    path = mt.write_fixture(name, str(tmp_path / (name + ".nam"))) if name == mt.POSTHEAD_LIVE else model_path(mt.LUTS.get(name, (name,))[0])
    model = nam.get_dsp(path, fast_tanh=fast_tanh, luts=luts) if luts else nam.get_dsp(path, fast_tanh=fast_tanh)
    t = mt.fixture_truth(name, fast_tanh, amplitude)
    x = mt.inputs(mt.in_channels(doc), amplitude)
    exp2_kernels = {WN_REG} if mt.has_smooth_activation(doc) else set()  # (no table reaches nam_wn_reg_kernel)
    _hold(FIXTURE_RUNS[name](nam, model), name, t, x, fast_tanh, amplitude, exp2_kernels, _census(mt.load_fixture_table()[name]))
