"""-m gpu accuracy tests: every kernel against the float64 truth of the function it computes, within FOUR times the error
the strict float32 oracle itself has on that input (tests/accuracy.py; the yardstick is checked on the CPU by
tests/test_oracle_truth.py, the measured ratios are recorded in profiles/accuracy/README.md):

    max |gpu - truth| <= 4 e32      over 8 streams x 768 frames, amplitudes 1 and 2.7, Reset(prewarm=True) on both sides

The parity tests' flat 5e-5 max(1, |y|) is 14 to 500 times wider than that and lets a constant with a wrong fifth digit
through. Every case asserts the kernel it ran on, so none can drift onto another one. The libm-mode cases of
wavenet_a1_standard on the four kernels that evaluate tanh as 1 - 2 / (exp2(2 x log2 e) + 1) (q, p4, p2, mfma) are held to the
float32 oracle built with that form (accuracy.EXP2_FORM_CASES says why: against tanhf's e32 nam_a1_p2_kernel and
nam_a1_mfma_kernel measure 4.5 and 4.9 at amplitude 1, an error of the form that the CPU build reproduces without a GPU; against
the form's own e32 they measure 1.8 and 2.0). nam_a1_kernel and nam_generic_kernel call tanhf and keep tanhf's yardstick.
"""
import numpy as np
import pytest

import accuracy
from conftest import model_path

pytestmark = pytest.mark.gpu

RAGGED = [64] * 11 + [37, 27]  # 768 frames: eleven buffers, then one cut in two
BLOCKS = [64] * 12
Q, P4 = "nam_a1_q_kernel", "nam_a1_p4_kernel"


def _calls(b, x, plan):
    """Blocking host calls of plan[i] frames each."""
    parts, a = [], 0
    for m in plan:
        parts.append(b.process(x[:, a:a + m]))
        a += m
    return np.concatenate(parts, axis=-1), []


def _session(b, x, bursts):
    """A persistent session over a device-resident window: 64-frame commands, a flush after each burst. Returns the
    output and the kernel each burst's launch started as."""
    import torch
    xd = torch.from_numpy(x[:, None, :].copy()).cuda()
    yd = torch.zeros((x.shape[0], b.model.NumOutputChannels(), x.shape[1]), dtype=torch.float32, device="cuda")
    assert b.model.NumInputChannels() == 1 and b.model.NumOutputChannels() == 1
    torch.cuda.synchronize()
    k, names = 0, []
    for burst in bursts:
        names.append(b.kernel_name())
        for _ in range(burst):
            b.process_device(xd.data_ptr() + k * 64 * 4, yd.data_ptr() + k * 64 * 4, 64, x.shape[1])
            k += 1
        b.flush()
    b.synchronize()
    torch.cuda.synchronize()
    assert k * 64 == x.shape[1]
    return yd.cpu().numpy(), names


def _forced(kernel, kname, plan=RAGGED, prefix=False):
    def run(nam, model, x):
        b = model.batch(accuracy.N_STREAMS, 64)
        if kernel is not None:
            b.set_kernel(getattr(nam, kernel))
        for m in sorted(set(plan)):  # every call length of the plan, the ragged 37 and 27 included
            got = b.kernel_name(m)
            assert got.startswith(kname) if prefix else got == kname, (m, got, kname)
        b.Reset(prewarm=True)
        y, _ = _calls(b, x, plan)
        b.close()
        return y
    return run


def _in_session(kname, bursts=(12,), want_names=None, widths=None):
    def run(nam, model, x):
        b = model.batch(accuracy.N_STREAMS, 64)
        b.Reset(prewarm=True)
        for ratio, streams in (widths or {}).items():
            b.SetSlimmableSize(ratio, streams)
        assert b.set_persistent(True) and b.kernel_name() == kname, b.kernel_name()
        y, names = _session(b, x, bursts)
        b.close()
        assert names == (want_names or [kname] * len(bursts)), names
        return y
    return run


SLIM_WIDTHS = {0.0: [0, 2, 4, 6], 1.0: [1, 3, 5, 7]}

# case -> (model, how it runs). The short-burst case: after three bursts of at most four buffers a session of the official topology
# starts its launches as nam_a1_p4_kernel (test_gpu_breadth.py: test_short_bursts_start_the_low_latency_kernel); the first three
# bursts — one buffer each — are nam_a1_q_kernel's, the other nine buffers nam_a1_p4_kernel's, on the same stream state.
CASES = {
    "q_session": ("wavenet_a1_standard", _in_session(Q)),
    "q_session_feather": ("synth_a1_feather", _in_session(Q)),
    "p4_short_bursts": ("wavenet_a1_standard", _in_session(Q, bursts=(1, 1, 1, 2, 1, 2, 1, 2, 1), want_names=[Q] * 3 + [P4] * 6)),
    "p4_session_relu": ("synth_a1_feather_relu", _in_session(P4)),
    "p2_buffers": ("wavenet_a1_standard", _forced("KERNEL_A1_IL", "nam_a1_p2_kernel")),
    "a1_mfma": ("wavenet_a1_standard", _forced("KERNEL_A1_MFMA", "nam_a1_mfma_kernel")),
    "a1_valu": ("wavenet_a1_standard", _forced("KERNEL_A1", "nam_a1_kernel")),
    "generic": ("wavenet_a1_standard", _forced("KERNEL_GENERIC", "nam_generic_kernel")),
    "kq_session": ("A2", _in_session("nam_kq_kernel")),
    "kt_mfma_blocks": ("A2", _forced(None, "nam_kt_mfma_kernel", plan=BLOCKS)),
    "wn_reg_a2_max": ("wavenet_a2_max", _in_session("nam_wn_reg_kernel")),
    "wn_reg_nano": ("synth_a1_nano", _forced("KERNEL_WN_REG", "nam_wn_reg_kernel")),
    "wn_reg_slimmable": ("slimmable_wavenet", _in_session("nam_wn_reg_kernel", widths=SLIM_WIDTHS)),
    "lstm_row": ("lstm", _forced(None, "nam_lstm_row_kernel", plan=BLOCKS, prefix=True)),
    "lstm_wide": ("synth_lstm_h18x2", _forced(None, "nam_lstm_wide_kernel", plan=BLOCKS, prefix=True)),
    "lstm_mfma": ("lstm", _forced("KERNEL_A1_MFMA", "nam_lstm_mfma", plan=BLOCKS, prefix=True)),
    "lstm_lanes": ("lstm", _forced("KERNEL_GENERIC", "nam_lstm_kernel", plan=BLOCKS)),
}
assert all(CASES[c][0] == accuracy.EXP2_FORM_MODEL for c in accuracy.EXP2_FORM_CASES)
PARAMS = [(case, ft, amp) for case, (name, _) in CASES.items() for ft in accuracy.fast_tanh_values(name) for amp in accuracy.AMPLITUDES]


@pytest.mark.parametrize("case,fast_tanh,amplitude", PARAMS, ids=[f"{c}-{'fast' if f else 'libm'}-x{a}" for c, f, a in PARAMS])
def test_kernel_within_four_e32_of_the_truth(nam_lib, case, fast_tanh, amplitude):
    nam = nam_lib
    name, run = CASES[case]
    x = accuracy.inputs(amplitude)
    model = nam.get_dsp(model_path(name), fast_tanh=fast_tanh)
    y = run(nam, model, x)
    assert y.dtype == np.float32 and np.isfinite(y).all()
    exp2 = (not fast_tanh) and case in accuracy.EXP2_FORM_CASES
    # one yardstick per width of the batch; a stream is held to the e32 of its own width
    groups = SLIM_WIDTHS.items() if name == "slimmable_wavenet" else [(None, list(range(accuracy.N_STREAMS)))]
    for ratio, streams in groups:
        ys = accuracy.yardstick(name, fast_tanh, amplitude, ratio)
        e32 = ys.e32_exp2 if exp2 else ys.e32
        e_gpu = float(np.max(np.abs(y[streams].astype(np.float64) - ys.truth[streams])))
        print(f"ACCURACY {case} {name} ratio={ratio} fast_tanh={int(fast_tanh)} amp={amplitude} yardstick={'exp2' if exp2 else 'libm'} "
              f"peak={ys.peak:.3f} e32={e32:.3e} e_gpu={e_gpu:.3e} e_gpu/e32={e_gpu / e32:.2f} tanhf_e32={ys.e32:.3e}")
        assert e_gpu <= accuracy.FACTOR * e32, (case, ratio, e_gpu, e32, e_gpu / e32)
