"""Lone-buffer launches through the host wrappers whose dynamic-LDS request can pass the 64 KB a launch gets by default
(csrc/kernels.h: launch_instance raises the limit once per kernel instantiation and device), on the first device and, where
there is one, on a second device of the same process."""
import ctypes

import numpy as np
import pytest

from conftest import model_path
from signals import stream_bank

pytestmark = pytest.mark.gpu

N_STREAMS, BLOCK, N = 3, 64, 64 * 2 + 5
# (fixture, kernel to force or None = AUTO, the kernel a one-buffer launch then runs)
A1_MFMA = ("wavenet_a1_standard", None, "nam_a1_mfma_kernel")  # AUTO's choice for lone buffers of the official sizes
WN_REG = ("synth_a1_nano", "KERNEL_WN_REG", "nam_wn_reg_kernel")  # 68 KB of LDS-resident rings
LSTM_MFMA = ("synth_lstm_h32", "KERNEL_A1_MFMA", "nam_lstm_mfma_kernel")  # 8 unit tiles: weights in LDS, not in registers (its
# request stays below 64 KB: here for the kernel the second-device test launches, on the first device too)
# nam_lstm_kernel above 64 KB: test_gpu_breadth.py::test_lstm_larger_than_lds_runs_from_global_scratch.
# nam_generic_kernel: no fixture's rows plus weights pass 64 KB (the largest, wavenet_a2_max, asks for 46 KB).


def _tol(fast_tanh):  # test_gpu_parity.py
    return 5e-5 if fast_tanh else 1e-4


def _lone_buffers_match_oracle(nam, oracle, case, fast_tanh, device):
    name, kernel, want = case
    x = stream_bank(N_STREAMS, N, seed=17)
    model = nam.get_dsp(model_path(name), fast_tanh=fast_tanh)
    b = model.batch(N_STREAMS, BLOCK, device=device)
    if kernel:
        b.set_kernel(getattr(nam, kernel))
    assert b.kernel_name() == want
    b.Reset(prewarm=True)
    y = b.process_stream(x, BLOCK)
    b.close()
    for s in range(N_STREAMS):
        ref = oracle.get_dsp(model_path(name), fast_tanh=fast_tanh)
        ref.Reset(48000.0, BLOCK)
        r = ref.process_stream(x[s], BLOCK)
        err, scale = float(np.max(np.abs(r - y[s]))), max(1.0, float(np.max(np.abs(r))))
        assert err <= _tol(fast_tanh) * scale, (name, device, s, err, scale)


@pytest.mark.parametrize("case", [A1_MFMA, WN_REG, LSTM_MFMA], ids=lambda c: c[2])
@pytest.mark.parametrize("fast_tanh", [True, False])
def test_lone_buffer_above_64_kb_of_lds(nam_lib, oracle, case, fast_tanh):
    _lone_buffers_match_oracle(nam_lib, oracle, case, fast_tanh, 0)


@pytest.mark.parametrize("case", [A1_MFMA, LSTM_MFMA], ids=lambda c: c[2])
def test_second_device_raises_its_own_lds_limit(nam_lib, oracle, case):
    """The limit belongs to the current device's copy of a kernel: a batch on device 0 runs first, then one on device 1."""
    count = ctypes.c_int(0)
    assert nam_lib.load_library().nam_hip_device_count(ctypes.byref(count)) == 0
    if count.value < 2:
        pytest.skip("one visible device")
    for device in (0, 1):
        _lone_buffers_match_oracle(nam_lib, oracle, case, True, device)
