"""-m gpu tests of Linear models (impulse responses) on nam_linear_kernel, against tests/linear_oracle.py:

    max |gpu - truth| <= 4 e32,   e32 = max(strict float32 oldest-first, newest-first) against the float64 truth

and, where one product decides a sample, bit for bit. The measured ratios are recorded in profiles/linear/README.md; every
case prints its figure before it asserts.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import linear_oracle as lo
from conftest import ROOT

pytestmark = pytest.mark.gpu
KERNEL = "nam_linear_kernel"


def _model(nam, doc):
    return nam.get_dsp_json(json.dumps(doc))


def _render64(nam, doc, x, max_frames=64):
    """x [streams, N] or [streams, in_ch, N] through a fresh batch in 64-frame blocking calls."""
    m = _model(nam, doc)
    b = m.batch(x.shape[0], max_frames)
    assert b.kernel_name() == KERNEL
    y = b.process_stream(x, 64)
    b.close()
    return y


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. accuracy ----
@pytest.mark.parametrize("amplitude", lo.AMPLITUDES)
@pytest.mark.parametrize("R,bias", lo.ACCURACY_CASES)
def test_accuracy(nam_lib, R, bias, amplitude):
    ys = lo.yardstick(R, bias, amplitude)
    y = _render64(nam_lib, lo.linear_doc(R, bias, seed=R), ys.x)[:, 0, :]
    print(f"linear accuracy R={R} bias={bias} amplitude={amplitude}: e32={ys.e32:.3e} ratio={ys.ratio(y):.3f}")
    assert ys.passes(y), ys.ratio(y)


# ---- 2. teeth ----
@pytest.mark.parametrize("R,k", sorted(lo.TEETH.items()))
def test_teeth(nam_lib, R, k):
    """One tap off by 1 + 2^-k: the GPU must FAIL the bound."""
    for amplitude in lo.AMPLITUDES:
        ys = lo.yardstick(R, True, amplitude)
        y = _render64(nam_lib, lo.perturbed(lo.linear_doc(R, True, seed=R), k), ys.x)[:, 0, :]
        print(f"linear teeth R={R} 2^-{k} amplitude={amplitude}: ratio={ys.ratio(y):.1f}")
        assert not ys.passes(y), ys.ratio(y)


# ---- 3. every tap, exactly ----
@pytest.mark.parametrize("R", [65, 4099])
def test_every_tap_exactly(nam_lib, R):
    doc = lo.linear_doc(R, True, seed=R)
    h, b = lo.taps_and_bias(doc)
    n = R + 64
    x = np.zeros((3, n), dtype=np.float32)
    x[1, 5] = 1.0
    y = _render64(nam_lib, doc, x)[:, 0, :]
    want = np.full((3, n), b, dtype=np.float32)
    want[1, 5:5 + R] = (h + b).astype(np.float32)  # one non-zero product per output: no order involved
    bad = np.argwhere(_bits(y) != _bits(want))
    assert bad.size == 0, (bad[:8], y[tuple(bad[0])], want[tuple(bad[0])])


# ---- 4. stream counts and isolation ----
@pytest.mark.parametrize("n_streams", [1, 3, 33, 257])
def test_stream_counts_and_isolation(nam_lib, n_streams):
    R, n = 257, 256
    doc = lo.linear_doc(R, True, seed=R)
    h, b = lo.taps_and_bias(doc)
    x = np.zeros((n_streams, n), dtype=np.float32)
    x[-1] = lo.inputs(n, 2.7)[0]
    y = _render64(nam_lib, doc, x)[:, 0, :]
    assert np.array_equal(_bits(y[:-1]), _bits(np.full((n_streams - 1, n), b, dtype=np.float32)))  # silent streams: exactly b
    ys = lo.Yardstick(h, b, x[-1:])
    print(f"linear streams={n_streams}: ratio={ys.ratio(y[-1:]):.3f}")
    assert ys.passes(y[-1:]), ys.ratio(y[-1:])


def test_same_bits_at_any_stream_count(nam_lib):
    R = 1025
    doc = lo.linear_doc(R, True, seed=R)
    x = lo.inputs(768, 1.0)
    y8 = _render64(nam_lib, doc, x)
    y1 = _render64(nam_lib, doc, x[3:4])
    y40 = _render64(nam_lib, doc, np.concatenate([x] * 5))
    assert np.array_equal(_bits(y8[3]), _bits(y1[0])) and np.array_equal(_bits(y40[35]), _bits(y1[0]))
    assert np.array_equal(_bits(_render64(nam_lib, doc, x)), _bits(y8))  # run to run


# ---- 5. channels ----
@pytest.mark.parametrize("in_ch,out_ch", [(2, 3), (3, 2)])
def test_channels(nam_lib, in_ch, out_ch):
    R, n, S = 65, 768, 3
    doc = lo.linear_doc(R, True, in_ch=in_ch, out_ch=out_ch, seed=R)
    h, b = lo.taps_and_bias(doc)
    bank = lo.inputs(n, 1.0)
    x = np.stack([np.stack([bank[(in_ch * s + c) % lo.N_STREAMS] * np.float32(1.0 + 0.5 * c) for c in range(in_ch)]) for s in range(S)])
    y = _render64(nam_lib, doc, x)
    assert y.shape == (S, out_ch, n)
    for c in range(min(in_ch, out_ch)):  # every channel its own input, the same impulse response
        ys = lo.Yardstick(h, b, np.ascontiguousarray(x[:, c, :]))
        print(f"linear channels in={in_ch} out={out_ch} ch={c}: ratio={ys.ratio(y[:, c, :]):.3f}")
        assert ys.passes(y[:, c, :]), (c, ys.ratio(y[:, c, :]))
    for c in range(min(in_ch, out_ch), out_ch):  # 0, not the bias
        assert np.array_equal(_bits(y[:, c, :]), np.zeros((S, n), dtype=np.uint32))


# ---- 6. partitions and wrap ----
@pytest.fixture(scope="module")
def long_case():
    R, n = 257, 20000
    doc = lo.linear_doc(R, True, seed=R)
    h, b = lo.taps_and_bias(doc)
    from signals import stream_bank
    x = np.ascontiguousarray(stream_bank(4, n, seed=3))
    return doc, x, lo.Yardstick(h, b, x)


def _hist_frames(model):
    return int(re.search(r"hist_frames=(\d+)", model.describe()).group(1))


@pytest.mark.parametrize("partition", ["ragged", "blocks"])
def test_partitions_and_wrap_host_calls(nam_lib, long_case, partition):
    doc, x, ys = long_case
    m = _model(nam_lib, doc)
    n = x.shape[1]
    assert 3 * _hist_frames(m) <= n  # a condition: the history ring wraps at least three times
    assert m.info.state_bytes_per_stream == 4 * _hist_frames(m)
    b = m.batch(4, 256)
    lengths = [1, 64, 63, 65, 17, 128, 200, 256] if partition == "ragged" else [64]
    parts, at, i = [], 0, 0
    while at < n:
        k = min(lengths[i % len(lengths)], n - at)
        parts.append(b.process(x[:, at:at + k]))
        at += k
        i += 1
    b.close()
    y = np.concatenate(parts, axis=-1)[:, 0, :]
    print(f"linear partition {partition}: ratio={ys.ratio(y):.3f}")
    assert ys.passes(y), ys.ratio(y)


def test_partitions_one_device_launch_and_render(nam_lib, long_case):
    import torch
    doc, x, ys = long_case
    m = _model(nam_lib, doc)
    n, stride = x.shape[1], x.shape[1] + 32
    # one process_device launch on a non-default stream, frame_stride > n_frames
    b = m.batch(4, 256)
    xd = torch.zeros((4, 1, stride), dtype=torch.float32, device="cuda")
    xd[:, 0, :n] = torch.from_numpy(x).cuda()
    yd = torch.full((4, 1, stride), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert b.kernel_name(n) == KERNEL
    b.process_device(xd.data_ptr(), yd.data_ptr(), n, stride, s.cuda_stream)
    s.synchronize()
    b.synchronize()
    y = yd.cpu().numpy()
    b.close()
    assert np.all(y[:, 0, n:] == 7.0)  # nothing behind n_frames is written
    print(f"linear one launch: ratio={ys.ratio(y[:, 0, :n]):.3f}")
    assert ys.passes(y[:, 0, :n]), ys.ratio(y[:, 0, :n])
    # one render with four unequal lengths
    b = m.batch(4, 256)
    lengths = [n, n - 1, 12345, 65]
    outs = b.render([x[i, :lengths[i]] for i in range(4)])
    b.close()
    for i in range(4):
        e = lo.error(outs[i][0], ys.truth[i, :lengths[i]])
        print(f"linear render stream {i} ({lengths[i]} frames): ratio={e / ys.e32:.3f}")
        assert outs[i].shape == (1, lengths[i]) and e <= lo.FACTOR * ys.e32, (i, e / ys.e32)


# ---- 7. reset ----
def test_reset_zeroes_the_history(nam_lib):
    R = 257
    doc = lo.linear_doc(R, True, seed=R)
    _, bias = lo.taps_and_bias(doc)
    b = _model(nam_lib, doc).batch(3, 64)
    noise = np.random.default_rng(7).uniform(-1, 1, size=(3, 5 * 64 + 17)).astype(np.float32)
    silence = np.zeros((3, 2 * R), dtype=np.float32)
    want = _bits(np.full((3, 2 * R), bias, dtype=np.float32))
    for prewarm in (True, False):
        y = b.process_stream(noise, 64)
        assert np.any(y != bias)
        b.Reset(prewarm=prewarm)
        assert np.array_equal(_bits(b.process_stream(silence, 64)[:, 0, :]), want), prewarm
    b.close()


# ---- 8. the rest of the surface ----
def test_surface(nam_lib):
    nam = nam_lib
    R = 257
    doc = lo.linear_doc(R, True, seed=R)
    ys = lo.yardstick(R, True, 1.0)
    x = ys.x
    m = _model(nam, doc)
    b = m.batch(lo.N_STREAMS, 64)
    assert b.kernel_name() == KERNEL and b.kernel_name(4096) == KERNEL
    y32 = b.process_stream(x, 64)
    # process_f64 equals process_f32, cast
    b.Reset()
    y64 = b.process_stream(x.astype(np.float64), 64)
    assert y64.dtype == np.float64 and np.array_equal(y64, y32.astype(np.float64))
    # submit / wait with 16 tickets in flight at once equals the blocking calls bit for bit (the 12 buffers of x, then 4 of them again)
    b.Reset()
    blocks = [x[:, i:i + 64] for i in range(0, x.shape[1], 64)] + [x[:, i:i + 64] for i in range(0, 256, 64)]
    assert len(blocks) == 16
    tickets = [b.submit(blk) for blk in blocks]
    got = np.concatenate([b.wait(t) for t in tickets], axis=-1)
    b.Reset()
    want = np.concatenate([b.process(blk) for blk in blocks], axis=-1)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got[:, :, :768]), _bits(y32))
    # persistent mode: not eligible, calls launch as usual
    b.Reset()
    assert b.set_persistent(True) is False
    yp = b.process_stream(x, 64)
    assert np.array_equal(_bits(yp), _bits(y32)) and ys.passes(yp[:, 0, :])
    t = b.submit(x[:, :64])
    assert b.wait(t).shape == (lo.N_STREAMS, 1, 64)
    b.set_persistent(False)
    # kernel choice: AUTO only
    b.set_kernel(nam.KERNEL_AUTO)
    with pytest.raises(nam.NamHipError, match="nam_linear_kernel only") as e:
        b.set_kernel(nam.KERNEL_A1_MFMA)
    assert e.value.code == nam.ERR_UNSUPPORTED
    assert b.get_kernel() == nam.KERNEL_AUTO and b.kernel_name() == KERNEL
    b.SetSlimmableSize(0.5)  # what it does for any non-slimmable model: nothing
    b.Reset()
    assert np.array_equal(_bits(b.process_stream(x, 64)), _bits(y32))
    # process_tensor
    import torch
    b.Reset()
    yt = b.process_tensor(torch.from_numpy(x[:, None, :].copy()).cuda())
    torch.cuda.synchronize()
    assert ys.passes(yt.cpu().numpy()[:, 0, :])
    b.close()


# ---- 9. the C++ adapter ----
def test_cpp_adapter_linear_check(nam_lib):
    """cpp/tools/linear_check: nam::get_dsp(path) + nam::DSP::process on the Linear fixture, the adapter's sources unchanged."""
    from signals import two_tone
    tool = os.path.join(ROOT, "cpp", "tools", "linear_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/linear_check"
    path = os.path.join(ROOT, "tests", "golden", "linear", "linear_r65.nam")  # (not golden/models: see make_linear_models.py)
    with open(path) as f:
        doc = json.load(f)
    assert doc == lo.linear_doc(65, True, seed=65)  # tests/golden/make_linear_models.py
    n = 768
    r = subprocess.run([tool, path, str(n)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    head = dict(l.split() for l in lines[:lines.index(f"y {n}")])
    assert head == {"in_channels": "1", "out_channels": "1", "prewarm_samples": "0", "sample_rate": "48000", "has_loudness": "0"}
    at = lines.index(f"y {n}")
    y = np.array([float(v) for v in lines[at + 1:at + 1 + n]], dtype=np.float64)
    h, b = lo.taps_and_bias(doc)
    ys = lo.Yardstick(h, b, two_tone(n)[None, :])
    print(f"linear_check: ratio={ys.ratio(y[None, :]):.3f}")
    assert ys.passes(y[None, :]), ys.ratio(y[None, :])
