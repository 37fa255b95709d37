"""-m gpu tests of a SlimmableContainer whose submodels are all Linear: one batch, one input ring, every stream on its own impulse
response (nam_linear_pairs_kernel over a work list of (column tile, submodel) pairs).

The contract is bit equality: a stream on submodel w produces the bits of a one-model Linear batch of w (nam_linear_kernel) fed the
same rows, counted from the stream's last reset or size change — same splits, taps oldest first as one fmaf chain, partial sums in
split order, the bias last. Accuracy against the float64 truth is linear_oracle's bound, max |gpu - truth| <= 4 e32. No stream and no
frame is left out of a comparison. The ring holds 9 x 128 + 512 = 1,664 frames at max_frames 64; the runs are 2,024 frames, so it wraps.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import linear_container as lc
import linear_oracle as lo
from conftest import ROOT
from signals import stream_bank

pytestmark = pytest.mark.gpu
KERNEL = "nam_linear_pairs_kernel"  # (the one-model batches: lc.one_model_outputs asserts nam_linear_kernel)
N_STREAMS = 70  # two full column tiles and a tile of 6
LENGTHS = [64] * 31 + [40]  # 2,024 frames: the 1,664-frame ring wraps
N = sum(LENGTHS)
# a fully mixed tile, a tile on one size, two sizes in the last tile
ASSIGN = [s % 4 for s in range(32)] + [2] * 32 + [0 if s % 2 else 3 for s in range(64, 70)]
bits = lc.bits


def _same(got, want, streams=None):
    """np.array_equal per stream; names the first stream and frame that differ."""
    for s in (range(got.shape[0]) if streams is None else streams):
        if not np.array_equal(bits(got[s]), bits(want[s])):
            at = int(np.argmax(bits(got[s]) != bits(want[s])))
            return f"stream {s} differs first at frame {at}: {got[s, at]!r} != {want[s, at]!r}"
    return ""


def _container_batch(nam, n_streams=N_STREAMS, sizes=None, doc=None, max_frames=64):
    b = lc.load(nam, doc or lc.container_doc()).batch(n_streams, max_frames)
    assert b.kernel_name() == KERNEL and b.kernel_name(4096) == KERNEL
    lc.assign(b, ASSIGN[:n_streams] if sizes is None else sizes)
    return b


def _run(b, x, lengths=LENGTHS):
    return np.concatenate([b.process(blk) for blk in lc.blocks_of(x, lengths)], axis=-1)[:, 0, :]


@pytest.fixture(scope="module")
def case(nam_lib):
    """The 70-stream input, what one-model batches make of it (the reference of every bit comparison), and the container's own
    blocking-call run. Computed once, read-only."""
    x = np.ascontiguousarray(stream_bank(N_STREAMS, N, seed=11), dtype=np.float32)
    want = lc.one_model_outputs(nam_lib, ASSIGN, x, LENGTHS)
    b = _container_batch(nam_lib)
    got = _run(b, x)
    b.close()
    for a in (x, want, got):
        a.setflags(write=False)
    return x, want, got


def _fresh_one_model(nam, w, row, lengths):
    """One stream on a one-model batch of submodel w, started fresh."""
    return lc.one_model_outputs(nam, [w], row[None, :], lengths)[0]


# ---- 1. bit for bit against one-model batches ----
def test_bits_of_one_model_batches_blocking_calls(nam_lib, case):
    x, want, got = case
    assert got.shape == (N_STREAMS, N)
    assert _same(got, want) == ""


def test_bits_of_one_model_batches_device_launch_and_render(nam_lib, case):
    import torch
    x, want, _ = case
    stride = N + 24
    b = _container_batch(nam_lib)
    xd = torch.zeros((N_STREAMS, 1, stride), dtype=torch.float32, device="cuda")
    xd[:, 0, :N] = torch.from_numpy(x.copy()).cuda()
    yd = torch.full((N_STREAMS, 1, stride), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    b.process_device(xd.data_ptr(), yd.data_ptr(), N, stride, s.cuda_stream)  # one launch of 2,024 frames: four pieces
    s.synchronize()
    b.synchronize()
    y = yd.cpu().numpy()
    b.close()
    assert np.all(y[:, 0, N:] == 7.0)  # frame_stride honoured: nothing behind n_frames is written
    assert _same(y[:, 0, :N], want) == ""
    b = _container_batch(nam_lib)
    outs = b.render([x[s] for s in range(N_STREAMS)])
    b.close()
    assert all(o.shape == (1, N) for o in outs)
    assert _same(np.stack([o[0] for o in outs]), want) == ""


# ---- 2. accuracy against the float64 truth ----
@pytest.mark.parametrize("w", range(4))
def test_accuracy(nam_lib, w):
    R = lc.SIZES[w]
    for amplitude in lo.AMPLITUDES:
        if R == 33:  # (not in linear_oracle's table: tests/test_linear_container_loader.py checks this yardstick's e32 > 0)
            h, bias = lo.taps_and_bias(lc.sub_doc(33))
            ys = lo.Yardstick(h, bias, lo.inputs(lo.n_frames_for(33), amplitude))
        else:
            ys = lo.yardstick(R, True, amplitude)
        b = _container_batch(nam_lib, lo.N_STREAMS, [w] * lo.N_STREAMS)
        y = b.process_stream(ys.x, 64)[:, 0, :]
        b.close()
        print(f"linear container accuracy R={R} amplitude={amplitude}: e32={ys.e32:.3e} ratio={ys.ratio(y):.3f}")
        for s in range(lo.N_STREAMS):
            e = lo.error(y[s], ys.truth[s])
            assert e <= lo.FACTOR * ys.e32, (s, e / ys.e32)


# ---- 3. teeth ----
def test_teeth(nam_lib):
    """Submodel 65's largest tap off by 1 + 2^-11: its streams must FAIL the bound, the streams of the other sizes keep their bits."""
    others = [0, 2, 3, 0, 2, 3, 0, 2]
    sizes = [1] * lo.N_STREAMS + others  # one column tile, mixed
    bad = lc.container_doc(subs={1: lo.perturbed(lc.sub_doc(65), lo.TEETH[65])})
    for amplitude in lo.AMPLITUDES:
        ys = lo.yardstick(65, True, amplitude)
        x = np.concatenate([ys.x, ys.x])
        outs = []
        for doc in (None, bad):
            b = _container_batch(nam_lib, len(sizes), sizes, doc)
            outs.append(b.process_stream(x, 64)[:, 0, :])
            b.close()
        good_y, bad_y = outs
        print(f"linear container teeth amplitude={amplitude}: ratio={ys.ratio(bad_y[:8]):.1f} (unperturbed {ys.ratio(good_y[:8]):.3f})")
        assert ys.passes(good_y[:8]), ys.ratio(good_y[:8])
        assert not ys.passes(bad_y[:8]), ys.ratio(bad_y[:8])
        assert _same(bad_y, good_y, range(8, 16)) == ""


# ---- 4. switching ----
def test_switching(nam_lib, case):
    x, _, got = case
    moves = {1: 3, 33: 0, 64: 1}  # stream -> its new submodel
    assert all(ASSIGN[s] != w for s, w in moves.items())
    k = 10
    at = 64 * k
    blocks = lc.blocks_of(x, LENGTHS)
    b = _container_batch(nam_lib)
    head = np.concatenate([b.process(blk) for blk in blocks[:k]], axis=-1)[:, 0, :]
    for s, w in moves.items():
        b.SetSlimmableSize(lc.RATIOS[w], [s])
    b.SetSlimmableSize(lc.RATIOS[ASSIGN[5]], [5])  # the size it already has: nothing changes
    b.SetSlimmableSize(lc.RATIOS[2], [s for s in range(32, 64) if s not in moves])  # the rest of a tile, likewise
    tail = np.concatenate([b.process(blk) for blk in blocks[k:]], axis=-1)[:, 0, :]
    assert _same(head, got[:, :at]) == ""
    stay = [s for s in range(N_STREAMS) if s not in moves]
    assert _same(tail, got[:, at:], stay) == ""  # every other stream: the bits of the run without the switch
    for s, w in moves.items():  # a moved stream: a one-model batch started fresh at that call
        assert np.array_equal(bits(tail[s]), bits(_fresh_one_model(nam_lib, w, x[s, at:], LENGTHS[k:]))), s
    # Reset zeroes everything and keeps the sizes
    b.Reset()
    again = np.concatenate([b.process(blk) for blk in blocks[:3]], axis=-1)[:, 0, :]
    b.close()
    assert _same(again, got[:, :192], stay) == ""
    for s, w in moves.items():
        assert np.array_equal(bits(again[s]), bits(_fresh_one_model(nam_lib, w, x[s, :192], LENGTHS[:3]))), s


# ---- 5. stream slots ----
def test_restart_streams(nam_lib, case):
    x, _, got = case
    k, at = 12, 64 * 12
    blocks = lc.blocks_of(x, LENGTHS)
    b = _container_batch(nam_lib)
    for blk in blocks[:k]:
        b.process(blk)
    b.restart_streams([3, 40])
    tail = np.concatenate([b.process(blk) for blk in blocks[k:]], axis=-1)[:, 0, :]
    b.close()
    assert _same(tail, got[:, at:], [s for s in range(N_STREAMS) if s not in (3, 40)]) == ""
    for s in (3, 40):  # zero history, the size kept
        assert np.array_equal(bits(tail[s]), bits(_fresh_one_model(nam_lib, ASSIGN[s], x[s, at:], LENGTHS[k:]))), s


def _blob_width(blob):
    return struct.unpack_from("<i", blob, 36)[0]  # stream_state.h: Header::width


def test_stream_state_moves_between_batches(nam_lib, case):
    x, _, got = case
    k, at = 12, 64 * 12
    blocks = lc.blocks_of(x, LENGTHS)
    a = _container_batch(nam_lib)
    for blk in blocks[:k]:
        a.process(blk)
    assert ASSIGN[5] == 1
    blob = a.get_stream_state(5)
    assert _blob_width(blob) == 1 and len(blob) == 80 + 4 * lc.RING_FRAMES
    # another stream count, another ring position, stream 40 on the largest size
    n2 = 41
    z = np.ascontiguousarray(stream_bank(n2, 5 * 64, seed=12), dtype=np.float32)
    c = lc.load(nam_lib, lc.container_doc()).batch(n2, 64)
    c.process_stream(z, 64)
    assert _blob_width(c.get_stream_state(40)) == 3
    # a plain Linear batch's blob (same ring length) is refused and changes nothing
    plain = lc.load(nam_lib, lc.sub_doc(1025)).batch(2, 64)
    plain.process(z[:2, :64])
    foreign = plain.get_stream_state(0)
    plain.close()
    assert len(foreign) == len(blob)
    before = c.get_stream_state(40)
    with pytest.raises(nam_lib.NamHipError, match="model_fp") as e:
        c.set_stream_state(40, foreign)
    assert e.value.code == nam_lib.ERR_INVALID_ARGUMENT
    assert c.get_stream_state(40) == before
    c.set_stream_state(40, blob)
    assert _blob_width(c.get_stream_state(40)) == 1
    # from the next call on the two streams produce the same bits; every other stream of the source is untouched by the get
    rest = np.ascontiguousarray(stream_bank(n2, N - at, seed=13), dtype=np.float32)
    rest[40] = x[5, at:]
    tail_a = np.concatenate([a.process(blk) for blk in blocks[k:]], axis=-1)[:, 0, :]
    tail_c = _run(c, rest, LENGTHS[k:])
    a.close()
    c.close()
    assert _same(tail_a, got[:, at:]) == ""
    assert np.array_equal(bits(tail_c[40]), bits(tail_a[5]))


# ---- 6. the rest of the surface ----
def test_surface(nam_lib, case):
    nam = nam_lib
    x, _, got = case
    b = _container_batch(nam)
    assert b.set_persistent(True) is False
    b.set_kernel(nam.KERNEL_AUTO)
    for kernel in (nam.KERNEL_GENERIC, nam.KERNEL_A1_MFMA, nam.KERNEL_WN_REG):
        with pytest.raises(nam.NamHipError, match="nam_linear_pairs_kernel only") as e:
            b.set_kernel(kernel)
        assert e.value.code == nam.ERR_UNSUPPORTED
    assert b.get_kernel() == nam.KERNEL_AUTO and b.kernel_name() == KERNEL
    # tickets 8 deep at 64 frames equal the blocking calls bit for bit (persistent mode asked for and not eligible: launches as usual)
    blocks = lc.blocks_of(x, LENGTHS)[:31]
    outs, tickets = [], []
    for blk in blocks:
        tickets.append(b.submit(blk))
        if len(tickets) == 8:
            outs.append(b.wait(tickets.pop(0)))
    outs += [b.wait(t) for t in tickets]
    assert _same(np.concatenate(outs, axis=-1)[:, 0, :], got[:, :64 * 31]) == ""
    # process_f64 equals process_f32, cast
    b.Reset()
    y64 = b.process(x[:, :64].astype(np.float64))
    assert y64.dtype == np.float64 and np.array_equal(y64[:, 0, :], got[:, :64].astype(np.float64))
    b.close()


@pytest.mark.parametrize("n_streams", [1, 32, 33])
def test_same_bits_at_any_stream_count(nam_lib, case, n_streams):
    x, _, got = case
    b = _container_batch(nam_lib, n_streams)
    y = _run(b, np.ascontiguousarray(x[:n_streams]))
    b.close()
    assert _same(y, got[:n_streams]) == ""


# ---- 7. the C++ adapter ----
def test_cpp_adapter_linear_container_check(nam_lib):
    """cpp/tools/linear_container_check: nam::get_dsp casts to nam::SlimmableModel, three nam::DSP instances at three sizes against a
    direct convolution on the host, the same through one BatchDSP with a size per stream."""
    tool = os.path.join(ROOT, "cpp", "tools", "linear_container_check")
    assert os.access(tool, os.X_OK), "build() makes cpp/tools/linear_container_check"
    r = subprocess.run([tool, lc.FIXTURE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout and "FAILED" not in r.stdout
