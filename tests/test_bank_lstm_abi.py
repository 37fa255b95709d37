"""Model banks of the LSTM family on the host side (include/nam_hip.h: nam_hip_bank_create is host-only): LSTMs of one shape that
nam_lstm_row_kernel (hidden <= 4) or nam_lstm_wide_kernel (5 .. 32 units) takes share a batch; what is refused and how the
refusal names its member and the field; that such a bank owns what it needs. The WaveNet families' sides are
tests/test_bank_abi.py and tests/test_bank_a2_abi.py."""
import pytest

from bank_harness import fixture, refused, survives_its_models
from bank_models import lstm_weights, write_lstm
from conftest import model_path


def _seeded(nam, tmp_path, seed, fast_tanh=True, **kw):
    tag = "_".join(f"{k}{v}" for k, v in sorted(kw.items()))
    p = str(tmp_path / f"lstm_bank_{seed}_{tag}.nam")
    write_lstm(p, seed, **kw)
    return nam.get_dsp(p, fast_tanh=fast_tanh)


def test_generator_seeds_differ_in_weights_and_initial_state():
    a, at = lstm_weights(501, 1, 1, 3, 1)
    b, _ = lstm_weights(502, 1, 1, 3, 1)
    c, _ = lstm_weights(501, 1, 1, 3, 1, state_seed=7)
    (lo, hi), = at
    assert hi - lo == 6 and len(a) == 70  # (lstm.nam's count: 4 * 3 * 4 + 12 + 3 + 3 + 3 + 1)
    assert a[lo:hi] != b[lo:hi] and a[:lo] != b[:lo]
    assert a[:lo] == c[:lo] and a[hi:] == c[hi:] and a[lo:hi] != c[lo:hi]  # state_seed: h0 / c0 alone


@pytest.mark.parametrize("fast_tanh", [True, False])
def test_lstm_bank_accepts_the_fixtures_and_seeded_members(nam_lib, tmp_path, fast_tanh):
    """The gate-row kernel's shape (lstm.nam: 1 x 3) and the wide kernel's (synth_lstm_h18x2: 2 x 18), with fast_tanh on and off
    (both kernels are instantiated on it). Before the LSTM family existed member 0 was refused."""
    nam = nam_lib
    row = [fixture(nam, "lstm", fast_tanh), _seeded(nam, tmp_path, 511, fast_tanh), _seeded(nam, tmp_path, 512, fast_tanh)]
    assert len(nam.ModelBank(row)) == 3
    assert len(nam.ModelBank(row[::-1])) == 3
    assert len(nam.ModelBank(row[:1])) == 1  # a bank of one model is legal
    wide = [fixture(nam, "synth_lstm_h18x2", fast_tanh), _seeded(nam, tmp_path, 513, fast_tanh, num_layers=2, hidden=18)]
    assert len(nam.ModelBank(wide)) == 2
    assert len(nam.ModelBank(wide[1:])) == 1


def test_lstm_bank_refusals_name_the_member_and_the_field(nam_lib, tmp_path):
    nam = nam_lib
    lstm = fixture(nam, "lstm")
    seeded = _seeded(nam, tmp_path, 520)
    assert "hidden" in refused(nam, [lstm, seeded, _seeded(nam, tmp_path, 521, hidden=4)], 2)
    assert "n_layers" in refused(nam, [lstm, _seeded(nam, tmp_path, 522, num_layers=2)], 1)
    assert "hidden" in refused(nam, [fixture(nam, "synth_lstm_h18x2"), _seeded(nam, tmp_path, 523, num_layers=2, hidden=20)], 1)  # (both pad to 20)
    assert "fast_tanh" in refused(nam, [lstm, _seeded(nam, tmp_path, 524, fast_tanh=False)], 1)
    assert "fast_tanh" in refused(nam, [fixture(nam, "lstm", False), seeded], 1)
    # half a second of prewarm at the FILE's sample rate
    assert "prewarm_samples" in refused(nam, [lstm, _seeded(nam, tmp_path, 525, sample_rate=44100)], 1)
    # 40 hidden units: the matrix-core / lanes kernels, which know no banks
    msg = refused(nam, [lstm, _seeded(nam, tmp_path, 526, hidden=40)], 1)
    assert "nam_lstm_mfma_kernel" in msg and "hidden 40" in msg, msg
    msg = refused(nam, [_seeded(nam, tmp_path, 526, hidden=40)], 0)
    assert "nam_lstm_mfma_kernel" in msg, msg
    # one family per bank, in either order: the LATER member is the one that differs
    std = fixture(nam, "wavenet_a1_standard")
    assert "family" in refused(nam, [lstm, std], 1)
    assert "family" in refused(nam, [std, lstm], 1)
    assert "family" in refused(nam, [fixture(nam, "A2"), lstm], 1)
    assert "family" in refused(nam, [lstm, seeded, fixture(nam, "A2")], 2)


def test_lstm_bank_survives_its_models(nam_lib, tmp_path):
    """The bank copies what it needs (blobs AND initial states): the member models are freed (their handles through
    nam_hip_model_free) before the bank is asked anything."""
    seeded = str(tmp_path / "lstm_survivor.nam")
    write_lstm(seeded, 530)
    survives_its_models(nam_lib, [model_path("lstm"), seeded], lambda: [_seeded(nam_lib, tmp_path, 531 + i) for i in range(3)])


def test_version_says_lstm_banks(nam_lib):
    v = nam_lib.load_library().nam_hip_version().decode()
    assert tuple(int(t) for t in v.split()[1].split(".")) >= (0, 2, 4), v
