"""The front-end oracle on the CPU: its spectrogram half pinned against torch.stft (torchaudio's Spectrogram is torch.stft with the
window it is given), its mel / dB half a restatement of torchaudio's documented formulas checked for consistency (see the oracle's
header), and the conditions on the inputs of fbank_cases.py that the device tests rely on, asserted on the oracle and on the float32
emulation alone."""
import numpy as np
import pytest
import torch

import fbank_cases as C
from oracle import fbank_oracle as F


def test_shapes_floor_and_tone_peak():
    rate, n = 16000, 16000
    t = np.arange(n) / rate
    fb = F.mel_filterbank(rate, 1024)
    assert fb.shape == (513, 80) and fb.min() >= 0.0 and (fb.sum(0) > 0).all()
    assert np.allclose(F.extract_audio_features(np.zeros(n), rate), -100.0)                  # clamp at 1e-10
    feats = F.extract_audio_features(np.sin(2 * np.pi * 1000.0 * t), rate)
    assert feats.shape == (1 + n // 512, 80)
    centre = np.argmax(fb[int(round(1000.0 / (rate / 2) * 512))])                             # mel bin that owns 1 kHz
    assert abs(int(np.argmax(feats[10])) - int(centre)) <= 1
    # a window-energy check on a full-scale tone: |X(f0)|^2 ~ (sum(win)/2)^2 within the owning triangle's weight
    win = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    assert abs(feats[10].max() - 10 * np.log10((win.sum() / 2) ** 2)) < 3.0


def test_linearity_in_db():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(8000)
    a, b = F.extract_audio_features(x, 16000), F.extract_audio_features(10.0 * x, 16000)
    assert np.allclose(b - a, 20.0, atol=1e-9)                                                 # power scales with amplitude^2


@pytest.mark.parametrize("n_fft", C.GRID_NFFT)
def test_oracle_spectrogram_is_torch_stft(n_fft):
    """float64 torch.stft with torchaudio's Spectrogram defaults (center, reflect, win_length = n_fft, onesided) and the periodic
    Hamming window, pushed through the oracle's mel matrix and dB: the oracle's own framing, window and rfft to 1e-9 dB"""
    worst = 0.0
    for ri, rate in enumerate(C.RATES):
        x = C.tone(C.cpu_len(n_fft) + 100 * ri, rate, n_fft + ri)
        spec = torch.stft(torch.from_numpy(x).double(), n_fft, hop_length=C.HOP, win_length=n_fft, window=torch.hamming_window(n_fft, dtype=torch.float64),
                          center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        power = (spec.real ** 2 + spec.imag ** 2).numpy().T                                    # [frames, n_fft/2 + 1]
        ref = 10.0 * np.log10(np.maximum(power @ F.mel_filterbank(rate, n_fft), 1e-10))
        want = F.extract_audio_features(x, rate, n_fft=n_fft)
        assert ref.shape == want.shape == (1 + len(x) // C.HOP, 80)
        worst = max(worst, float(np.max(np.abs(ref - want))))
    print(f"n_fft {n_fft}: oracle vs torch.stft {worst:.3g} dB")
    assert worst < 1e-9


@pytest.mark.parametrize("n_fft", C.GRID_NFFT)
def test_filterbank_properties(n_fft):
    for rate in C.RATES:
        fb = F.mel_filterbank(rate, n_fft)
        assert fb.shape == (n_fft // 2 + 1, 80) and fb.min() >= 0.0 and np.isfinite(fb).all()
        empty = fb.max(0) == 0.0
        for m in np.nonzero(~empty)[0]:                                                        # a triangle: up to one peak, then down
            col, top = fb[:, m], int(np.argmax(fb[:, m]))
            assert (np.diff(col[:top + 1]) >= 0.0).all() and (np.diff(col[top:]) <= 0.0).all(), (rate, n_fft, m)
        got = C.classify(np.zeros((2, 80)), fb)[0]
        assert np.array_equal(got[0], empty) and np.array_equal(got[1], empty), "classify's empty class is the all-zero filters"
        assert empty.sum() < 40, "most filters own a DFT bin"
    assert (F.mel_filterbank(16000, 64).max(0) == 0.0).sum() == 30                             # 37.5 % of the bins at n_fft 64, 16 kHz
    if n_fft >= 1024:
        assert not empty.any()


@pytest.fixture(scope="module")
def emulated():
    """per case of fbank_cases.cases(): (name, rate, n_fft, the float32 emulation's output, the oracle's, the mel filterbank), computed once"""
    out = []
    for name, rate, n_fft, x in C.cases():
        fb = F.mel_filterbank(rate, n_fft)
        want = F.extract_audio_features(x, rate, n_fft=n_fft)
        out.append((name, rate, n_fft, C.emulate(x, rate, n_fft), want, fb))
    return out


def test_input_conditions(emulated):
    """what the device tests take for granted about their inputs"""
    assert len(emulated) == len(C.GRID_NFFT) * len(C.RATES) * len(C.SIGNALS)
    n_deep = n_rest = 0
    for name, rate, n_fft, _, want, fb in emulated:
        empty, near, deep = C.classify(want, fb)
        assert (empty ^ near ^ deep).all() and not (empty & near).any() and not (near & deep).any()
        if name in C.NO_DEEP:
            assert not deep.any(), f"{name} at rate {rate}, n_fft {n_fft}: {int(deep.sum())} bins 60 dB under their frame's peak"
        if name in C.HAS_DEEP:
            assert deep.any(), f"{name} at rate {rate}, n_fft {n_fft}: the deep class is not exercised"
        if name == "zeros":
            assert (want == C.FLOOR).all()
        n_deep += int(deep.sum())
        n_rest += int(near.sum())
    share = n_deep / (n_deep + n_rest)
    print(f"deep share of the non-empty bins: {share:.3f}")
    assert 0.0 < share <= 0.25


def test_emulation_meets_the_bars(emulated):
    """the float32 emulation passes check() on every case, and its worst deep-class error is the figure EPS_DEEP is ten times of"""
    worst = {"near": 0.0, "empty": 0.0, "deep": 0.0}
    for name, rate, n_fft, got, want, fb in emulated:
        e = C.check(got, want, fb, f"{name} at rate {rate}, n_fft {n_fft}")
        worst = {k: max(v, e[k]) for k, v in worst.items()}
    print("float32 emulation, worst per class:", {k: f"{v:.3g}" for k, v in worst.items()})
    # EPS_MEASURED is this maximum as first measured (2.55e-11); another BLAS sums in another order, so a factor of two either way
    assert C.EPS_DEEP == 10.0 * C.EPS_MEASURED and 0.5 * C.EPS_MEASURED < worst["deep"] <= 2.0 * C.EPS_MEASURED
