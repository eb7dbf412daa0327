"""What test_fbank_cpu.py and test_fbank.py share: seeded float32 signals at the level edges of the feature front-end, a plain NumPy
float32 emulation of the device's arithmetic, and the bars a front-end output is held to against the float64 oracle.

Absolute level does not decide how well float32 reproduces a mel bin: depth below the frame's own largest bin does (cancellation in
the DFT sums is relative to the frame's energy).  So the oracle's bins fall into three classes (classify) and each has its own bar
(check).  The deep class's bar comes from the emulation's error against the oracle on the cases below, never from a device."""
import functools

import numpy as np

from oracle import fbank_oracle as F

HOP, N_MELS, FLOOR = 512, 80, -100.0
GRID_NFFT = (64, 192, 256, 512, 1024, 1088, 2048, 2112, 4096)
RATES = (8000, 16000, 22051, 44100, 48000)          # 22051: odd, so sample_rate // 2 matters
NEAR_DEPTH = 60.0                                     # dB below the frame's largest bin
NEAR_BAR = 2e-3                                       # dB: the project's bar since the front-end exists
EMPTY_BAR = 1e-4                                      # dB around the floor: the accumulator is exactly 0, 10 log10f(1e-10f)
EPS_MEASURED = 2.6e-11                                # see check()
EPS_DEEP = 10.0 * EPS_MEASURED


# ---- signals ------------------------------------------------------------------------------------------------------------------------
def tone(n, rate, seed):
    """noise + 440 Hz tone (make_wave of test_pool_wave.py)"""
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)).astype(np.float32)


def quiet(n, rate, seed):
    return (1e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def loud(n, rate, seed):
    """far outside [-1, 1]"""
    return (30.0 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def zeros(n, rate, seed):
    return np.zeros(n, np.float32)


def dc(n, rate, seed):
    """a DC-offset microphone: every bin but the lowest lies 80 dB and more under the frame's peak"""
    return (0.9 + 1e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def step(n, rate, seed):
    """silence, then 0.9 from a sample on: 13 past a frame's centre, so inside that frame's window whatever n_fft is"""
    x = 1e-6 * np.random.default_rng(seed).standard_normal(n)
    x[n // 2 // HOP * HOP + 13:] += 0.9
    return x.astype(np.float32)


def impulse(n, rate, seed):
    x = np.zeros(n, np.float32)
    x[n // 2 + 3] = 1.0
    return x


def int16(n, rate, seed):
    """noise on the grid of a 16-bit recording"""
    return (np.round(0.1 * np.random.default_rng(seed).standard_normal(n) * 32768.0) / 32768.0).astype(np.float32)


SIGNALS = {"tone": tone, "quiet": quiet, "loud": loud, "zeros": zeros, "dc": dc, "step": step, "impulse": impulse, "int16": int16}
NO_DEEP = ("tone", "quiet", "loud", "int16")         # noise-like: no bin 60 dB under its frame's peak (asserted in test_fbank_cpu.py)
HAS_DEEP = ("dc", "step")


def make(name, n, rate, n_fft, seed):
    """The signal `name` of n samples.  A noise-like one (NO_DEEP) is drawn again, seed + 7919 k, until the float64 oracle has no
    bin deeper than NEAR_DEPTH under its frame's peak: frame 0 is symmetric about its centre under reflect padding, so each of its
    DFT bins has one degree of freedom instead of two and dips 60 dB with a probability near 1e-3, a few bins over the grid.  The
    condition is on the oracle alone; with it every non-empty bin of these signals is held to the dB bar."""
    if name not in NO_DEEP:
        return SIGNALS[name](n, rate, seed)
    fb = F.mel_filterbank(rate, n_fft)
    for k in range(32):
        x = SIGNALS[name](n, rate, seed + 7919 * k)
        if not classify(F.extract_audio_features(x, rate, n_fft=n_fft), fb)[2].any():
            return x
    raise AssertionError(f"{name} at rate {rate}, n_fft {n_fft}: 32 draws, each with a deep bin")


def cpu_len(n_fft):
    """samples of a CPU case: 6 frames and more, not a multiple of the hop"""
    return 2560 + n_fft + 77


def cases():
    """(name, rate, n_fft, wave) over the whole grid, n_fft outermost (the emulation's DFT matrix is built once per n_fft)"""
    for n_fft in GRID_NFFT:
        for ri, rate in enumerate(RATES):
            for si, name in enumerate(SIGNALS):
                yield name, rate, n_fft, make(name, cpu_len(n_fft), rate, n_fft, 1000 * ri + 10 * si + n_fft)


# ---- float32 emulation of the device's arithmetic -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def dft_rows(n_fft):
    """[2 * (n_fft/2 + 1), n_fft] float32: rows (w cos, -w sin) interleaved, built in float64 with an exact phase reduction"""
    n = np.arange(n_fft)
    win = 0.54 - 0.46 * np.cos(2.0 * np.pi * n / n_fft)
    ph = 2.0 * np.pi * ((np.arange(n_fft // 2 + 1)[:, None] * n[None, :]) % n_fft) / n_fft
    rows = np.empty((2 * (n_fft // 2 + 1), n_fft), np.float32)
    rows[0::2] = win * np.cos(ph)
    rows[1::2] = -win * np.sin(ph)
    return rows


def frames_of(wave, n_fft):
    x = np.asarray(wave, np.float32)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    return xp[np.arange(n_fft)[None, :] + HOP * np.arange(1 + x.shape[0] // HOP)[:, None]]


def emulate(wave, rate, n_fft):
    """the two matrix products of rnnt_fbank in float32 -> [1 + n // 512, 80] float32 (dB)"""
    spec = frames_of(wave, n_fft) @ dft_rows(n_fft).T
    assert spec.dtype == np.float32
    power = spec[:, 0::2] * spec[:, 0::2] + spec[:, 1::2] * spec[:, 1::2]
    mel = power @ F.mel_filterbank(rate, n_fft).astype(np.float32)
    assert mel.dtype == np.float32
    return np.float32(10.0) * np.log10(np.maximum(mel, np.float32(1e-10)))


# ---- classes and bars -----------------------------------------------------------------------------------------------------------------
def classify(want, fb):
    """want [T, 80] (float64 oracle, dB), fb = F.mel_filterbank(rate, n_fft) -> boolean masks (empty, near, deep) of want's shape:
    empty -- the filter's column of fb is all zero (small n_fft: its triangle falls between two DFT bins);
    near  -- within NEAR_DEPTH dB of the frame's largest bin; deep -- the rest."""
    empty = np.broadcast_to((fb.sum(0) == 0.0)[None, :], want.shape)
    peak = want.max(axis=1, keepdims=True)
    near = ~empty & (want >= peak - NEAR_DEPTH)
    return empty, near, ~empty & ~near


def errors(got, want, fb):
    """the three figures check() bounds, as a dict (max over the class, 0.0 for a class without bins), with the class sizes"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    empty, near, deep = classify(want, fb)
    peak = np.broadcast_to(want.max(axis=1, keepdims=True), want.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        rel = np.abs(10.0 ** (got / 10.0) - 10.0 ** (want / 10.0)) / 10.0 ** (peak / 10.0)

    def worst(v, m):
        return float(np.max(v[m])) if m.any() else 0.0
    return {"near": worst(np.abs(got - want), near), "empty": worst(np.abs(got - FLOOR), empty), "deep": worst(rel, deep),
            "n_near": int(near.sum()), "n_empty": int(empty.sum()), "n_deep": int(deep.sum())}


def check(got, want, fb, what=""):
    """The bars of a front-end output against the float64 oracle; returns errors(got, want, fb).

    near:  |got - want| < NEAR_BAR = 2e-3 dB.  The float32 emulation's worst over cases() is 2.2e-4 dB on every signal but the step, and
           1.2e-3 dB in the frame the step falls into (n_fft 4096 at 44.1 kHz, a bin 50 dB under the peak; 6.5e-4 dB at n_fft 2048).
    empty: |got + 100| < EMPTY_BAR = 1e-4 dB.
    deep:  |10^(got/10) - 10^(want/10)| <= EPS_DEEP * 10^(peak/10), peak the frame's largest oracle bin: an error of the float32
           sums, which is relative to the frame's energy and not to the bin's own.  The emulation's worst over cases() (360 cases,
           measured on a CPU against the oracle) is EPS_MEASURED = 2.6e-11 (2.55e-11, the DC case); EPS_DEEP is ten times that, because the kernels'
           split-K summation order is not NumPy's.  Neither figure comes from a device."""
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    e = errors(got, want, fb)
    assert e["near"] < NEAR_BAR, f"{what}: near class off by {e['near']:.3g} dB"
    assert e["empty"] < EMPTY_BAR, f"{what}: empty filters off the floor by {e['empty']:.3g} dB"
    assert e["deep"] <= EPS_DEEP, f"{what}: deep class off by {e['deep']:.3g} of the frame's peak power (bar {EPS_DEEP:.3g})"
    return e
