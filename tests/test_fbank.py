"""The feature front-end on the device (rnnt_fbank; rnnt_pool_wave for the stream pool) over its documented range -- n_fft a multiple of
64 in [64, 4096], any sample_rate >= 2, any number of frames -- against the float64 oracle, with the bars of fbank_cases.check.

Below 1024 rows both GEMMs of a call run gemm16 (split-K over 4 waves, or 8 where K >= 1024 divides by 128); from 1024 rows on
rnnt_fbank takes gemm_ns (LDS tiles of 64 rows over implicit, overlapping frames), the pool never does.  The cases sit on either side
of that switch, at every padded K of the mel projection, at the sample counts where the reflections and the last frame move, and at
the level edges of fbank_cases.  Needs a real MI355X.  Nothing here provokes a device fault: every refusal is a host-side decision."""
import numpy as np
import pytest
import torch

import fbank_cases as C
import test_pool_wave as PW
from ctc_vr_amd.lib import ERR_ARG, ERR_SHAPE, RnntEngine, RnntError
from oracle import fbank_oracle as F

pytestmark = pytest.mark.gpu

HOP = C.HOP
GPU_NFFT = C.GRID_NFFT + (3072,)
GRID_FRAMES = ((5, 1), (17, 100), (33, 511), (60, 256), (9, 300))     # per rate of C.RATES: (frames, samples past the last hop)


@pytest.fixture(scope="module")
def eng():
    """a 4-slot context without weights"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = RnntEngine(max_streams=4, max_chunk_frames=16, max_cache_frames=64, max_enc_frames=16, vocab_size=16, blank_id=0, max_beam=0)
    yield e
    e.close()


def waves(B, n, rate, seed):
    return np.stack([C.tone(n, rate, seed + 17 * b) for b in range(B)])


def against_oracle(got, x, rate, n_fft, what):
    """every stream of got [B, T, 80] through check() -> the worst figures over the streams"""
    fb = F.mel_filterbank(rate, n_fft)
    assert got.shape == (x.shape[0], 1 + x.shape[1] // HOP, 80), (what, got.shape)
    worst = {"near": 0.0, "empty": 0.0, "deep": 0.0}
    for b in range(x.shape[0]):
        e = C.check(got[b], F.extract_audio_features(x[b], rate, n_fft=n_fft), fb, f"{what}, stream {b}")
        worst = {k: max(v, e[k]) for k, v in worst.items()}
    return worst


def show(what, worst):
    print(f"[fbank] {what}: near {worst['near']:.3g} dB, empty {worst['empty']:.3g} dB, deep {worst['deep']:.3g} of the peak power")


# ---- 1. n_fft x rate below 1024 rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", GPU_NFFT)
def test_grid_against_oracle(n_fft, eng):
    """gemm16 with both split-K widths and every padded K of the mel projection: 1088, 1600 and 2112 were refused"""
    worst = {"near": 0.0, "empty": 0.0, "deep": 0.0}
    for (frames, past), rate in zip(GRID_FRAMES, C.RATES):
        n = (frames - 1) * HOP + past
        assert n > n_fft // 2
        x = waves(3, n, rate, n_fft + rate)
        for rows in (x, x[1:2]):                                # B = 3 and B = 1
            e = against_oracle(PW.fbank(eng, rows, rate, n_fft), rows, rate, n_fft, f"n_fft {n_fft}, rate {rate}, B {len(rows)}, n {n}")
            worst = {k: max(v, e[k]) for k, v in worst.items()}
    show(f"grid n_fft {n_fft}", worst)


# ---- 2. sample counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", (256, 1024, 4096))
def test_sample_count_edges(n_fft, eng):
    k = n_fft // HOP + 2
    counts = {"minimum: both reflections inside frame 0": n_fft // 2 + 1, "below n_fft": n_fft - 1, "one before a hop": HOP * k - 1,
              "last frame centred on n": HOP * k, "one past a hop": HOP * k + 1}
    for what, n in counts.items():
        x = waves(2, n, 16000, n_fft + n)
        against_oracle(PW.fbank(eng, x, 16000, n_fft), x, 16000, n_fft, f"n_fft {n_fft}, n {n} ({what})")
    before = eng.counters()[0]
    with pytest.raises(RnntError) as e:
        PW.fbank(eng, waves(1, n_fft // 2, 16000, 1), 16000, n_fft)
    assert e.value.status == ERR_SHAPE and eng.counters()[0] == before, "n = n_fft/2 has no reflection: refused before any launch"


# ---- 3. levels ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n_fft", ((16000, 1024), (48000, 2048)))
def test_level_edges(rate, n_fft, eng):
    n = 8 * HOP + 300
    fb = F.mel_filterbank(rate, n_fft)
    for name in C.SIGNALS:
        x = C.make(name, n, rate, n_fft, 5 + n_fft)
        got = PW.fbank(eng, x, rate, n_fft)
        assert got.shape == (9, 80) and np.isfinite(got).all(), name
        e = C.check(got, F.extract_audio_features(x, rate, n_fft=n_fft), fb, f"{name}, n_fft {n_fft}")
        show(f"level {name} n_fft {n_fft}", e)
        if name == "zeros":
            assert np.all(got == got[0, 0]) and abs(float(got[0, 0]) - C.FLOOR) < C.EMPTY_BAR, "silence is the floor in every bin"
        if name in C.HAS_DEEP:
            assert e["n_deep"] > 0
        if name in C.NO_DEEP:
            assert e["n_deep"] == 0


# ---- 4. the 1024-row switch ---------------------------------------------------------------------------------------------------------------
SWITCH = ((1024, 31, 33), (1024, 32, 32), (1024, 1, 1025), (1024, 3, 343), (1024, 33, 32), (64, 33, 32), (2048, 33, 32), (4096, 1, 1025))


@pytest.mark.parametrize("n_fft,B,T", SWITCH)
def test_row_switch_against_oracle(n_fft, B, T, eng):
    """1023 rows (gemm16), then 1024, 1025, 1029 and 1056 (gemm_ns; with 33 streams of 32 frames every second 64-row tile straddles
    two streams' padded signals)"""
    n = (T - 1) * HOP + (0 if B == 1 else 13)                   # 524 288 samples in the largest one-stream call
    x = waves(B, n, 16000, n_fft + B)
    got = PW.fbank(eng, x, 16000, n_fft)
    assert PW.same_bits(PW.fbank(eng, x, 16000, n_fft), got), "two launches of one call differ"
    show(f"switch n_fft {n_fft} rows {B * T}", against_oracle(got, x, 16000, n_fft, f"n_fft {n_fft}, B {B}, T {T}"))


@pytest.mark.parametrize("n_fft", (1024, 2048))
def test_row_switch_same_wave_either_side(n_fft, eng):
    """31 streams of 33 frames alone (1023 rows) and with a 32nd (1056 rows): other kernel, other summation order, so no bit equality,
    but each side is within the near bar of the oracle, hence within twice that of the other"""
    x = waves(32, 32 * HOP, 16000, n_fft + 99)                  # 524 288 samples
    small, large = PW.fbank(eng, x[:31], 16000, n_fft), PW.fbank(eng, x, 16000, n_fft)
    fb = F.mel_filterbank(16000, n_fft)
    worst = 0.0
    for b in range(31):
        _, _, deep = C.classify(F.extract_audio_features(x[b], 16000, n_fft=n_fft), fb)
        held = ~deep                                            # near and empty bins: the ones with a bar in dB
        worst = max(worst, float(np.max(np.abs(small[b].astype(np.float64) - large[b])[held])))
    print(f"[fbank] across the switch, n_fft {n_fft}: {worst:.3g} dB")
    assert worst < 2 * C.NEAR_BAR


# ---- 5. independence below 1024 rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", (64, 1024, 2112, 4096))
def test_batch_row_is_the_single_call(n_fft, eng):
    x = waves(3, 7 * HOP + 77, 16000, n_fft + 3)
    got = PW.fbank(eng, x, 16000, n_fft)
    for b in range(3):
        assert PW.same_bits(PW.fbank(eng, x[b], 16000, n_fft), got[b]), f"n_fft {n_fft}: row {b} of the batch differs from its B = 1 call"


def test_matrix_cache_follows_rate_and_n_fft(eng):
    x = waves(1, 10 * HOP + 5, 16000, 8)[0]
    runs = [PW.fbank(eng, x, rate, n_fft) for rate, n_fft in ((16000, 1024), (8000, 1024), (16000, 4096), (16000, 64), (16000, 1024))]
    assert PW.same_bits(runs[0], runs[4]), "the matrices of (16000, 1024) came back different"
    assert not PW.same_bits(runs[0], runs[1]), "another sample rate at the same n_fft kept the mel matrix"
    fb = F.mel_filterbank(8000, 1024)
    C.check(runs[1], F.extract_audio_features(x, 8000, n_fft=1024), fb, "rate 8000 after rate 16000")


# ---- 6. the pool over the range -----------------------------------------------------------------------------------------------------------
def run_alone(eng, x, split, seed, slot, rate, n_fft):
    """test_pool_wave.run_alone with room for the frames a flush emits at a large n_fft (up to n_fft / 512 more than the packet holds)"""
    eng.stream_wave_reset(slot, PW._stream())
    rng, at, parts = np.random.default_rng(seed), 0, []
    for k, final in PW.packets(len(x), split, rng):
        parts += PW.push(eng, [(slot, x[at:at + k], final)], rate, n_fft, cap=(k + n_fft) // HOP + 3)
        at += k
    return np.concatenate(parts, 0)


@pytest.mark.parametrize("rate,n_fft", ((16000, 64), (48000, 2048), (44100, 4096)))
def test_pool_frames_over_the_range(rate, n_fft, eng):
    """n_fft 64: the hop is eight windows, samples between frames are dropped on arrival; 2048 and 4096: carries up to WAVE_CARRY_CAP"""
    fb = F.mel_filterbank(rate, n_fft)
    for li, n in enumerate((n_fft // 2 + 1, HOP * (n_fft // HOP + 4), HOP * (n_fft // HOP + 5) + 379)):
        x = C.tone(n, rate, n_fft + n)
        want = PW.fbank(eng, x, rate, n_fft)
        C.check(want, F.extract_audio_features(x, rate, n_fft=n_fft), fb, f"n_fft {n_fft}, n {n}")
        for si, split in enumerate(PW.SPLITS):
            got = run_alone(eng, x, split, seed=n, slot=(li + si) % 4, rate=rate, n_fft=n_fft)
            assert PW.same_bits(got, want), f"n_fft {n_fft}, n {n}, {split}: frames differ from rnnt_fbank"


@pytest.mark.parametrize("n_fft", (2048, 4096))
def test_pool_carry_reaches_its_cap(n_fft, eng):
    """a push that ends one sample short of a frame leaves n_fft samples behind: the whole of WAVE_CARRY_CAP at n_fft 4096"""
    x = C.tone(n_fft + 1023 + 700 + 2000, 16000, n_fft + 1)
    eng.stream_wave_reset(2, PW._stream())
    at, parts, longest = 0, [], 0
    for k, final in ((n_fft + 1023, False), (700, False), (2000, True)):
        parts += PW.push(eng, [(2, x[at:at + k], final)], 16000, n_fft, cap=(k + n_fft) // HOP + 3)
        at += k
        carry = eng.wave_state(2, PW._stream())["carry"]
        longest = max(longest, len(carry))
        if at == n_fft + 1023:
            assert len(carry) == n_fft and np.array_equal(carry, x[at - n_fft:at]), "the carry is the last n_fft samples"
    assert longest == n_fft
    assert PW.same_bits(np.concatenate(parts, 0), PW.fbank(eng, x, 16000, n_fft))


def test_pool_1024_rows_in_one_call():
    """64 slots, 16 frames each: 1024 rows in the call, where rnnt_fbank would change kernel; the pool must not (GemmCapScope)"""
    e = RnntEngine(max_streams=64, max_chunk_frames=16, max_cache_frames=64, max_enc_frames=16, vocab_size=16, blank_id=0, max_beam=0)
    try:
        n = 512 + 15 * HOP + 100                                # not final: frames 0..15 are complete
        x = waves(64, n, 16000, 640)
        alone = []
        for s in range(64):
            alone += PW.push(e, [(s, x[s], False)])
        e.stream_wave_reset(-1, PW._stream())
        together = PW.push(e, [(s, x[s], False) for s in range(64)])
        assert sum(len(f) for f in together) == 1024
        for s in range(64):
            assert together[s].shape == (16, 80) and PW.same_bits(together[s], alone[s]), f"slot {s}: frames depend on the neighbours"
        fb = F.mel_filterbank(16000, 1024)
        for s in (0, 31, 63):
            C.check(together[s], F.extract_audio_features(x[s], 16000)[:16], fb, f"slot {s}")
    finally:
        e.close()


# ---- 7. refusals decide first -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", (1088, 1216, 2048, 2112, 3072, 4096))
def test_pool_call_succeeds_or_refuses_before_its_first_launch(n_fft, eng):
    """these n_fft were refused inside the second or the fourth launch of the call"""
    eng.stream_wave_reset(-1, PW._stream())
    x = C.tone(n_fft + 600, 16000, n_fft)
    state, launches = PW.state_bytes(eng, 1), eng.counters()[0]
    try:
        (frames,) = PW.push(eng, [(1, x, False)], 16000, n_fft)
    except RnntError:
        assert eng.counters()[0] == launches, "a refused call had launched already"
        assert PW.state_bytes(eng, 1) == state, "a refused call changed the slot"
        raise AssertionError(f"n_fft {n_fft} is inside the documented range and was refused")
    assert frames.shape == ((len(x) - n_fft // 2) // HOP + 1, 80) and eng.counters()[0] > launches
    # an utterance in progress, a carry on the device: a call without room for its frames is refused, and nothing has run
    state, launches = PW.state_bytes(eng, 1), eng.counters()[0]
    assert state[0] == n_fft + 600 and len(state[5]) > 0
    with pytest.raises(RnntError) as e:
        PW.push(eng, [(1, x[:1500], False)], 16000, n_fft, cap=1)
    assert e.value.status == ERR_ARG
    assert eng.counters()[0] == launches and PW.state_bytes(eng, 1) == state
