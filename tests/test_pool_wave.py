"""Audio in for the stream pool on the device (rnnt_pool_wave, rnnt_stream_wave_reset, rnnt_stream_get_wave_state;
StreamPool.feed_wave).

The contract under test: per slot, the frames emitted since its reset are the rows of rnnt_fbank over the slot's whole waveform,
bit for bit, whatever the packet split and whatever the neighbours do.  Both run the same two GEMMs (gemm16 below 1024 rows: 16-row
tiles, fixed split-K order) on the same cached matrices, so frames are compared as bytes; the only tolerance here is the bar of
test_fbank_frontend_against_oracle against the float64 restatement.  Needs a real MI355X.  Nothing here provokes a device fault:
every refusal is a host-side argument check."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.features import extract_audio_features
from ctc_vr_amd.lib import ERR_ARG, ERR_SHAPE, ERR_STATE, RnntEngine, RnntError
from ctc_vr_amd.online_rnnt_model import StreamPool

pytestmark = pytest.mark.gpu

RATE, NFFT, HOP = 16000, 1024, 512
LENGTHS = (513, 1024, 2560, 8000, 12345)
SPLITS = ("all_at_once", "packets_320", "random_0_700", "empty_final")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def eng():
    """a 4-slot context without weights"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    e = RnntEngine(max_streams=4, max_chunk_frames=16, max_cache_frames=64, max_enc_frames=16, vocab_size=16, blank_id=0, max_beam=0)
    yield e
    e.close()


def make_wave(n, seed, rate=RATE, silence=False):
    rng = np.random.default_rng(seed)
    w = 0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)
    if silence:
        w[n // 3:n // 3 + 2000] = 0.0                          # a stretch of digital silence: the -100 dB floor
    return w.astype(np.float32)


def packets(n, split, rng):
    """[(samples, final)] of an utterance of n samples under a split"""
    if split == "all_at_once":
        return [(n, True)]
    if split == "empty_final":
        return [(n, False), (0, True)]
    if split == "packets_320":
        sizes = [min(320, n - a) for a in range(0, n, 320)] or [0]
        return [(k, i == len(sizes) - 1) for i, k in enumerate(sizes)]
    out, left = [], n
    while left > 0:
        k = min(int(rng.integers(0, 701)), left)
        out.append((k, False))
        left -= k
    out.insert(len(out) // 2, (0, False))                      # a zero-sample packet whatever the draw
    return out + [(0, True)]


def push(eng, rows, rate=RATE, n_fft=NFFT, cap=None):
    """one rnnt_pool_wave call: rows = [(slot, samples float32 array, final)] -> the new frames of every row, [frames, 80] arrays"""
    n_max = max(max(len(x) for _, x, _ in rows), 1)
    host = np.zeros((len(rows), n_max), np.float32)
    for i, (_, x, _) in enumerate(rows):
        host[i, :len(x)] = x
    wave = torch.from_numpy(host).cuda()
    cap = n_max // HOP + 3 if cap is None else cap
    out = torch.full((len(rows), cap, 80), float("nan"), device="cuda")
    frames = eng.pool_wave([s for s, _, _ in rows], wave.data_ptr(), n_max, [len(x) for _, x, _ in rows], [f for _, _, f in rows], out.data_ptr(),
                           cap, rate, n_fft, _stream())
    got = out.cpu().numpy()                                    # synchronises: the call itself does not
    return [got[i, :frames[i]].copy() for i in range(len(rows))]


def run_alone(eng, x, split, seed=0, slot=0, rate=RATE, n_fft=NFFT):
    """an utterance through one slot under a split -> its concatenated frames"""
    eng.stream_wave_reset(slot, _stream())
    rng, at, parts = np.random.default_rng(seed), 0, []
    for k, final in packets(len(x), split, rng):
        parts += push(eng, [(slot, x[at:at + k], final)], rate, n_fft)
        at += k
    return np.concatenate(parts, 0)


def fbank(eng, x, rate=RATE, n_fft=NFFT):
    return extract_audio_features(eng, torch.from_numpy(x), rate, n_fft=n_fft, stream=_stream()).cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def state_bytes(eng, slot):
    s = eng.wave_state(slot, _stream())
    return (s["samples"], s["frames"], s["sample_rate"], s["n_fft"], s["finished"], s["carry"].tobytes())


@pytest.fixture(scope="module")
def single(eng):
    """per length: the wave and the frames of its single final push, computed once"""
    cache = {}

    def get(n):
        if n not in cache:
            x = make_wave(n, 100 + n)
            cache[n] = (x, run_alone(eng, x, "all_at_once"))
            cache[n][1].setflags(write=False)
        return cache[n]
    return get


@pytest.mark.parametrize("split", SPLITS[1:])
@pytest.mark.parametrize("n", LENGTHS)
def test_split_invariance(n, split, eng, single):
    x, want = single(n)
    assert want.shape == (1 + n // HOP, 80) and np.isfinite(want).all()
    got = run_alone(eng, x, split, seed=n, slot=1 + LENGTHS.index(n) % 3)
    assert same_bits(got, want), f"N={n} {split}: frames differ from the single final push"


@pytest.mark.parametrize("n", LENGTHS)
def test_frames_are_rnnt_fbank_bitwise(n, eng, single):
    """under 1024 rows rnnt_fbank takes gemm16 too, and the pool always does under its row cap: same kernel, same tiles, same bits"""
    x, got = single(n)
    want = fbank(eng, x)
    assert same_bits(got, want), f"N={n}: max |diff| {np.max(np.abs(got - want))} dB against rnnt_fbank"


def test_against_float64_restatement(eng):
    """the bar of test_fbank_frontend_against_oracle: 2e-3 dB on bins above -60 dB, 0.05 dB below"""
    from oracle import fbank_oracle as F
    x = make_wave(12345, 7, silence=True)
    got = run_alone(eng, x, "packets_320")
    want = F.extract_audio_features(x, RATE)
    assert got.shape == want.shape
    hi = want > -60.0
    assert (~hi).any() and hi.any(), "the wave has both loud bins and the silence floor"
    assert np.max(np.abs(got[hi] - want[hi])) < 2e-3
    assert np.max(np.abs(got[~hi] - want[~hi])) < 0.05 or np.all(got[~hi] < -59.9)


def test_neighbours_do_not_matter(eng):
    """three slots at different phases with ragged packet sizes in shared calls, one of them finishing mid-way and re-opened for a second
    utterance: every utterance's frames are those of its alone run, and the idle fourth slot's state never changes"""
    eng.stream_wave_reset(-1, _stream())
    utt = {"a": make_wave(8000, 21), "b": make_wave(5000, 22), "c": make_wave(12345, 23), "d": make_wave(3000, 24)}
    push(eng, [(3, make_wave(700, 25), False)])                # the bystander holds a carry of its own
    idle = state_bytes(eng, 3)
    assert idle[0] == 700 and len(idle[5]) == 700 * 4
    plan = {"a": (0, 0, 320), "c": (2, 1, 777), "b": (1, 2, 500), "d": (1, None, 411)}      # slot, first step, packet size
    at, got, start = {k: 0 for k in utt}, {k: [] for k in utt}, {k: v[1] for k, v in plan.items()}
    step = 0
    while any(at[k] < len(utt[k]) for k in utt):
        rows, names = [], []
        for k in ("c", "a", "b", "d"):                         # row order is not slot order
            slot, _, size = plan[k]
            if start[k] is None or step < start[k] or at[k] >= len(utt[k]):
                continue
            x = utt[k][at[k]:at[k] + size]
            at[k] += len(x)
            rows.append((slot, x, at[k] == len(utt[k])))
            names.append(k)
        for k, f in zip(names, push(eng, rows)):
            got[k].append(f)
        if at["b"] == len(utt["b"]) and start["d"] is None:   # b ended in this call: its slot is re-opened for d
            assert state_bytes(eng, 1)[4] is True
            eng.stream_wave_reset(1, _stream())
            start["d"] = step + 1
        assert state_bytes(eng, 3) == idle, f"step {step}: the idle slot's state changed"
        step += 1
    eng.stream_wave_reset(-1, _stream())
    for k, x in utt.items():
        want = run_alone(eng, x, "all_at_once")
        assert same_bits(np.concatenate(got[k], 0), want), f"utterance {k}: frames differ from its alone run"


@pytest.mark.parametrize("n", [2048, 2049])
def test_n_fft_below_hop(n, eng):
    """n_fft = 256 at 8 kHz: gaps between frames; N a multiple of 512 puts the last frame's centre on N"""
    from oracle import fbank_oracle as F
    x = make_wave(n, 31 + n, rate=8000)
    want = fbank(eng, x, 8000, 256)
    assert want.shape == (5, 80)
    for split in SPLITS:
        got = run_alone(eng, x, split, seed=n, rate=8000, n_fft=256)
        assert same_bits(got, want), f"N={n} {split}"
    ref = F.extract_audio_features(x, 8000, n_fft=256)
    hi = ref > -60.0
    assert np.max(np.abs(want[hi] - ref[hi])) < 2e-3


def test_short_utterance_is_no_error(eng):
    eng.stream_wave_reset(0, _stream())
    (frames,) = push(eng, [(0, make_wave(400, 41), True)])
    assert frames.shape == (0, 80)
    s = eng.wave_state(0, _stream())
    assert s["samples"] == 400 and s["frames"] == 0 and s["finished"]
    # a row with no samples and no final flag is a no-op, also on a fresh slot: nothing is fixed
    eng.stream_wave_reset(1, _stream())
    before = state_bytes(eng, 1)
    assert push(eng, [(1, np.zeros(0, np.float32), False)], 8000, 256)[0].shape == (0, 80)
    assert state_bytes(eng, 1) == before and before[:5] == (0, 0, 0, 0, False)
    # the final flag with no new samples flushes the tail
    eng.stream_wave_reset(2, _stream())
    x = make_wave(1300, 42)
    head = push(eng, [(2, x, False)])[0]
    tail = push(eng, [(2, np.zeros(0, np.float32), True)])[0]
    assert head.shape == (2, 80) and tail.shape == (1, 80)
    assert same_bits(np.concatenate([head, tail], 0), fbank(eng, x))


def test_refusals_change_nothing(eng):
    eng.stream_wave_reset(-1, _stream())
    push(eng, [(0, make_wave(700, 51), False), (3, make_wave(1500, 52), False)])      # in progress at (16000, 1024)
    push(eng, [(1, make_wave(900, 53), True)])                                          # finished; slot 2 stays fresh
    before = [state_bytes(eng, s) for s in range(4)]
    x = torch.zeros(2, 600, device="cuda")
    out = torch.zeros(2, 4, 80, device="cuda")

    def call(slots, samples, final=None, wave=x.data_ptr(), o=out.data_ptr(), cap=4, rate=RATE, n_fft=NFFT, n_samples=600):
        return lambda: eng.pool_wave(slots, wave, n_samples, samples, final or [False] * len(slots), o, cap, rate, n_fft, _stream())
    cases = [
        ("null wave", call([0], [600], wave=None), ERR_ARG),
        ("null out", call([0], [600], o=None), ERR_ARG),
        ("slot listed twice", call([0, 0], [10, 10]), ERR_ARG),
        ("slot out of range", call([4], [10]), ERR_ARG),
        ("negative slot", call([2, -1], [10, 10]), ERR_ARG),
        ("more samples than the row holds", call([2, 0], [10, 601]), ERR_ARG),
        ("negative sample count", call([2], [-1]), ERR_ARG),
        ("n_fft differs from the utterance in progress", call([2, 0], [600, 600], n_fft=512), ERR_ARG),
        ("sample_rate differs from the utterance in progress", call([3], [600], rate=8000), ERR_ARG),
        ("cap_frames below a row's frames", call([2, 3], [0, 600], cap=0), ERR_ARG),
        ("n_fft not a multiple of 64", call([2], [600], n_fft=1000), ERR_SHAPE),
        ("n_fft above the range", call([2], [600], n_fft=8192), ERR_SHAPE),
        ("sample_rate below the range", call([2], [600], rate=1), ERR_SHAPE),
        ("push to a finished slot", call([2, 1], [600, 600]), ERR_STATE),
        ("flush of a finished slot", call([1], [0], final=[True]), ERR_STATE),
    ]
    for what, fn, status in cases:
        with pytest.raises(RnntError) as e:
            fn()
        assert e.value.status == status, f"{what}: status {e.value.status}, expected {status}"
        assert [state_bytes(eng, s) for s in range(4)] == before, f"{what}: a refused call changed a slot's state"
    with pytest.raises(RnntError) as e:
        eng.stream_wave_reset(4, _stream())
    assert e.value.status == ERR_ARG
    after = push(eng, [(0, make_wave(600, 54), False), (2, make_wave(600, 55), False)])                     # and the slots go on as if never asked
    assert [f.shape for f in after] == [(1, 80), (1, 80)]      # slot 0: 1300 samples, frame 1; slot 2: 600 samples, frame 0


def test_launch_count_does_not_depend_on_n_active(eng):
    counts = []
    for slots in ([0], [0, 1, 2, 3]):
        eng.stream_wave_reset(-1, _stream())
        push(eng, [(s, make_wave(300, 60 + s), False) for s in slots])
        before = eng.counters()[0]
        frames = push(eng, [(s, make_wave(2000, 70 + s), False) for s in slots])
        assert all(f.shape == (4, 80) for f in frames)          # 2300 samples: frames 0..3
        counts.append(eng.counters()[0] - before)
    assert counts[0] == counts[1] > 0, f"launches per push: {counts}"


def test_end_to_end_tokens(np_state_dict):
    """two callers as 20 ms packets through feed_wave / step / close against the same pool fed, through feed, the chunks sliced from
    rnnt_fbank of the whole waves: tokens exact"""
    pool = StreamPool(np_state_dict(0), 2, vocab_size=T.VOCAB, blank_id=T.BLANK, max_chunk_frames=16, max_cache_frames=64, chunk_frames=16)
    waves = [make_wave(32000, 81), make_wave(20800, 82)]        # 2 s and 1.3 s: 63 and 41 frames
    slots = [pool.open(), pool.open()]
    for k in range(0, 32000, 320):
        for s, w in zip(slots, waves):
            if k < len(w):
                pool.feed_wave(s, torch.from_numpy(w[k:k + 320]), final=False)
        pool.step()
    got = [pool.close(s) for s in slots]                        # close() flushes the tails
    pool.reset()
    slots = [pool.open(), pool.open()]
    feats = [extract_audio_features(pool.engine, torch.from_numpy(w), RATE) for w in waves]
    assert [f.size(0) for f in feats] == [63, 41]
    for a in range(0, 63, 16):
        for s, f in zip(slots, feats):
            if a < f.size(0):
                pool.feed(s, f[a:a + 16].contiguous())
        pool.step()
    want = [pool.close(s) for s in slots]
    assert got == want
    pool.engine.close()
