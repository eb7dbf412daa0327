"""Audio in for the stream pool, without a GPU: the four new C-ABI symbols agree with the header and the ctypes table;
rnnt_wave_stage_host -- the staging and carry roll of rnnt_pool_wave for one slot, through the index helper the two kernels use --
chained over a packet split reproduces, as exact float copies, the frames of the reflect-padded whole waveform; wave_plan turns any
number of packets into one call and the chunks that leave the FIFOs; StreamPool.feed_wave over a recording fake engine."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.online_rnnt_model import StreamPool, wave_frames, wave_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_pool_wave", "rnnt_stream_wave_reset", "rnnt_stream_get_wave_state", "rnnt_wave_stage_host")
HOP = 512
LENGTHS = (0, 100, 512, 513, 1023, 1024, 1536, 2560, 8000, 12345)
SPLITS = ("all_at_once", "packets_320", "random_0_700", "empty_final")


def test_new_symbols_in_header_signatures_and_library():
    src = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = rlib.load()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rnnt_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in rlib.SIGNATURES, f"{name} is missing from lib.SIGNATURES"
        res, args = rlib.SIGNATURES[name]
        assert res is rlib.c_i32 and len(args) == n_args, f"{name}: header has {n_args} arguments, SIGNATURES {len(args)}"
        assert hasattr(lib, name), f"librnnt_hip.so does not export {name}"
    assert lib.rnnt_abi_version() == 3
    assert ctypes.sizeof(rlib.RnntConfig) == 10 * 4


def test_null_context_is_an_argument_error():
    lib = rlib.load()
    one = np.zeros(1, np.int32)
    p = one.ctypes.data_as(ctypes.c_void_p)
    assert lib.rnnt_pool_wave(None, 1, p, p, 1, p, p, 16000, 1024, p, 1, p, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_wave_reset(None, 0, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_wave_state(None, 0, None, None, None, None, None, None, None, 0, None) == rlib.ERR_ARG


# ---- rnnt_wave_stage_host ---------------------------------------------------------------------------------------------------------
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


def chain(x, split, n_fft, rng):
    """the utterance through rnnt_wave_stage_host packet by packet -> (frames' sample windows, frame counts, longest carry)"""
    carry, at, windows, counts, longest = np.zeros(0, np.float32), 0, [], [], 0
    for k, final in packets(x.size, split, rng):
        staged, first, nf, carry = rlib.wave_stage_host(carry, at, x[at:at + k], final, n_fft)
        assert first == len(windows), "frames come out in order, nothing twice"
        assert staged.size >= ((nf - 1) * HOP + n_fft if nf else 0)
        windows += [staged[r * HOP:r * HOP + n_fft] for r in range(nf)]
        counts.append(nf)
        longest = max(longest, carry.size)
        at += k
    return windows, counts, longest


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n_fft", [1024, 256])
def test_stage_host_reproduces_the_reflect_padded_frames(n_fft, split):
    rng = np.random.default_rng(1000 + n_fft + SPLITS.index(split))
    for n in LENGTHS:
        x = rng.standard_normal(n).astype(np.float32)
        windows, counts, longest = chain(x, split, n_fft, rng)
        assert longest <= n_fft, f"N={n}: a carry of {longest} samples exceeds the stated bound n_fft = {n_fft}"
        if n <= n_fft // 2:
            assert sum(counts) == 0 and not windows, f"N={n}: no frame without reflect padding"
            continue
        assert sum(counts) == 1 + n // HOP, f"N={n}: {counts}"
        padded = np.pad(x, n_fft // 2, "reflect")
        want = np.stack([padded[f * HOP:f * HOP + n_fft] for f in range(1 + n // HOP)])
        got = np.stack(windows)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"N={n}: a staged frame is not an exact copy"


def test_stage_host_frames_before_the_end_are_those_that_fit():
    """before the final flag a push emits exactly the frames whose span has ended, and none until x[n_fft/2] exists"""
    x = np.arange(3000, dtype=np.float32)
    for n_fft in (1024, 256):
        carry, at = np.zeros(0, np.float32), 0
        for k in (n_fft // 2, 1, 511, 1, 700, 0, 1275 - n_fft // 2):
            _, first, nf, carry = rlib.wave_stage_host(carry, at, x[at:at + k], False, n_fft)
            at += k
            fit = [f for f in range(10) if f * HOP + n_fft // 2 <= at] if at >= n_fft // 2 + 1 else []
            assert first + nf == len(fit) == wave_frames(at, n_fft, False), (n_fft, at)


def test_stage_host_refusals():
    x = np.zeros(600, np.float32)
    with pytest.raises(rlib.RnntError) as e:
        rlib.wave_stage_host(np.zeros(3, np.float32), 600, x, False, 1024)      # 600 samples so far carry 600, not 3
    assert e.value.status == rlib.ERR_ARG
    with pytest.raises(rlib.RnntError) as e:
        rlib.wave_stage_host(np.zeros(0, np.float32), 0, x, False, 1000)        # n_fft outside rnnt_fbank's range
    assert e.value.status == rlib.ERR_SHAPE


# ---- wave_plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_one_call_whatever_the_slots_and_packets():
    queue = [(2, 320, False), (0, 320, False), (2, 320, False), (1, 0, False), (0, 9000, True), (2, 0, False)]
    call, chunks, samples, fifo = wave_plan(queue, {0: 0, 1: 5000, 2: 8000}, {2: 15}, 16, 1024)
    slots, counts, finals, frames = call
    assert slots == [2, 0, 1] and counts == [640, 9320, 0] and finals == [False, True, False]
    # slot 2: 8000 -> 8640 samples: frames 15..15 (f*512 + 512 <= N: 15 -> 16); slot 0: final with 9320 samples: 19 frames; slot 1: none
    assert frames == [1, 19, 0]
    assert samples == {0: 9320, 1: 5000, 2: 8640}
    assert chunks == [(2, 0, 16), (0, 0, 16), (0, 16, 3)], "full chunks in order, the remainder at final"
    assert fifo == {2: 0, 0: 0, 1: 0}
    assert wave_plan([], {0: 7}, {0: 3}, 16) == (None, [], {0: 7}, {0: 3})


def test_plan_frame_counts_are_the_librarys():
    rng = np.random.default_rng(3)
    for n_fft in (1024, 256):
        at, carry, fifo, samples = 0, np.zeros(0, np.float32), {}, {}
        x = rng.standard_normal(6000).astype(np.float32)
        for k in (0, 100, 413, 1, 511, 2000, 975, 2000):
            final = at + k == x.size
            _, _, nf, carry = rlib.wave_stage_host(carry, at, x[at:at + k], final, n_fft)
            call, _, samples, fifo = wave_plan([(5, k, final)], samples, fifo, 16, n_fft)
            assert call[3] == [nf]
            at += k
        assert at == x.size


# ---- StreamPool.feed_wave over a recording fake engine ------------------------------------------------------------------------------
class FakeEngine:
    """Records what StreamPool asks of the library.  pool_wave emits wave_frames' frames, each filled with its slot's running frame
    index; pool_chunk records the first column of every row's chunk, so the frames' order is visible; one token per call and slot."""

    def __init__(self):
        self.wave_calls, self.chunk_calls, self.opened = [], [], []
        self.samples, self.emitted, self.tokens = {}, {}, {}

    def reset(self, n, stream=None):
        self.n = n

    def stream_open(self, slot, stream=None):
        self.opened.append(slot)
        self.samples[slot], self.emitted[slot], self.tokens[slot] = 0, 0, []

    def pool_wave(self, slots, wave_ptr, n_samples, samples, final, out_ptr, cap_frames, sample_rate=16000, n_fft=1024, stream=None):
        assert wave_ptr != 0 and out_ptr != 0 and max(samples) <= n_samples
        self.wave_calls.append((list(slots), list(samples), [bool(f) for f in final], sample_rate, n_fft))
        frames = []
        out = np.ctypeslib.as_array(ctypes.cast(out_ptr, ctypes.POINTER(ctypes.c_float)), shape=(len(slots), cap_frames, 80))
        for i, (s, k, f) in enumerate(zip(slots, samples, final)):
            self.samples[s] += k
            nf = wave_frames(self.samples[s], n_fft, f) - self.emitted[s]
            assert nf <= cap_frames
            for r in range(nf):
                out[i, r, :] = self.emitted[s] + r
            self.emitted[s] += nf
            frames.append(nf)
        return np.array(frames, np.int32)

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        x = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(len(slots), length, 80))
        self.chunk_calls.append((list(slots), int(length), list(offsets), [x[i, :, 0].astype(int).tolist() for i in range(len(slots))]))
        for s in slots:
            self.tokens[s].append(100 * s + len(self.tokens[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def stream_tokens(self, slot, start=0, stream=None):
        return self.tokens[slot][start:]


def test_feed_wave_one_call_per_step_and_chunks_in_order():
    fake = FakeEngine()
    pool = StreamPool(None, 4, engine=fake, chunk_frames=16)
    a, b, c = pool.open(), pool.open(), pool.open()
    n_a, n_b = 20000, 9000                                    # 40 and 18 frames
    for k in range(0, 20000, 320):                             # 20 ms packets; slot b ends earlier, slot c gets one empty packet
        pool.feed_wave(a, torch.zeros(320), final=k + 320 >= n_a)
        if k < n_b:
            pool.feed_wave(b, torch.zeros(min(320, n_b - k)), final=k + 320 >= n_b)
        if k == 0:
            pool.feed_wave(c, torch.zeros(0))
        before = len(fake.wave_calls)
        pool.step()
        assert len(fake.wave_calls) == before + 1, "one rnnt_pool_wave call per step whatever the number of slots"
    assert fake.wave_calls[0][0] == [a, b, c] and fake.wave_calls[0][3:] == (16000, 1024)
    assert all(len(call[0]) == 1 for call in fake.wave_calls[n_b // 320 + 1:])
    per_slot = {a: [], b: []}
    for slots, length, offs, firsts in fake.chunk_calls:
        for s, row in zip(slots, firsts):
            per_slot[s].append(row)
    assert per_slot[a] == [list(range(0, 16)), list(range(16, 32)), list(range(32, 40))], "chunks in order, the remainder at final"
    assert per_slot[b] == [list(range(0, 16))], "the 2-frame remainder is under 7 frames: skipped as feed() skips it"
    assert pool.close(a) == [0, 1, 2] and pool.close(b) == [100]
    with pytest.raises(rlib.RnntError):
        pool.feed_wave(a, torch.zeros(320))                    # closed


def test_close_flushes_a_wave_slot_that_was_not_finalised():
    fake = FakeEngine()
    pool = StreamPool(None, 2, engine=fake, chunk_frames=16, n_fft=256, sample_rate=8000)
    s, other = pool.open(), pool.open()
    pool.feed_wave(s, torch.zeros(5000))                       # 10 frames fit (f*512 + 128 <= 5000), none is a full chunk
    pool.feed_wave(other, torch.zeros(700))
    assert pool.step() == {} and fake.chunk_calls == []
    n = len(fake.wave_calls)
    assert pool.close(s) == [0]
    assert fake.wave_calls[n:] == [([s], [0], [True], 8000, 256)], "close() pushes the final flag with no samples"
    assert fake.chunk_calls == [([s], 10, [0], [list(range(10))])]
    assert pool.open() == s                                   # the slot is free again and starts from nothing
    pool.feed_wave(s, torch.zeros(100), final=True)
    with pytest.raises(rlib.RnntError):
        pool.feed_wave(s, torch.zeros(100))                    # after the final packet
    pool.step()
    assert fake.wave_calls[-1] == ([s], [100], [True], 8000, 256) and pool.close(s) == []


def test_feed_and_feed_wave_do_not_mix():
    pool = StreamPool(None, 2, engine=FakeEngine())
    w, f = pool.open(), pool.open()
    pool.feed_wave(w, torch.zeros(320))
    with pytest.raises(rlib.RnntError):
        pool.feed(w, torch.zeros(16, 80))
    assert pool.feed(f, torch.zeros(16, 80))
    with pytest.raises(rlib.RnntError):
        pool.feed_wave(f, torch.zeros(320))
    pool.close(w), pool.close(f)
    assert pool.open() == w and pool.feed(w, torch.zeros(16, 80)), "a re-opened slot is fed either way again"
