"""Memory of the per-slot transducer prefix search (rnnt_pool_prefix_frames): its buffers are allocated on the first use, counted by
rnnt_live_device_bytes, kept by later calls and resets, and returned by rnnt_destroy.  Needs a real MI355X: `pytest -m gpu`."""
import gc

import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.lib import RnntEngine

pytestmark = pytest.mark.gpu


def test_first_use_allocates_and_destroy_returns(np_state_dict):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    s = torch.cuda.current_stream().cuda_stream
    gc.collect()
    base = rlib.live_device_bytes()
    eng = RnntEngine(max_streams=2, max_chunk_frames=32, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=0)
    eng.load_state_dict(np_state_dict(0))
    eng.reset(2, s)
    eng.stream_open(0, s)
    assert eng.stream_prefix_size(0) == (1, 0, 1)                          # host only
    before = rlib.live_device_bytes()
    assert before > base
    enc = torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(3)).cuda()
    eng.pool_prefix_frames([0, 1], enc.data_ptr(), 3, 4, 0.3, 0.7, s)
    first = rlib.live_device_bytes()
    rows, lcap = 2 * 16, 64 + 1
    assert first - before >= 2 * rows * (1024 * 4 + lcap * 4 + 4 + 8 + 8)  # the two buffer sets at least
    eng.pool_prefix_frames([1, 0], enc.data_ptr(), 3, 4, 0.3, 0.7, s)
    hyps = eng.stream_prefix(0, True, s)[0]
    assert len(hyps) == 4 and rlib.live_device_bytes() >= first
    read = rlib.live_device_bytes()
    eng.stream_prefix_reset(-1, s)
    eng.reset(2, s)
    eng.pool_prefix_frames([0], enc.data_ptr(), 3, 4, 0.0, 1.0, s)
    eng.stream_prefix(0, True, s)
    torch.cuda.synchronize()
    assert rlib.live_device_bytes() == read                                # later calls, reads and resets reuse what is there
    eng.close()
    gc.collect()
    assert rlib.live_device_bytes() == base
