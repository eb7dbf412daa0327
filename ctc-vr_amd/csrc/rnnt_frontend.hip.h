// Feature front-end helpers (rnnt_fbank, rnnt_pool_wave): reflect padding / per-slot staging and power spectrum around the two GEMMs.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
#pragma once

// ------------------------------------------------------------------------------------------------
// Feature front-end (data/dataloader.py:15-41, torchaudio MelSpectrogram(center=True, pad_mode="reflect") + AmplitudeToDB):
// reflect_pad makes the n_fft/2-padded signal, the windowed DFT is a GEMM over implicit frames (row stride = hop) against
// interleaved (w cos, -w sin) rows, power_spectrum squares and adds the pairs, the mel projection is a second GEMM with
// the dB conversion as its epilogue.
// ------------------------------------------------------------------------------------------------
__global__ void reflect_pad(const float* __restrict__ x, float* __restrict__ y, int B, int n, int pad, long long ystride) {
    const long long total = (long long)B * ystride;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(id / ystride);
        const int i = (int)(id - (long long)b * ystride);
        float v = 0.f;
        if (i < n + 2 * pad) {
            int j = i - pad;
            if (j < 0) j = -j;                      // reflect without repeating the edge sample
            if (j >= n) j = 2 * (n - 1) - j;
            v = x[(long long)b * n + j];
        }
        y[id] = v;
    }
}
// spec [M][2*nfp] interleaved (re, im) -> pw [M][kp]: re^2 + im^2 for k < nfreq, 0 for the padding columns
__global__ void power_spectrum(const float* __restrict__ spec, float* __restrict__ pw, long long M, int nfreq, int kp, int ldspec) {
    const long long total = M * kp;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const long long m = id / kp;
        const int k = (int)(id - m * kp);
        float v = 0.f;
        if (k < nfreq) {
            const float2 c = *reinterpret_cast<const float2*>(spec + m * ldspec + 2 * k);
            v = c.x * c.x + c.y * c.y;
        }
        pw[id] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming front-end per slot of the stream pool (rnnt_pool_wave).  A slot has received n samples x[0, n) and emitted the frames
// [0, f0); frame f covers x[f*hop - half, f*hop + half) of the reflect-padded signal.  Everything a later frame can still read is
// the CARRY x[cs, n), cs = max(0, f0*hop - half - 1): the next frame's span starts at f0*hop - half, and the right reflection
// j -> 2(n-1) - j of a final frame centred on n (n a multiple of hop) reads one sample before its own span.  Its length is at most
// n_fft: f0 is the first frame that does not fit, f0*hop + half > n, so n - cs <= 2*half; with f0*hop <= half + 1, n < n_fft.
// With n_fft < hop the carry start can lie beyond n: the samples in the gap between two frames are dropped as they arrive.
// One push stages, per row, the samples its new frames read so that frame f0 starts at position WAVE_PRE of a 16-byte aligned row
// (position p holds x index j0 + p - WAVE_PRE, j0 = f0*hop - half, reflected at either end), then rolls the carry from that row.
// wave_plan_row is the one place the index arithmetic lives: host validation, rnnt_wave_stage_host and both kernels call it.
// ------------------------------------------------------------------------------------------------
constexpr int WAVE_HOP = 512, WAVE_PRE = 4, WAVE_MAX_NFFT = 4096, WAVE_CARRY_CAP = WAVE_MAX_NFFT, WAVE_TAB_INTS = 4;
static_assert(WAVE_PRE % 4 == 0 && WAVE_PRE >= 1, "frame 0 of a staged row is 16-byte aligned and one carried sample precedes it");

struct WaveRow {
    int n_old, n_new, n_tot, final;
    int f0, nf;              // first frame of the push, frames it emits
    int cs_old, cl_old;      // carry before the push: x[cs_old, cs_old + cl_old)
    int cs_new, cl_new;      // and after it
    int j0;                  // x index at staged position WAVE_PRE
    int len;                 // staged positions [0, len) hold samples, the rest of the row is zero
};
// frames emittable from n samples: every frame whose span ends by n once frame 0's left reflection (x[half]) exists; at the end of
// the utterance all 1 + n/hop of them, none when reflect padding is impossible (n <= half)
__host__ __device__ inline int wave_frames(int n, int half, int final) {
    if (final) return n > half ? 1 + n / WAVE_HOP : 0;
    return n >= half + 1 ? (n - half) / WAVE_HOP + 1 : 0;
}
__host__ __device__ inline WaveRow wave_plan_row(int n_old, int n_new, int final, int n_fft) {
    WaveRow r;
    const int half = n_fft / 2;
    r.n_old = n_old; r.n_new = n_new; r.n_tot = n_old + n_new; r.final = final;
    r.f0 = wave_frames(n_old, half, 0);
    r.nf = wave_frames(r.n_tot, half, final) - r.f0;
    r.j0 = r.f0 * WAVE_HOP - half;
    r.cs_old = r.j0 - 1 > 0 ? r.j0 - 1 : 0;
    r.cl_old = n_old > r.cs_old ? n_old - r.cs_old : 0;
    const int j1 = (r.f0 + r.nf) * WAVE_HOP - half;
    r.cs_new = j1 - 1 > 0 ? j1 - 1 : 0;
    r.cl_new = r.n_tot > r.cs_new ? r.n_tot - r.cs_new : 0;
    const int span = r.nf > 0 ? (r.nf - 1) * WAVE_HOP + n_fft : 0, held = r.n_tot - r.j0;
    r.len = WAVE_PRE + (span > held ? span : (held > 0 ? held : 0));
    return r;
}
// the value at staged position p < r.len: carry | new samples, reflected at the left edge and, at the end of the utterance, the right
__host__ __device__ inline float wave_sample(const WaveRow& r, const float* carry, const float* fresh, int p) {
    int j = r.j0 + p - WAVE_PRE;
    if (j < 0) j = -j;                               // reflect without repeating the edge sample
    if (j >= r.n_tot) {
        if (!r.final) return 0.f;
        j = 2 * (r.n_tot - 1) - j;
        if (j < 0) return 0.f;
    }
    if (j >= r.n_old) return fresh[j - r.n_old];
    const int k = j - r.cs_old;
    return k >= 0 && k < r.cl_old ? carry[k] : 0.f;   // outside the carry: a position no frame reads
}
// tab: WAVE_TAB_INTS per active row = slot, samples so far, new samples, final.  staged [n][stride], zero-filled beyond a row's samples.
__global__ void wave_stage(const float* __restrict__ wave, const float* __restrict__ carry, float* __restrict__ staged, const int* __restrict__ tab,
                           int n, int n_samples, int n_fft, long long stride) {
    const long long total = (long long)n * stride;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(id / stride);
        const int p = (int)(id - (long long)i * stride);
        const int* e = tab + i * WAVE_TAB_INTS;
        const WaveRow r = wave_plan_row(e[1], e[2], e[3], n_fft);
        staged[id] = p < r.len ? wave_sample(r, carry + (long long)e[0] * WAVE_CARRY_CAP, wave + (long long)i * n_samples, p) : 0.f;
    }
}
// carry[slot][k] = x[cs_new + k] from the staged row (never from the carry itself: no read/write overlap inside the launch)
__global__ void wave_carry_roll(const float* __restrict__ staged, float* __restrict__ carry, const int* __restrict__ tab, int n, int n_fft, long long stride) {
    const long long total = (long long)n * n_fft;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(id / n_fft);
        const int k = (int)(id - (long long)i * n_fft);
        const int* e = tab + i * WAVE_TAB_INTS;
        const WaveRow r = wave_plan_row(e[1], e[2], e[3], n_fft);
        if (k < r.cl_new) carry[(long long)e[0] * WAVE_CARRY_CAP + k] = staged[(long long)i * stride + (r.cs_new + k - r.j0 + WAVE_PRE)];
    }
}
