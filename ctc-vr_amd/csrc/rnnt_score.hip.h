// Teacher-forced scoring: the forward (alpha) recursions of the transducer and CTC likelihoods, and the gather behind the
// fallback of the fused lattice kernel.  Forward only: no gradients.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).  Below them their max-plus (Viterbi) twins for forced
// alignment: same wavefronts, back-pointers in global memory, and the back-trace by one lane of the same launch.
//
// The transducer likelihood is the sum over all monotonic alignments (torchaudio.functional.rnnt_loss with reduction "none",
// online_rnnt_model.py:247-255; its clamp only touches gradients); the CTC one is nn.CTCLoss(reduction="none")
// (online_rnnt_model.py:22-23).  Both recursions run in f64 like the beam scores: one workgroup per utterance, a chain of
// T_b + U_b (transducer) or T_b (CTC) dependent steps with one barrier each, so they are latency-bound and not tuned here.
#pragma once

#define SCORE_UMAX 255           // labels per utterance: transducer threads cover u = 0..255, CTC threads s = 0..510

// fallback of joint_lattice_rows<.., PICK>: the two columns of a materialised log-softmax lattice lat [M][V], M = B * T * U1
__global__ void pick_gather(const float* __restrict__ lat, const int* __restrict__ targets, float* __restrict__ pick, long long M, int T,
                            int U1, int V, int tstride, int blank) {
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long long)gridDim.x * blockDim.x) {
        const long long bt = m / U1;
        const int u = (int)(m - bt * U1);
        int vt = targets ? ldgi(targets + (bt / T) * tstride + min(u, tstride - 1)) : blank;
        vt = min(max(vt, 0), V - 1);                           // padded cells only: valid labels are checked on the host
        pick[2 * m] = ldg1(lat + m * V + blank);
        pick[2 * m + 1] = ldg1(lat + m * V + vt);
    }
}

__device__ __forceinline__ double score_logaddexp(double a, double b) {
    const double mx = fmax(a, b), mn = fmin(a, b);
    return mx == -INFINITY ? mx : mx + log1p(exp(mn - mx));
}

// alpha[0,0] = 0; alpha[t,u] = logaddexp(alpha[t-1,u] + pick[t-1,u][0], alpha[t,u-1] + pick[t,u-1][1]);
// nll = -(alpha[T_b-1,U_b] + pick[T_b-1,U_b][0]).  Anti-diagonal wavefront: on diagonal d thread u owns cell (d - u, u), keeps its
// own alpha in a register and hands it to thread u + 1 through LDS (two buffers: one barrier per diagonal).
// pick [B][T][U1][2]; lens [2][B]: T_b in [1, T], U_b in [0, U1 - 1]; launched with 256 threads, U1 <= 256.
__global__ __launch_bounds__(256) void transducer_alpha(const float* __restrict__ pick, const int* __restrict__ lens, int B, int T, int U1,
                                                        double* __restrict__ nll) {
    __shared__ double xa[2][SCORE_UMAX + 1];
    const int b = blockIdx.x, u = threadIdx.x;
    const int Tb = ldgi(lens + b), Ub = ldgi(lens + B + b);
    const float* pb = pick + (long long)b * T * U1 * 2;
    double a = -INFINITY;
    const int nd = Tb + Ub;                                    // diagonals 0 .. T_b + U_b - 1
    for (int d = 0; d < nd; ++d) {
        const int t = d - u;
        const bool live = u <= Ub && t >= 0 && t < Tb;
        if (live) {
            if (d == 0) a = 0.0;
            else {
                // `a` still holds alpha[t-1,u] (the cell this thread owned on diagonal d - 1), the neighbour's alpha[t,u-1] is in LDS
                const double below = t > 0 ? a + (double)ldg1(pb + ((long long)(t - 1) * U1 + u) * 2) : -INFINITY;
                const double left = u > 0 ? xa[(d - 1) & 1][u - 1] + (double)ldg1(pb + ((long long)t * U1 + u - 1) * 2 + 1) : -INFINITY;
                a = t == 0 ? left : (u == 0 ? below : score_logaddexp(below, left));
            }
        }
        xa[d & 1][u] = a;
        __syncthreads();
    }
    if (u == Ub) nll[b] = -(a + (double)ldg1(pb + ((long long)(Tb - 1) * U1 + Ub) * 2));
}

// transducer_alpha over the n-best layout of rnnt_transducer_nll_nbest: the N hypotheses of an utterance lie side by side along U,
// pick [B][T][N * U1][2], so cell (t, u) of hypothesis n is at ((b T + t) N U1 + n U1 + u) * 2.  One workgroup per (b, n) =
// blockIdx.x; tlens [B]: T_b in [1, T]; ulens [B][N]: U_bn in [0, U1 - 1]; nhyp [B].  Workgroups with n >= nhyp[b] store 0 and
// leave (their lengths are not read).  Same recursion, same order of operations; launched with 256 threads, U1 <= 256.
__global__ __launch_bounds__(256) void transducer_alpha_nbest(const float* __restrict__ pick, const int* __restrict__ tlens,
                                                              const int* __restrict__ ulens, const int* __restrict__ nhyp, int T, int N,
                                                              int U1, double* __restrict__ nll) {
    __shared__ double xa[2][SCORE_UMAX + 1];
    const int bn = blockIdx.x, b = bn / N, n = bn - b * N, u = threadIdx.x;
    if (n >= ldgi(nhyp + b)) {                                 // uniform over the workgroup
        if (u == 0) nll[bn] = 0.0;
        return;
    }
    const int Tb = ldgi(tlens + b), Ub = ldgi(ulens + bn);
    const long long US = (long long)N * U1;                    // cells per frame
    const float* pb = pick + ((long long)b * T * US + (long long)n * U1) * 2;
    double a = -INFINITY;
    const int nd = Tb + Ub;
    for (int d = 0; d < nd; ++d) {
        const int t = d - u;
        const bool live = u <= Ub && t >= 0 && t < Tb;
        if (live) {
            if (d == 0) a = 0.0;
            else {
                const double below = t > 0 ? a + (double)ldg1(pb + ((long long)(t - 1) * US + u) * 2) : -INFINITY;
                const double left = u > 0 ? xa[(d - 1) & 1][u - 1] + (double)ldg1(pb + ((long long)t * US + u - 1) * 2 + 1) : -INFINITY;
                a = t == 0 ? left : (u == 0 ? below : score_logaddexp(below, left));
            }
        }
        xa[d & 1][u] = a;
        __syncthreads();
    }
    if (u == Ub) nll[bn] = -(a + (double)ldg1(pb + ((long long)(Tb - 1) * US + Ub) * 2));
}

// Standard CTC forward over the S = 2 L_b + 1 extended states (blank, y_1, blank, ..., y_L, blank) and T_b frames, the
// recursion of nn.CTCLoss: alpha_t[s] = logsumexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2] if y differs) + lp[t][ext s].
// nll = -logaddexp(alpha[S-1], alpha[S-2]); an infeasible pair (fewer frames than labels plus adjacent repeats) keeps both at
// -inf and gives +inf.  lp [B][T][V] log-probabilities; targets [B][tstride]; lens [2][B]; launched with 512 threads.
__global__ __launch_bounds__(512) void ctc_alpha(const float* __restrict__ lp, const int* __restrict__ targets, const int* __restrict__ lens,
                                                 int B, int T, int V, int tstride, int blank, double* __restrict__ nll) {
    __shared__ double xa[2][2 * SCORE_UMAX + 2];
    const int b = blockIdx.x, s = threadIdx.x;
    const int Tb = ldgi(lens + b), Lb = ldgi(lens + B + b);
    const int S = 2 * Lb + 1;
    const bool live = s < S;
    const float* lb = lp + (long long)b * T * V;
    int col = blank, skip = 0;
    if (live && (s & 1)) {
        col = ldgi(targets + (long long)b * tstride + (s >> 1));
        skip = s >= 3 && ldgi(targets + (long long)b * tstride + (s >> 1) - 1) != col;
    }
    double a = live && s < 2 ? (double)ldg1(lb + col) : -INFINITY;
    xa[0][s] = a;
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        if (live) {
            const double* pv = xa[(t - 1) & 1];
            const double a1 = s >= 1 ? pv[s - 1] : -INFINITY, a2 = skip ? pv[s - 2] : -INFINITY;
            double mx = fmax(a, fmax(a1, a2));
            if (mx == -INFINITY) mx = 0.0;
            a = log(exp(a - mx) + exp(a1 - mx) + exp(a2 - mx)) + mx + (double)ldg1(lb + (long long)t * V + col);
        }
        xa[t & 1][s] = a;
        __syncthreads();
    }
    if (s == S - 1) nll[b] = -score_logaddexp(a, S > 1 ? xa[(Tb - 1) & 1][S - 2] : -INFINITY);
}

// ---- forced alignment: the max-plus twins of the two recursions ----------------------------------------------------------------------
// Only f64 additions and comparisons, so both are bitwise their float64 restatements (ctc_vr_amd.testing.transducer_align_ref,
// ctc_align_ref), ties included.  Back-pointers go to a global work buffer, not LDS: a column's words are written once, 32 (16)
// frames at a time, and the back-trace reads at most U_b + T_b / 32 (T_b) of them, so the size of an utterance never selects
// another code path.  The stores of a workgroup are visible to its lane 0 after the barrier that ends the recursion.

// v[0,0] = 0; v[t,u] = max(v[t-1,u] + pick[t-1,u][0], v[t,u-1] + pick[t,u-1][1]), the blank move winning ties;
// best = v[T_b-1,U_b] + pick[T_b-1,U_b][0].  Wavefront, arguments and launch as transducer_alpha.  Bit t & 31 of
// bp[b][u][t >> 5] is set when cell (t, u) was reached by the label move; W = ceil(T / 32) words per column.  emit [B][ts]:
// emit[b][u] = the frame at which label u is emitted on the best path (non-decreasing in u), -1 for u >= U_b.
__global__ __launch_bounds__(256) void transducer_viterbi(const float* __restrict__ pick, const int* __restrict__ lens, int B, int T, int U1,
                                                          int ts, unsigned* bp, double* __restrict__ best, int* __restrict__ emit) {
    __shared__ double xv[2][SCORE_UMAX + 1];
    const int b = blockIdx.x, u = threadIdx.x;
    const int Tb = ldgi(lens + b), Ub = ldgi(lens + B + b);
    const int W = (T + 31) >> 5;
    const float* pb = pick + (long long)b * T * U1 * 2;
    unsigned* bpb = bp + (long long)b * U1 * W;
    double v = -INFINITY;
    unsigned bits = 0;
    const int nd = Tb + Ub;
    for (int d = 0; d < nd; ++d) {
        const int t = d - u;
        const bool live = u <= Ub && t >= 0 && t < Tb;
        if (live) {
            bool label = false;
            if (d == 0) v = 0.0;
            else {
                const double below = t > 0 ? v + (double)ldg1(pb + ((long long)(t - 1) * U1 + u) * 2) : -INFINITY;
                const double left = u > 0 ? xv[(d - 1) & 1][u - 1] + (double)ldg1(pb + ((long long)t * U1 + u - 1) * 2 + 1) : -INFINITY;
                label = t == 0 || (u > 0 && !(below >= left));
                v = label ? left : below;
            }
            bits |= (unsigned)label << (t & 31);
            if ((t & 31) == 31 || t == Tb - 1) {
                bpb[u * W + (t >> 5)] = bits;
                bits = 0;
            }
        }
        xv[d & 1][u] = v;
        __syncthreads();
    }
    if (u == Ub) best[b] = v + (double)ldg1(pb + ((long long)(Tb - 1) * U1 + Ub) * 2);
    int* eb = emit + (long long)b * ts;
    if (u >= Ub && u < ts) eb[u] = -1;
    if (u == 0) {
        // back-trace from (T_b-1, U_b): T_b - 1 + U_b dependent steps of one lane; a word is reloaded only when the column or the
        // 32-frame block changes.  In row 0 every remaining move is a blank one.
        int t = Tb - 1, uu = Ub, wi = -1;
        unsigned w = 0;
        while (uu > 0 && t >= 0) {
            const int i = uu * W + (t >> 5);
            if (i != wi) { w = bpb[i]; wi = i; }
            if ((w >> (t & 31)) & 1) eb[--uu] = t;
            else --t;
        }
    }
}

// v_t[s] = max(v_{t-1}[s], v_{t-1}[s-1], v_{t-1}[s-2] if y differs) + lp[t][ext s] over ctc_alpha's states; among equals stay
// beats s-1 beats s-2.  The path ends in S-1 if v[S-1] >= v[S-2] (or S == 1), else in S-2; best is that value, -inf for a
// transcript its frames cannot hold, whose row of align is all -1.  Bits 2 (t & 15) .. +1 of bp[b][s][t >> 4] hold the step
// (0, 1 or 2 states down) into (t, s); W = ceil(T / 16) words per state, 2 tstride + 1 states per row.  align [B][T]: the label
// of the state occupied at frame t (the blank included), -1 for t >= T_b.  Arguments and launch as ctc_alpha.
__global__ __launch_bounds__(512) void ctc_viterbi(const float* __restrict__ lp, const int* __restrict__ targets, const int* __restrict__ lens,
                                                   int B, int T, int V, int tstride, int blank, unsigned* bp, double* __restrict__ best,
                                                   int* __restrict__ align) {
    __shared__ double xv[2][2 * SCORE_UMAX + 2];
    const int b = blockIdx.x, s = threadIdx.x;
    const int Tb = ldgi(lens + b), Lb = ldgi(lens + B + b);
    const int S = 2 * Lb + 1, W = (T + 15) >> 4;
    const bool live = s < S;
    const float* lb = lp + (long long)b * T * V;
    unsigned* bpb = bp + (long long)b * (2 * tstride + 1) * W;
    int col = blank, skip = 0;
    if (live && (s & 1)) {
        col = ldgi(targets + (long long)b * tstride + (s >> 1));
        skip = s >= 3 && ldgi(targets + (long long)b * tstride + (s >> 1) - 1) != col;
    }
    double v = live && s < 2 ? (double)ldg1(lb + col) : -INFINITY;
    unsigned bits = 0;
    xv[0][s] = v;
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        if (live) {
            const double* pv = xv[(t - 1) & 1];
            const double a1 = s >= 1 ? pv[s - 1] : -INFINITY, a2 = skip ? pv[s - 2] : -INFINITY;
            double m = v;
            unsigned k = 0;
            if (a1 > m) { m = a1; k = 1; }
            if (a2 > m) { m = a2; k = 2; }
            v = m + (double)ldg1(lb + (long long)t * V + col);
            bits |= k << (2 * (t & 15));
            if ((t & 15) == 15 || t == Tb - 1) {
                bpb[s * W + (t >> 4)] = bits;
                bits = 0;
            }
        }
        xv[t & 1][s] = v;
        __syncthreads();
    }
    const double* fv = xv[(Tb - 1) & 1];
    const double e1 = fv[S - 1], e2 = S > 1 ? fv[S - 2] : -INFINITY;
    const bool last = S == 1 || e1 >= e2;
    const double bs = last ? e1 : e2;
    const bool feasible = !(bs == -INFINITY);
    int* ab = align + (long long)b * T;
    for (int t = (feasible ? Tb : 0) + s; t < T; t += 512) ab[t] = -1;
    if (s == 0) {
        best[b] = bs;
        if (feasible) {
            // back-trace: T_b - 1 dependent steps of one lane, a word reloaded when the state or the 16-frame block changes
            int st = last ? S - 1 : S - 2, wi = -1;
            unsigned w = 0;
            for (int t = Tb - 1;; --t) {
                ab[t] = (st & 1) ? ldgi(targets + (long long)b * tstride + (st >> 1)) : blank;
                if (t == 0) break;
                const int i = st * W + (t >> 4);
                if (i != wi) { w = bpb[i]; wi = i; }
                st = max(st - (int)((w >> (2 * (t & 15))) & 3), 0);
            }
        }
    }
}
