// Back-off n-gram model for shallow fusion in the CTC prefix search (rnnt_ctc_prefix.hip.h) and the transducer prefix search
// (rnnt_prefix.hip.h) as the flat tables rnnt_ngram_set uploads,
// its step, and the kernel that scores given token sequences with it (ngram_score_rows).
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
// The model is a trie over the listed n-grams (node 0 = the root, node ids in list order) with Aho-Corasick fail arcs: fail[c] is the
// node of the longest proper suffix of c's n-gram that is listed.  Children are a CSR of (token, child) sorted by token per node, as
// in the context graph; the root's children are also a dense row [vocab + 2], since every back-off chain ends there.  The host
// prescales the values once (W = weight * logp + bonus, B = weight * bow, U = weight * unk + bonus), so the step only ADDS, in one
// order, and host, device and the f64 restatement give the same bits.
#pragma once

// fail == nullptr: no model.  eos < 0: no n-gram ends in EOS, the end term is 0.
struct NgTables {
    const int* fail; const int* off; const int* ctok; const int* cid;
    const int* root;             // [vocab + 2] child of the root over a token, or -1
    const double* W; const double* B;
    double U;
    int start, eos;
};

// a hypothesis record holds NG_START until its first step: the start state of the model the search runs under
constexpr int NG_START = -1;

__host__ __device__ inline int ng_child(const NgTables& g, int node, int tok) {
    return node == 0 ? g.root[tok] : cg_child(g.off, g.ctok, g.cid, node, tok);
}

// step(state, tok): the score, *next = the node it lands in.  Additions only, in this order.
__host__ __device__ inline double ng_step(const NgTables& g, int state, int tok, int* next) {
    double acc = 0.0;
    int node = state == NG_START ? g.start : state;
    for (;;) {
        const int c = ng_child(g, node, tok);
        if (c >= 0) { *next = c; return acc + g.W[c]; }
        if (node == 0) { *next = 0; return acc + g.U; }
        acc += g.B[node];
        node = g.fail[node];
    }
}

__host__ __device__ inline double ng_eos(const NgTables& g, int state) {
    int nx;
    return g.eos < 0 ? 0.0 : ng_step(g, state, g.eos, &nx);
}

// rnnt_ngram_score: thread i walks sequence i (tokens [n][cap], lens [n]) from the start state.  step [n][cap] per-token scores,
// zero beyond the length; total [n] their sum in walk order, plus the end term when with_eos.
struct NgScoreP {
    NgTables g;
    const int* lens; const int* tokens;
    double* step; double* total;
    int n, cap, with_eos;
};

__global__ __launch_bounds__(64) void ngram_score_rows(NgScoreP p) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= p.n) return;
    const int len = p.lens[i];
    const int* tk = p.tokens + (size_t)i * p.cap;
    double* out = p.step + (size_t)i * p.cap;
    int state = NG_START;
    double tot = 0.0;
    for (int q = 0; q < p.cap; ++q) {
        double sc = 0.0;
        if (q < len) {
            int nx;
            sc = ng_step(p.g, state, tk[q], &nx);
            state = nx;
            tot += sc;
        }
        out[q] = sc;
    }
    if (p.with_eos) tot += ng_eos(p.g, state);
    p.total[i] = tot;
}
