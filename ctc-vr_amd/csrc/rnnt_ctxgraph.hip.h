// WeNet's ContextGraph (wenet/utils/context_graph.py) as the flat tables rnnt_context_set uploads, and its forward step; shared by the
// CTC prefix search (rnnt_ctc_prefix.hip.h) and the transducer prefix search (rnnt_prefix.hip.h).
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
#pragma once

// context graph (fail == nullptr: none): flat node arrays, children as a CSR of (token, child) sorted by token per node
struct CpGraph {
    const int* fail; const int* off; const int* ctok; const int* cid;
    const double* tscore; const double* nscore; const double* oscore;
};

// the child of `node` over `tok`, or -1: binary search in the node's sorted CSR row
__host__ __device__ inline int cg_child(const int* off, const int* ctok, const int* cid, int node, int tok) {
    int lo = off[node], hi = off[node + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, v = ctok[mid];
        if (v == tok) return cid[mid];
        if (v < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// ContextGraph.forward_one_step (context_graph.py:212-247) on the flat tables: returns the step's score, *next = the node it lands in
__host__ __device__ inline double cg_step(const int* fail, const int* off, const int* ctok, const int* cid, const double* tscore,
                                          const double* nscore, const double* oscore, int state, int tok, int* next) {
    int node = cg_child(off, ctok, cid, state, tok);
    double score;
    if (node >= 0) score = tscore[node];
    else {
        node = fail[state];
        while (cg_child(off, ctok, cid, node, tok) < 0) {
            node = fail[node];
            if (node == 0) break;                                    // root
        }
        const int c = cg_child(off, ctok, cid, node, tok);
        if (c >= 0) node = c;
        score = nscore[node] - nscore[state];                        // the score of the fail path
    }
    *next = node;
    return score + oscore[node];
}
