// Standalone check + timing of the layer-major attention kernels in bf16x3 (rel_attention_lm_bf, the tiled form, against
// rel_attention_lm_res, the resident form), at the bench geometry: B = 64 streams x 188 frames, chunks of 3 encoder frames (the last
// one 5), chunk 0's K/V parked in the last rows of a tcap-row cache, every later chunk's window [0, end of chunk).  pshift drifts by
// one row per chunk (synthetic: the kernels only need the positional rows in range).  Checks: resident vs tiled, a CPU double
// reference on sampled rows, resident run-to-run bitwise; then times both, and the resident kernel's ablations (ABL bits: 1 no K/V
// loads, 2 no positional term, 4 no online softmax; results meaningless there).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/attn_check tools/attn_check.hip && tools/attn_check [tcap]
#include "../ctc-vr_amd/csrc/rnnt_kernels.hip.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static const int B = 64, TQ0 = 3;

template <typename L>
static float time_us(L launch, int n) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    launch(); CK(hipDeviceSynchronize());
    CK(hipEventRecord(a));
    for (int k = 0; k < n; ++k) launch();
    CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, a, b));
    CK(hipEventDestroy(a)); CK(hipEventDestroy(b));
    return 1000.f * ms / n;
}

int main(int argc, char** argv) {
    const int tcap = argc > 1 ? atoi(argv[1]) : 256;
    // ---- chunk plan and rows (host_lm.hip.inc's block building for a uniform call) -------------------------------------------
    std::vector<int> tq;
    for (int c = 0; c < 61; ++c) tq.push_back(3);
    tq.push_back(5);
    int F = 0;
    for (int t : tq) F += t;
    const int park0 = tcap - TQ0;
    if (tcap < F) { printf("tcap %d < F %d\n", tcap, F); return 1; }
    std::vector<LmBlock> blocks;
    LmBlock cur;
    int pmax = 0;
    auto reset = [&]() { memset(&cur, 0, sizeof(cur)); for (int k = 0; k < LM_ROWS; ++k) cur.r[k].f = -1; };
    auto flush = [&]() { if (cur.n_rows) blocks.push_back(cur); reset(); };
    reset();
    for (int c = 0, fpos = 0; c < (int)tq.size(); fpos += tq[c], ++c) {
        const int kv0 = c == 0 ? park0 : 0, T2 = c == 0 ? TQ0 : fpos - TQ0 + tq[c];
        const int psh = 2000 + c - kv0;
        for (int q0 = 0; q0 < tq[c]; ++q0) {
            const LmRow rw{fpos + q0, kv0, kv0 + T2, psh};
            bool join = cur.n_rows > 0 && cur.n_rows < LM_ROWS && rw.ks <= cur.amax && rw.ke >= cur.amin;
            if (join) join = std::max(pmax, psh) - std::min(cur.pmin, psh) <= LM_PEXT;
            if (!join) { flush(); cur.amin = rw.ks; cur.amax = rw.ke; cur.pmin = psh; pmax = psh; }
            cur.amin = std::min(cur.amin, rw.ks); cur.amax = std::max(cur.amax, rw.ke);
            cur.pmin = std::min(cur.pmin, psh); pmax = std::max(pmax, psh);
            cur.r[cur.n_rows++] = rw;
        }
    }
    flush();
    const std::vector<LmRow> rows = lm_rows_of(blocks.data(), blocks.size());
    std::vector<LmResHdr> hdr;
    std::vector<LmRow> flat;
    int stride = 0;
    if (!lm_res_plan({rows}, hdr, flat, stride)) { printf("the resident plan refuses this geometry\n"); return 1; }
    printf("B %d F %d tcap %d: %zu blocks, %d segments, LDS tiled %d B resident %d B\n", B, F, tcap, blocks.size(), hdr[0].nseg, LMB_LDS, LMR_LDS);
    // ---- data ---------------------------------------------------------------------------------------------------------------------
    std::mt19937 rng(7);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> hq((size_t)B * F * RNNT_D), hk((size_t)B * tcap * RNNT_D), hv(hk.size()), hp((size_t)RNNT_PE_LEN * RNNT_D), hu(RNNT_D), hw(RNNT_D);
    for (auto& x : hq) x = nd(rng);
    for (auto& x : hk) x = nd(rng);
    for (auto& x : hv) x = nd(rng);
    for (auto& x : hp) x = 0.5f * nd(rng);
    for (auto& x : hu) x = 0.1f * nd(rng);
    for (auto& x : hw) x = 0.1f * nd(rng);
    float *q, *kc, *vc, *pt, *bu, *bv, *o1, *o2, *o3;
    LmBlock* dblk;
    LmResHdr* dhdr;
    LmRow* drows;
    const size_t on = (size_t)B * F * RNNT_D;
    CK(hipMalloc(&q, hq.size() * 4)); CK(hipMalloc(&kc, hk.size() * 4)); CK(hipMalloc(&vc, hv.size() * 4)); CK(hipMalloc(&pt, hp.size() * 4));
    CK(hipMalloc(&bu, RNNT_D * 4)); CK(hipMalloc(&bv, RNNT_D * 4));
    CK(hipMalloc(&o1, on * 4)); CK(hipMalloc(&o2, on * 4)); CK(hipMalloc(&o3, on * 4));
    CK(hipMalloc(&dblk, blocks.size() * sizeof(LmBlock))); CK(hipMalloc(&dhdr, sizeof(LmResHdr))); CK(hipMalloc(&drows, flat.size() * sizeof(LmRow)));
    CK(hipMemcpy(q, hq.data(), hq.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(kc, hk.data(), hk.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(vc, hv.data(), hv.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(pt, hp.data(), hp.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(bu, hu.data(), RNNT_D * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(bv, hw.data(), RNNT_D * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dblk, blocks.data(), blocks.size() * sizeof(LmBlock), hipMemcpyHostToDevice));
    CK(hipMemcpy(dhdr, hdr.data(), sizeof(LmResHdr), hipMemcpyHostToDevice));
    CK(hipMemcpy(drows, flat.data(), flat.size() * sizeof(LmRow), hipMemcpyHostToDevice));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rel_attention_lm_bf<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LMB_LDS));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rel_attention_lm_res<2, false, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, LMR_LDS));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rel_attention_lm_res<2, false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, LMR_LDS));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rel_attention_lm_res<2, false, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, LMR_LDS));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rel_attention_lm_res<2, false, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, LMR_LDS));
    const LmAttnP ta{q, kc, vc, pt, bu, bv, o1, dblk, F, (long long)tcap, nullptr, 0};
    LmResP ra{q, kc, vc, pt, bu, bv, o2, dhdr, drows, stride, F, (long long)tcap, nullptr, 0};
    const dim3 tg(B * RNNT_H, (unsigned)blocks.size()), rg(B * RNNT_H);
    auto tiled = [&]() { hipLaunchKernelGGL((rel_attention_lm_bf<2, false>), tg, dim3(256), LMB_LDS, 0, ta); };
    auto res = [&]() { hipLaunchKernelGGL((rel_attention_lm_res<2, false, 0>), rg, dim3(64 * LMR_NW), LMR_LDS, 0, ra); };
    tiled(); res();
    ra.out = o3; res(); ra.out = o2;
    CK(hipDeviceSynchronize());
    std::vector<float> r1(on), r2(on), r3(on);
    CK(hipMemcpy(r1.data(), o1, on * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(r2.data(), o2, on * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(r3.data(), o3, on * 4, hipMemcpyDeviceToHost));
    double dmax = 0.0;
    bool finite = true;
    for (size_t k = 0; k < on; ++k) { dmax = std::max(dmax, (double)std::fabs(r1[k] - r2[k])); finite = finite && std::isfinite(r2[k]); }
    const bool bitwise = memcmp(r2.data(), r3.data(), on * 4) == 0;
    // CPU double reference on sampled (stream, row, head)
    double emax_t = 0.0, emax_r = 0.0;
    for (int smp = 0; smp < 64; ++smp) {
        const int b = (smp * 37) % B, fi = (smp * 53) % (int)rows.size(), h = smp % RNNT_H;
        const LmRow& rw = rows[fi];
        std::vector<double> sc;
        for (int a = rw.ks; a < rw.ke; ++a) {
            double s = 0.0;
            for (int d = 0; d < RNNT_DK; ++d) {
                const double qd = hq[((size_t)b * F + rw.f) * RNNT_D + h * RNNT_DK + d];
                s += (qd + hu[h * RNNT_DK + d]) * hk[((size_t)b * tcap + a) * RNNT_D + h * RNNT_DK + d];
                s += (qd + hw[h * RNNT_DK + d]) * hp[(size_t)(a + rw.pshift) * RNNT_D + h * RNNT_DK + d];
            }
            sc.push_back(s / 8.0);
        }
        double mx = -1e300, sum = 0.0;
        for (double s : sc) mx = std::max(mx, s);
        for (double& s : sc) { s = std::exp(s - mx); sum += s; }
        for (int d = 0; d < RNNT_DK; ++d) {
            double acc = 0.0;
            for (int a = rw.ks; a < rw.ke; ++a) acc += sc[a - rw.ks] * hv[((size_t)b * tcap + a) * RNNT_D + h * RNNT_DK + d];
            acc /= sum;
            const size_t ix = ((size_t)b * F + rw.f) * RNNT_D + h * RNNT_DK + d;
            emax_t = std::max(emax_t, std::fabs(acc - r1[ix]));
            emax_r = std::max(emax_r, std::fabs(acc - r2[ix]));
        }
    }
    printf("resident vs tiled max |diff| %.3e; vs CPU double: tiled %.3e resident %.3e; resident finite %d, run-to-run bitwise %d\n", dmax, emax_t, emax_r,
           (int)finite, (int)bitwise);
    const bool ok = finite && bitwise && dmax < 2e-5 && emax_r < 1e-4;
    // ---- timing ---------------------------------------------------------------------------------------------------------------------
    const int n = 50;
    printf("tiled rel_attention_lm_bf      %7.1f us\n", time_us(tiled, n));
    printf("resident rel_attention_lm_res  %7.1f us\n", time_us(res, n));
    printf("  ablation no K/V loads        %7.1f us\n", time_us([&]() { hipLaunchKernelGGL((rel_attention_lm_res<2, false, 1>), rg, dim3(64 * LMR_NW), LMR_LDS, 0, ra); }, n));
    printf("  ablation no positional term  %7.1f us\n", time_us([&]() { hipLaunchKernelGGL((rel_attention_lm_res<2, false, 2>), rg, dim3(64 * LMR_NW), LMR_LDS, 0, ra); }, n));
    printf("  ablation no online softmax   %7.1f us\n", time_us([&]() { hipLaunchKernelGGL((rel_attention_lm_res<2, false, 4>), rg, dim3(64 * LMR_NW), LMR_LDS, 0, ra); }, n));
    printf("%s\n", ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
