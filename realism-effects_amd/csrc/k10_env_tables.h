// K10 cores: the arithmetic of the environment's importance tables — what rfx_amd/envmap.py build_importance (js/envmap.js buildImportance) computes
// on the host, the reference's EquirectHdrInfoUniform.gatherData — with no HIP dependency, in the manner of k9_piz.h: k10_env_tables.hip runs these
// statements on the device, a plain x86 program (tests/test_env_tables_cpu.py builds one under the sanitizers) runs the same ones in k10_host_build.
//
// The contract is BIT IDENTITY with build_importance for every finite input, which fixes the order of every rounding:
//   weight      (0.2126 r + 0.7152 g) + 0.0722 b, the operands widened to double first: three double multiplies, two double adds, no fma
//               (this file and its users are compiled -ffp-contract=off, and every function below says so itself)
//   row sums    a chain of double adds, left to right, that STARTS with the first weight (numpy's cumsum: a row of -0.0 keeps its sign)
//   row CDF     (float)run, then — the row's sum non-zero — (float)((double)(float)run / sum): a correctly rounded double divide; an all-black row
//               keeps its unnormalised zeros
//   marginal    the same rule over the H row sums, one chain of H adds
//   total       the row-major chain over all W H weights: NOT the sum of the row sums (the two differ in the double)
//   inverse     the reference's own probe sequence per entry (k10_closest): with a negative texel the CDF is not monotone, and the answer is the
//               probe sequence's, not a lower bound
//   flipY       the worker's lossy "un-flip" is reproduced (k10_src_row): in the array order the worker sees — the stored (GL) order reversed — row
//               r ends up holding row min(r, H - 1 - r) of that order
// NaN / Inf texels are outside the contract.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef K10_FN
#define K10_FN static inline
#endif
#if defined(__clang__)
#define K10_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define K10_NO_CONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

constexpr int K10_TILE = 64;           // k10_rows: lanes = rows of a workgroup, and the columns of one staged tile
constexpr int K10_TOTAL_CHUNK = 2048;  // k10_total: weights per LDS buffer (two buffers)
constexpr int K10_MAX_EDGE = 16384;    // rfx_set_environment's limit: a row's CDF is 64 KiB of LDS

// what K10 leaves behind the tables (device memory; K1 reads `whole` and `decimal`)
struct K10Sums {
    double total;          // totalSumValue
    float whole, decimal;  // (float)trunc(total), (float)(total - trunc(total))
};

// the row of the stored level 0 (row 0 = bottom, as rfx_set_environment keeps it) that row r of the tables is built from
K10_FN int k10_src_row(int r, int H, int flipY) {
    if (!flipY) return r;
    const int m = r < H - 1 - r ? r : H - 1 - r;
    return H - 1 - m;
}
K10_FN double k10_weight(float r, float g, float b) {
    K10_NO_CONTRACT
    const double x = 0.2126 * (double)r, y = 0.7152 * (double)g, z = 0.0722 * (double)b;
    const double xy = x + y;
    return xy + z;
}
// one CDF entry, normalised by its row's (or the column of row sums') last running sum
K10_FN float k10_normalise(float run, double sum) {
    K10_NO_CONTRACT
    return sum != 0.0 ? (float)((double)run / sum) : run;
}
// binarySearchFindClosestIndexOf for target (i + 1) / n: cdf(k) is entry k of the normalised CDF
template <class CDF>
K10_FN int k10_closest(const CDF &cdf, int n, int i) {
    K10_NO_CONTRACT
    const double target = (double)(i + 1) / (double)n;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)cdf(mid) < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
K10_FN float k10_centre(int index, int n) {
    K10_NO_CONTRACT
    return (float)(((double)index + 0.5) / (double)n);
}
K10_FN void k10_split_total(double total, K10Sums *s) {
    K10_NO_CONTRACT
    const double whole = (double)(long long)total;  // the hosts' float(int(total)): towards zero, and +0 for a total in (-1, 0)
    s->total = total;
    s->whole = (float)whole;
    s->decimal = (float)(total - whole);
}

#ifndef K10_NO_HOST
// The whole build in one thread, phase by phase as the kernels do it: texels = the stored level 0 (W x H RGBA floats), marginal H floats, conditional
// W x H, cdf a scratch row of max(W, H) floats, rowsum H doubles.
static inline void k10_host_build(const float *texels, int W, int H, int flipY, float *marginal, float *conditional, float *cdf, double *rowsum, K10Sums *sums) {
    K10_NO_CONTRACT
    double total = 0.0;
    for (int r = 0; r < H; r++) {
        const float *row = texels + (size_t)k10_src_row(r, H, flipY) * W * 4;
        double run = 0.0;
        for (int x = 0; x < W; x++) {
            const double w = k10_weight(row[4 * x], row[4 * x + 1], row[4 * x + 2]);
            run = x ? run + w : w;
            total = (r | x) ? total + w : w;
            cdf[x] = (float)run;
        }
        rowsum[r] = run;
        for (int x = 0; x < W; x++) cdf[x] = k10_normalise(cdf[x], run);
        const auto at = [&](int k) { return cdf[k]; };
        for (int x = 0; x < W; x++) conditional[(size_t)r * W + x] = k10_centre(k10_closest(at, W, x), W);
    }
    double run = 0.0;
    for (int r = 0; r < H; r++) {
        run = r ? run + rowsum[r] : rowsum[r];
        cdf[r] = (float)run;
    }
    for (int r = 0; r < H; r++) cdf[r] = k10_normalise(cdf[r], run);
    const auto at = [&](int k) { return cdf[k]; };
    for (int r = 0; r < H; r++) marginal[r] = k10_centre(k10_closest(at, H, r), H);
    k10_split_total(total, sums);
}
#endif
