// K10 — the environment's importance tables on the device: marginalWeights, conditionalWeights and totalSumValue from level 0 of the held
// environment, bit for bit what rfx_amd/envmap.py build_importance returns (k10_env_tables.h states the rounding contract and holds the arithmetic).
// Five launches on one stream:
//   k10_rows            one lane per row (the order of a row's adds is the contract: no scan), 64 rows per single-wave workgroup; the texels come
//                       as coalesced 64 x 64 tiles whose WEIGHTS are staged in LDS, the running sums leave as coalesced float tiles — no lane walks
//                       memory at a stride of W x 16 B.  Leaves (float)run in `conditional` and the row sums in the scratch.
//   k10_total           the one sequential part: the row-major chain over all W H weights.  One workgroup; waves 1 .. 4 load the texels of the NEXT
//                       2048 and put their weights into one of two LDS buffers while wave 0 adds the current 2048 in order, every lane reading the
//                       same LDS address (a broadcast), sixteen reads ahead of the adds: one dependent double add per texel.
//   k10_marginal_chain  the chain over the H row sums: (float)run into `marginal`, the last sum into the scratch
//   k10_invert (x 2)    one workgroup per CDF: normalise it into LDS (a row fits at the maximum edge: 16384 floats = 64 KiB), then one probe
//                       sequence per entry; the table overwrites the CDF in place.  Instantiated for three LDS sizes so that small maps keep
//                       their occupancy.
// No atomics, no scratch memory, no host wait.
#include "rfx_device.h"
#include "rfx_kernels.h"

#define K10_FN RFX_DEV
#define K10_NO_HOST
#include "k10_env_tables.h"

namespace {

constexpr int K10_PAD = K10_TILE + 1;  // lane r walks row r of a tile: the odd pitch spreads the lanes over the banks

__global__ __launch_bounds__(K10_TILE) void k10_rows(const float4 *env, int W, int H, int flipY, float *cdf, double *rowsum) {
    __shared__ double w[K10_TILE * K10_PAD];
    __shared__ float f[K10_TILE * K10_PAD];
    const int lane = threadIdx.x, r0 = blockIdx.x * K10_TILE, rows = min(K10_TILE, H - r0);
    double run = 0.0;
    for (int c0 = 0; c0 < W; c0 += K10_TILE) {
        const int cols = min(K10_TILE, W - c0);
        if (lane < cols)
            for (int i = 0; i < rows; i++) {
                const float4 t = env[(size_t)k10_src_row(r0 + i, H, flipY) * W + c0 + lane];
                w[i * K10_PAD + lane] = k10_weight(t.x, t.y, t.z);
            }
        __syncthreads();
        if (lane < rows)
            for (int k = 0; k < cols; k++) {
                const double v = w[lane * K10_PAD + k];
                run = (c0 | k) ? run + v : v;
                f[lane * K10_PAD + k] = (float)run;
            }
        __syncthreads();
        if (lane < cols)
            for (int i = 0; i < rows; i++) cdf[(size_t)(r0 + i) * W + c0 + lane] = f[i * K10_PAD + lane];
    }
    if (lane < rows) rowsum[r0 + lane] = run;
}

constexpr int K10_TOTAL_LOADERS = 256, K10_TOTAL_THREADS = 64 + K10_TOTAL_LOADERS;
#define K10_LOAD16(X, at) _Pragma("unroll") for (int j_ = 0; j_ < 16; j_++) X[j_] = src[(at) + j_]
#define K10_ADD16(X) _Pragma("unroll") for (int j_ = 0; j_ < 16; j_++) total += X[j_]
// the instruction scheduler sinks a register set's LDS reads to just in front of its adds (fewer live registers), which puts the read latency
// back into the chain: nothing moves across this point
#if defined(__HIP_DEVICE_COMPILE__)
#define K10_KEEP_ORDER() __builtin_amdgcn_sched_barrier(0)
#else
#define K10_KEEP_ORDER() ((void)0)
#endif
__global__ __launch_bounds__(K10_TOTAL_THREADS) void k10_total(const float4 *env, int W, int logW, int H, int flipY, K10Sums *sums) {
    __shared__ double buf[2][K10_TOTAL_CHUNK];
    const long long N = (long long)W * H;
    const int tid = threadIdx.x, lt = tid - 64;
    const bool loader = tid >= 64;
    // texel i of the row-major order of the TABLES' rows
    const auto fill = [&](int b, long long base) {
        for (int j = lt; j < K10_TOTAL_CHUNK; j += K10_TOTAL_LOADERS) {
            const long long i = base + j;
            if (i >= N) break;
            const int row = (int)(i >> logW), col = (int)(i & (W - 1));
            const float4 t = env[(size_t)k10_src_row(row, H, flipY) * W + col];
            buf[b][j] = k10_weight(t.x, t.y, t.z);
        }
    };
    if (loader) fill(0, 0);
    __syncthreads();
    double total = 0.0;
    int b = 0;
    for (long long base = 0; base < N; base += K10_TOTAL_CHUNK, b ^= 1) {
        if (loader) {
            if (base + K10_TOTAL_CHUNK < N) fill(b ^ 1, base + K10_TOTAL_CHUNK);
        } else {
            const int n = (int)(N - base < K10_TOTAL_CHUNK ? N - base : K10_TOTAL_CHUNK);
            const double *src = buf[b];
            int k = 0;
            if (base == 0) total = src[k++];  // the chain starts WITH the first weight
            // the adds in order, sixteen at a time from one register set while the LDS reads of the next sixteen fill the other: the chain
            // waits for an add's latency, not for an LDS read's
            double A[16], B[16];
            if (n - k >= 16) {
                K10_LOAD16(A, k);
                k += 16;
                while (n - k >= 32) {
                    K10_LOAD16(B, k);
                    K10_KEEP_ORDER();
                    K10_ADD16(A);
                    K10_KEEP_ORDER();
                    K10_LOAD16(A, k + 16);
                    K10_KEEP_ORDER();
                    K10_ADD16(B);
                    K10_KEEP_ORDER();
                    k += 32;
                }
                if (n - k >= 16) {
                    K10_LOAD16(B, k);
                    K10_KEEP_ORDER();
                    K10_ADD16(A);
                    K10_ADD16(B);
                    k += 16;
                } else K10_ADD16(A);
            }
            for (; k < n; k++) total += src[k];
        }
        __syncthreads();
    }
    if (tid == 0) k10_split_total(total, sums);
}

__global__ __launch_bounds__(64) void k10_marginal_chain(const double *rowsum, int H, float *cdf, double *last) {
    __shared__ double s[64];
    const int lane = threadIdx.x;
    double run = 0.0;
    for (int r0 = 0; r0 < H; r0 += 64) {
        const int n = min(64, H - r0);
        if (lane < n) s[lane] = rowsum[r0 + lane];
        __syncthreads();
        float mine = 0.0f;
        for (int k = 0; k < n; k++) {
            run = (r0 | k) ? run + s[k] : s[k];
            if (k == lane) mine = (float)run;
        }
        if (lane < n) cdf[r0 + lane] = mine;
        __syncthreads();
    }
    if (lane == 0) *last = run;
}

// block b: CDF b (n entries at io + b n, its last running sum sum[b]) -> the inverse table, in place
template <int CAP>
__global__ __launch_bounds__(256) void k10_invert(float *io, const double *sum, int n) {
    __shared__ float cdf[CAP];
    float *row = io + (size_t)blockIdx.x * n;
    const double s = sum[blockIdx.x];
    for (int x = threadIdx.x; x < n; x += 256) cdf[x] = k10_normalise(row[x], s);
    __syncthreads();
    const auto at = [&](int k) { return cdf[k]; };
    for (int x = threadIdx.x; x < n; x += 256) row[x] = k10_centre(k10_closest(at, n, x), n);
}
void launch_invert(float *io, const double *sum, int n, int count, hipStream_t stream) {
    if (n <= 1024) hipLaunchKernelGGL(k10_invert<1024>, dim3(count), dim3(256), 0, stream, io, sum, n);
    else if (n <= 4096) hipLaunchKernelGGL(k10_invert<4096>, dim3(count), dim3(256), 0, stream, io, sum, n);
    else hipLaunchKernelGGL(k10_invert<K10_MAX_EDGE>, dim3(count), dim3(256), 0, stream, io, sum, n);
}

}  // namespace

// W, H: powers of two <= 16384 (rfx_set_environment's rule).  scratch: rfx_env_tables_scratch_bytes(H) bytes, K10Sums first.
hipError_t rfx_launch_env_tables(const float4 *env, int W, int H, int flipY, float *marginal, float *conditional, void *scratch, hipStream_t stream) {
    K10Sums *sums = (K10Sums *)scratch;
    double *last = (double *)(sums + 1), *rowsum = last + 1;
    int logW = 0;
    while ((1 << logW) < W) logW++;
    hipLaunchKernelGGL(k10_rows, dim3((H + K10_TILE - 1) / K10_TILE), dim3(K10_TILE), 0, stream, env, W, H, flipY, conditional, rowsum);
    hipLaunchKernelGGL(k10_total, dim3(1), dim3(K10_TOTAL_THREADS), 0, stream, env, W, logW, H, flipY, sums);
    hipLaunchKernelGGL(k10_marginal_chain, dim3(1), dim3(64), 0, stream, (const double *)rowsum, H, marginal, last);
    launch_invert(conditional, rowsum, W, H, stream);
    launch_invert(marginal, last, H, 1, stream);
    return hipGetLastError();
}
