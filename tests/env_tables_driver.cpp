// tests/test_env_tables_cpu.py: K10's arithmetic (csrc/k10_env_tables.h k10_host_build — the statements the kernels run) on the host, built under
// AddressSanitizer + UBSan with buffers of exactly the sizes the library allocates.
//   env_tables_driver <in> <out>
// in:  cases back to back — int32 W, H, flipY, then W * H * 4 floats (level 0 as stored, row 0 = bottom)
// out: per case — H floats (marginalWeights), W * H floats (conditionalWeights), the double total, the float whole and decimal parts
#include <stdio.h>
#include <stdlib.h>

#include "k10_env_tables.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int head[3];
    while (fread(head, sizeof(int), 3, in) == 3) {
        const int W = head[0], H = head[1], flipY = head[2];
        if (W < 1 || H < 1 || W > K10_MAX_EDGE || H > K10_MAX_EDGE) return 3;
        const size_t n = (size_t)W * H;
        // (malloc, not vectors: the sanitizer's red zones sit right behind the last element)
        float *texels = (float *)malloc(n * 4 * sizeof(float)), *marginal = (float *)malloc(H * sizeof(float)), *conditional = (float *)malloc(n * sizeof(float));
        float *cdf = (float *)malloc((size_t)(W > H ? W : H) * sizeof(float));
        double *rowsum = (double *)malloc(H * sizeof(double));
        if (!texels || !marginal || !conditional || !cdf || !rowsum) return 4;
        if (fread(texels, sizeof(float), n * 4, in) != n * 4) return 3;
        K10Sums sums;
        k10_host_build(texels, W, H, flipY, marginal, conditional, cdf, rowsum, &sums);
        static_assert(sizeof(K10Sums) == 16, "the double, then the two floats");
        if (fwrite(marginal, sizeof(float), H, out) != (size_t)H || fwrite(conditional, sizeof(float), n, out) != n || fwrite(&sums, sizeof sums, 1, out) != 1) return 5;
        free(texels); free(marginal); free(conditional); free(cdf); free(rowsum);
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
