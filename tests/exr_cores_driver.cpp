// The stand-alone driver of tests/test_exr_cores_cpu.py: csrc/k9_rle.h and csrc/k9_pxr24.h on plain memory, no HIP and no Python in the process,
// so the sanitizers it is built with see every access.  Every buffer handed to them is a heap block of EXACTLY the size the format states.
//   driver <corpus> <results>
//   corpus : records  uint32 kind, then
//              kind 0 (RLE)    uint32 packed | uint32 raw | packed bytes
//              kind 1 (PXR24)  uint32 cols | uint32 rows | uint32 channels | one byte per channel (1: HALF, 0: FLOAT) | the inflated bytes
//                              (rows x cols x (2 per HALF + 3 per FLOAT channel))
//   results: records  kind 0   int32 code | uint64 iterations | raw bytes (code 0 only)
//                     kind 1   the raw block: per row and channel `cols` samples, 2 bytes for HALF and 4 for FLOAT
// The expander's loop counts one iteration through K9_ITER; a record whose count passes input bytes + output bytes aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t g_iters, g_cap;
#define K9_ITER()                                                                                   \
    do {                                                                                            \
        if (++g_iters > g_cap) { std::fprintf(stderr, "iteration cap %llu passed\n", (unsigned long long)g_cap); std::abort(); } \
    } while (0)
#include "k9_rle.h"
#include "k9_pxr24.h"

static uint8_t *block(size_t n) { return (uint8_t *)std::malloc(n ? n : 1); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t kind;
    while (std::fread(&kind, 4, 1, in) == 1) {
        if (kind == 0) {
            uint32_t head[2];
            if (std::fread(head, 4, 2, in) != 2) return 3;
            uint8_t *packed = block(head[0]), *raw = block(head[1]);
            if (head[0] && std::fread(packed, 1, head[0], in) != head[0]) return 3;
            // (a zero-size block may not be touched either: hand the expander the end of a one-byte block)
            g_iters = 0;
            g_cap = (uint64_t)head[0] + head[1];
            const int32_t code = k9_rle_host(head[0] ? packed : packed + 1, head[0], head[1] ? raw : raw + 1, head[1]);
            std::fwrite(&code, 4, 1, out);
            std::fwrite(&g_iters, 8, 1, out);
            if (code == K9_OK && head[1]) std::fwrite(raw, 1, head[1], out);
            std::free(packed);
            std::free(raw);
        } else if (kind == 1) {
            uint32_t head[3];
            if (std::fread(head, 4, 3, in) != 3) return 3;
            const uint32_t cols = head[0], rows = head[1], nchan = head[2];
            uint8_t *half = block(nchan);
            if (std::fread(half, 1, nchan, in) != nchan) return 3;
            size_t per_texel = 0;
            for (uint32_t c = 0; c < nchan; c++) per_texel += k9_pxr24_planes(half[c]);
            const size_t n = (size_t)rows * cols * per_texel;
            uint8_t *bytes = block(n);
            if (n && std::fread(bytes, 1, n, in) != n) return 3;
            uint32_t *sample = (uint32_t *)std::malloc(sizeof(uint32_t) * cols);
            const uint8_t *seg = bytes;
            for (uint32_t r = 0; r < rows; r++)
                for (uint32_t c = 0; c < nchan; c++) {
                    k9_pxr24_segment_host(seg, cols, half[c], sample);
                    seg += (size_t)cols * k9_pxr24_planes(half[c]);
                    for (uint32_t i = 0; i < cols; i++) {
                        const uint16_t h = (uint16_t)sample[i];
                        if (half[c]) std::fwrite(&h, 2, 1, out);
                        else std::fwrite(&sample[i], 4, 1, out);
                    }
                }
            if (seg != bytes + n) return 4;
            std::free(sample);
            std::free(bytes);
            std::free(half);
        } else
            return 3;
    }
    std::fclose(out);
    return 0;
}
