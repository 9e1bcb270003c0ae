// The stand-alone driver of tests/test_inflate_core_cpu.py: csrc/k9_inflate.h on plain memory, no HIP and no Python in the process, so the
// sanitizers it is built with see every access of the decoder.  Input and output buffers are heap blocks of EXACTLY the packed and the raw size.
//   driver <corpus> <results>
//   corpus : records  uint32 packed | uint32 raw | packed bytes
//   results: records  int32 code | uint64 iterations | raw bytes (code 0 only)
// Every loop of the decoder counts one iteration through K9_ITER; a record whose count passes input bits + output bytes aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t g_iters, g_cap;
#define K9_ITER()                                                                                   \
    do {                                                                                            \
        if (++g_iters > g_cap) { std::fprintf(stderr, "iteration cap %llu passed\n", (unsigned long long)g_cap); std::abort(); } \
    } while (0)
#include "k9_inflate.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[2];
    while (std::fread(head, 4, 2, in) == 2) {
        uint8_t *packed = (uint8_t *)std::malloc(head[0] ? head[0] : 1), *raw = (uint8_t *)std::malloc(head[1] ? head[1] : 1);
        if (head[0] && std::fread(packed, 1, head[0], in) != head[0]) return 3;
        // (a zero-size block may not be touched either: hand the decoder the end of a one-byte block)
        const uint8_t *p = head[0] ? packed : packed + 1;
        uint8_t *r = head[1] ? raw : raw + 1;
        g_iters = 0;
        g_cap = 8ull * head[0] + head[1];
        const int32_t code = k9_inflate_host(p, head[0], r, head[1]);
        std::fwrite(&code, 4, 1, out);
        std::fwrite(&g_iters, 8, 1, out);
        if (code == K9_OK && head[1]) std::fwrite(raw, 1, head[1], out);
        std::free(packed);
        std::free(raw);
    }
    std::fclose(out);
    return 0;
}
