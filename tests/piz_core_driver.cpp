// The stand-alone driver of tests/test_piz_core_cpu.py: csrc/k9_piz.h on plain memory, no HIP and no Python in the process, so the sanitizers it is
// built with see every access.  Every buffer handed to the cores is a heap block of EXACTLY the size the format or the header states.
//   driver <corpus> <results>
//   corpus : records  uint32 kind, then
//              kind 0 (Huffman block)  uint32 nwords | uint32 bytes | the Huffman block
//              kind 1 (wavelet)        uint32 nx | uint32 ny | uint32 14-bit arithmetic (1) or modulo-16-bit (0) | nx x ny words
//              kind 2 (PIZ block)      uint32 cols | uint32 rows | uint32 channels | one byte per channel (1: HALF, 0: FLOAT) | uint32 bytes | the block
//   results: records  kind 0   int32 code | uint64 iterations | the words (code 0 only)
//                     kind 1   the decoded words
//                     kind 2   int32 code | uint64 iterations | int32 mx | the raw block, scanline-interleaved (code 0 only)
// Every input-dependent loop counts one iteration through K9_ITER; a record whose count passes input bits + output words aborts the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t g_iters, g_cap;
#define K9_ITER()                                                                                   \
    do {                                                                                            \
        if (++g_iters > g_cap) { std::fprintf(stderr, "iteration cap %llu passed\n", (unsigned long long)g_cap); std::abort(); } \
    } while (0)
#include "k9_piz.h"

static uint8_t *block(size_t n) { return (uint8_t *)std::malloc(n ? n : 1); }

// the Huffman block at [at, at + len) of `in` -> words[nwords]
static int huffman(const uint8_t *in, size_t in_len, size_t at, size_t len, uint16_t *words, size_t nwords) {
    K9PizHostIO *io = new K9PizHostIO;
    io->in = in; io->in_len = in_len; io->out = words;
    io->symbols = (uint16_t *)std::malloc(sizeof(uint16_t) * K9_PIZ_ENCSIZE);
    const int code = k9_piz_huf_decode(*io, at, len, nwords);
    std::free(io->symbols);
    delete io;
    return code;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t kind;
    while (std::fread(&kind, 4, 1, in) == 1) {
        if (kind == 0) {
            uint32_t head[2];
            if (std::fread(head, 4, 2, in) != 2) return 3;
            uint8_t *packed = block(head[1]);
            uint16_t *words = (uint16_t *)block(2 * (size_t)head[0]);
            if (head[1] && std::fread(packed, 1, head[1], in) != head[1]) return 3;
            g_iters = 0;
            g_cap = 8ull * head[1] + head[0];
            const int32_t code = huffman(head[1] ? packed : packed + 1, head[1], 0, head[1], words, head[0]);
            std::fwrite(&code, 4, 1, out);
            std::fwrite(&g_iters, 8, 1, out);
            if (code == K9_OK && head[0]) std::fwrite(words, 2, head[0], out);
            std::free(packed);
            std::free(words);
        } else if (kind == 1) {
            uint32_t head[3];
            if (std::fread(head, 4, 3, in) != 3) return 3;
            const size_t n = (size_t)head[0] * head[1];
            uint16_t *words = (uint16_t *)block(2 * n);
            if (n && std::fread(words, 2, n, in) != n) return 3;
            k9_piz_plane_host(words, (int)head[0], (int)head[1], 1, (int)head[0], head[2] != 0);
            if (n) std::fwrite(words, 2, n, out);
            std::free(words);
        } else if (kind == 2) {
            uint32_t head[3], bytes;
            if (std::fread(head, 4, 3, in) != 3) return 3;
            const uint32_t cols = head[0], rows = head[1], nchan = head[2];
            uint8_t *half = block(nchan);
            if (std::fread(half, 1, nchan, in) != nchan || std::fread(&bytes, 4, 1, in) != 1) return 3;
            uint8_t *packed = block(bytes);
            if (bytes && std::fread(packed, 1, bytes, in) != bytes) return 3;
            size_t per_texel = 0;  // words
            for (uint32_t c = 0; c < nchan; c++) per_texel += half[c] ? 1 : 2;
            const size_t nwords = (size_t)rows * cols * per_texel;
            uint16_t *words = (uint16_t *)block(2 * nwords), *raw = (uint16_t *)block(2 * nwords), *rev = (uint16_t *)block(K9_PIZ_REV_BYTES);
            g_iters = 0;
            g_cap = 8ull * bytes + nwords;
            int32_t code, mx = -1;
            {
                K9PizHostIO *io = new K9PizHostIO;
                io->in = bytes ? packed : packed + 1; io->in_len = bytes; io->out = nullptr; io->symbols = nullptr;
                K9PizHead hd;
                code = k9_piz_head(*io, bytes, &hd);
                delete io;
                if (!code) {
                    // the reverse lookup table as the wave builds it: a count per lane, then every lane writes behind the lanes before it
                    // (the bitmap bytes: their own exact-sized block)
                    const size_t bm_n = hd.bm_min <= hd.bm_max ? hd.bm_max - hd.bm_min + 1u : 0u;
                    uint8_t *bm = block(bm_n);
                    if (bm_n) std::memcpy(bm, packed + 4, bm_n);
                    unsigned cnt[64], total = 0;
                    for (int l = 0; l < 64; l++) total += cnt[l] = k9_piz_rev_count(bm_n ? bm : bm + 1, hd.bm_min, hd.bm_max, l);
                    unsigned base = 0;
                    for (int l = 0; l < 64; l++) {
                        k9_piz_rev_write(bm_n ? bm : bm + 1, hd.bm_min, hd.bm_max, l, base, total, rev);
                        base += cnt[l];
                    }
                    std::free(bm);
                    mx = (int32_t)total - 1;
                    code = huffman(packed, bytes, hd.huf_at, hd.huf_len, words, nwords);
                }
            }
            if (!code) {
                // per channel: its one or two word planes through the cells, the lookup, and the samples into the scanline-interleaved block
                size_t before = 0;  // words per texel of the channels before
                for (uint32_t c = 0; c < nchan; c++) {
                    const int size = half[c] ? 1 : 2;
                    uint16_t *plane = words + (size_t)rows * cols * before;
                    for (int j = 0; j < size; j++) k9_piz_plane_host(plane + j, (int)cols, (int)rows, size, (int)cols * size, mx < (1 << 14));
                    for (uint32_t r = 0; r < rows; r++)
                        for (uint32_t k = 0; k < cols * (uint32_t)size; k++)
                            raw[(size_t)r * cols * per_texel + (size_t)cols * before + k] = rev[plane[(size_t)r * cols * size + k]];
                    before += (size_t)size;
                }
            }
            std::fwrite(&code, 4, 1, out);
            std::fwrite(&g_iters, 8, 1, out);
            std::fwrite(&mx, 4, 1, out);
            if (code == K9_OK && nwords) std::fwrite(raw, 2, nwords, out);
            std::free(half); std::free(packed); std::free(words); std::free(raw); std::free(rev);
        } else
            return 3;
    }
    std::fclose(out);
    return 0;
}
