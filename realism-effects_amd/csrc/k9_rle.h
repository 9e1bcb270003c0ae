// K9 RLE core: OpenEXR's run-length code (what its RLE compression stores behind ZIP's predictor and byte split), with no HIP dependency, in the
// manner of k9_inflate.h: k9_exr_import.hip instantiates it with the wave-wide IO (one wave per chunk, the walk below wave-uniform, a fill or a
// literal stored by all lanes), a plain x86 program with K9RleHostIO (tests/test_exr_cores_cpu.py builds one under the sanitizers).
//
// The code: a signed count byte n, then n >= 0: ONE byte, which stands n + 1 times; n < 0: -n literal bytes.
// The safety rules, which hold for ANY input bytes:
//   reads    a count byte is read at i < in_len; a run's byte at i < in_len; a literal of m bytes only when i + m <= in_len (K9_E_RLE_INPUT);
//   writes   a run or literal of m bytes only when pos + m <= out_len, the block's raw size known from the file header (K9_E_RLE_OVERRUN);
//   loops    every iteration consumes at least two input bytes and produces at least one output byte (K9_ITER marks it: a test build counts).
// The IO concept is k9_inflate.h's `word` and `copy_in`, and
//   void fill(size_t pos, unsigned byte, unsigned len)      out[pos + k] = byte, k < len
#pragma once
#include "k9_inflate.h"

enum {
    K9_E_RLE_INPUT = 12,    // a run or a literal reaches past the packed bytes
    K9_E_RLE_OVERRUN = 13,  // more than out_len bytes
    K9_E_RLE_SHORT = 14     // the packed bytes end with fewer than out_len bytes
};

template <class IO>
K9_FN unsigned k9_rle_byte(IO &io, size_t i) { return (unsigned)(io.word(i >> 2) >> (8 * (unsigned)(i & 3))) & 255u; }

// Exactly in_len packed bytes -> exactly out_len bytes.  K9_OK or the first error; what out[] holds after an error is unspecified (but inside out_len).
template <class IO>
K9_FN int k9_rle_expand(IO &io, size_t in_len, size_t out_len) {
    size_t i = 0, pos = 0;
    while (i < in_len) {
        K9_ITER();
        const unsigned c = k9_rle_byte(io, i++);
        if (c & 128u) {
            const unsigned m = 256u - c;  // 1 .. 128 literal bytes
            if ((size_t)m > in_len - i) return K9_E_RLE_INPUT;
            if ((size_t)m > out_len - pos) return K9_E_RLE_OVERRUN;
            io.copy_in(pos, i, m);
            i += m;
            pos += m;
        } else {
            const unsigned m = c + 1u;  // 1 .. 128 times the next byte
            if (i >= in_len) return K9_E_RLE_INPUT;
            if ((size_t)m > out_len - pos) return K9_E_RLE_OVERRUN;
            io.fill(pos, k9_rle_byte(io, i++), m);
            pos += m;
        }
    }
    if (pos != out_len) return K9_E_RLE_SHORT;
    return K9_OK;
}

#ifndef K9_NO_HOST_IO
struct K9RleHostIO : K9HostIO {
    void fill(size_t pos, unsigned byte, unsigned len) {
        for (unsigned k = 0; k < len; k++) out[pos + k] = (uint8_t)byte;
    }
};
K9_FN int k9_rle_host(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len) {
    K9RleHostIO io;
    io.in = in; io.in_len = in_len; io.out = out;
    return k9_rle_expand(io, in_len, out_len);
}
#endif
