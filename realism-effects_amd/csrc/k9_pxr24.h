// K9 PXR24 arithmetic: what follows the inflate of a PXR24 chunk, with no HIP dependency (k9_exr_import.hip's k9_exr_planes runs it with one lane
// per sample; tests/test_exr_cores_cpu.py runs k9_pxr24_segment_host, the same steps over an array of 64 lanes, under the sanitizers).
//
// The inflated bytes are, per row and channel in file order, k byte planes of `cols` bytes each, most significant first (HALF: k = 2; FLOAT: k = 3,
// the float cut to its upper 24 bits by the writer), holding the difference of every sample to its left neighbour in the block's row (the first
// one: to 0).  A sample is the prefix sum of the differences along its row segment modulo 2^(8k): summed in uint32 — whose wrap at 2^32 is a wrap
// modulo 2^(8k) too — and masked.  HALF: the low 16 bits are the half; FLOAT: the 24 bits << 8 are the float.
// The scan: 64 samples per step, one per lane — the log-step inclusive scan below (lane l adds the value of lane l - off for off = 1, 2 .. 32) —
// plus the carry, the sum of every step before: lane 63's result.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef K9_FN
#define K9_FN static inline
#endif

K9_FN unsigned k9_pxr24_planes(int half) { return half ? 2u : 3u; }
// the difference stored for sample i of a row segment whose k planes of `cols` bytes start at seg; 0 for i >= cols (a lane past the row's end)
K9_FN uint32_t k9_pxr24_diff(const uint8_t *seg, unsigned cols, unsigned k, unsigned i) {
    if (i >= cols) return 0u;
    uint32_t d = 0u;
    for (unsigned b = 0; b < k; b++) d = (d << 8) | seg[(size_t)b * cols + i];
    return d;
}
// one step of the inclusive scan: `below` is the running value of lane `lane - off` (anything for lane < off)
K9_FN uint32_t k9_pxr24_scan_step(int lane, int off, uint32_t own, uint32_t below) { return lane >= off ? own + below : own; }
// the sample's bits in its plane from the prefix sum of the differences up to it
K9_FN uint32_t k9_pxr24_bits(uint32_t sum, int half) { return half ? (sum & 0xffffu) : ((sum & 0xffffffu) << 8); }

#ifndef K9_NO_HOST_IO
// one (row, channel) segment as the device walks it: out[i] = the bits of sample i (a uint16 value for HALF, a float's 32 bits otherwise)
K9_FN void k9_pxr24_segment_host(const uint8_t *seg, unsigned cols, int half, uint32_t *out) {
    const unsigned k = k9_pxr24_planes(half);
    uint32_t carry = 0u;
    for (unsigned base = 0; base < cols; base += 64u) {
        uint32_t s[64], t[64];
        for (int l = 0; l < 64; l++) s[l] = k9_pxr24_diff(seg, cols, k, base + (unsigned)l);
        for (int off = 1; off < 64; off <<= 1) {
            for (int l = 0; l < 64; l++) t[l] = k9_pxr24_scan_step(l, off, s[l], l >= off ? s[l - off] : 0u);
            for (int l = 0; l < 64; l++) s[l] = t[l];
        }
        for (int l = 0; l < 64; l++) {
            s[l] += carry;
            if (base + (unsigned)l < cols) out[base + (unsigned)l] = k9_pxr24_bits(s[l], half);
        }
        carry = s[63];
    }
}
#endif
