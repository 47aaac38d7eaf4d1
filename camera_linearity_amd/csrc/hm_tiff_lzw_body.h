// hm_tiff_lzw_body.h - the TIFF LZW decoder as plain C++ over pointers, a table struct and an "emitter": the body of the device decoder
// of hm_tiff_device.hip. It includes nothing of HIP, so the same text compiles for the host, where a stand-alone program runs it under
// AddressSanitizer with an emitter that replays the wave's 64-lane copy serially (tools/lzw_body_check.cpp).
//
// Stream rules: exactly those of hm_tiff_lzw_decode (hm_tiff.hip) - MSB-first codes of 9..12 bits, Clear = 256, EOI = 257, early change,
// input that ends without EOI is accepted, a first code >= 256 after a Clear and code > next are HM_EINVAL, output past `cap` is HM_ESHAPE.
// As there, the string table holds (position, length) into the OUTPUT: emitting a code is one forward copy inside the output.
//
// Bounds, for any input: reads of src are at ip < src_len; table reads are at 258 <= code < next <= 4096 and table writes at next < 4096;
// an emission is refused (HM_ESHAPE) before it is made unless op + n <= cap, and its source [from, from + period) lies below op, so an
// emitter touches [0, cap) of its output only. Every iteration of the loop takes nbits >= 9 bits of input or leaves it, so the loop ends
// after at most 8 * src_len / 9 + 1 iterations.
#pragma once
#include <stdint.h>

#ifndef HM_LZW_HD
#if defined(__HIPCC__)
#define HM_LZW_HD __host__ __device__ inline
#else
#define HM_LZW_HD inline
#endif
#endif

namespace hm_lzw {

enum { kClear = 256, kEoi = 257, kFirst = 258, kMax = 4096 };
enum { kEinval = -1, kEshape = -6 };            // HM_EINVAL, HM_ESHAPE of hdrmerge.h (checked by a static_assert where both are visible)

struct Table {                                   // 24 KiB: one per decoder (on the device: one per wave, in LDS)
    uint32_t pos[kMax];
    uint16_t len[kMax];
};

// Emit is any type with
//   void literal(int64_t op, uint8_t byte)                          out[op] = byte
//   void copy(int64_t op, uint32_t from, uint32_t n, uint32_t period) out[op + k] = out[from + (k < period ? k : k - period)], k < n
// where n <= period + 1: period == n is a plain copy of a string that lies wholly below op; period == n - 1 is the KwKwK case, whose
// source ends where the destination starts, so its last byte is its own first byte (the string is periodic with the old string's length).
template <class Emit>
HM_LZW_HD int64_t decode(const uint8_t* src, int64_t src_len, int64_t cap, Table& t, Emit& out) {
    if (cap > 0xFFFFFFFFll) cap = 0xFFFFFFFFll;
    int nbits = 9, next = kFirst, old = -1;
    uint32_t old_pos = 0, old_len = 0;
    uint32_t acc = 0;
    int have = 0;
    int64_t ip = 0, op = 0;
    for (;;) {
        while (have < nbits && ip < src_len) { acc = (acc << 8) | src[ip++]; have += 8; }      // have <= 19 bits: no bit is lost from acc
        if (have < nbits) break;                                   // ran out of input without EOI: accept what we have
        const int code = static_cast<int>((acc >> (have - nbits)) & ((1u << nbits) - 1u));
        have -= nbits;
        if (code == kEoi) break;
        if (code == kClear) { nbits = 9; next = kFirst; old = -1; continue; }
        uint32_t from = 0, n = 1, period = 1;
        if (old < 0) {
            if (code >= 256) return kEinval;
        } else {
            if (code > next || next >= kMax + 1) return kEinval;
            if (code >= kFirst) {
                if (code >= kMax) return kEinval;
                if (code < next) { from = t.pos[code]; n = t.len[code]; period = n; }
                else { from = old_pos; n = old_len + 1; period = old_len; }                    // KwKwK
            }
            if (next < kMax) {
                t.pos[next] = old_pos;
                t.len[next] = static_cast<uint16_t>(old_len + 1);
                ++next;
            }
        }
        if (op + n > cap) return kEshape;
        if (code < 256) out.literal(op, static_cast<uint8_t>(code));
        else out.copy(op, from, n, period);
        old = code; old_pos = static_cast<uint32_t>(op); old_len = n;
        op += n;
        if (next + 1 >= (1 << nbits) && nbits < 12) ++nbits;       // early change
    }
    return op;
}

}  // namespace hm_lzw
