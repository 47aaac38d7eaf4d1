// hm_tiff_lzw_enc_body.h - the TIFF LZW encoder as plain C++ over pointers, a dictionary struct and an "ops" object: the body of the device
// encoder of hm_tiff_encode.hip and of the host build's hm_tiff_encode_strips. The writing twin of hm_tiff_lzw_body.h: it includes nothing
// of HIP, so the same text compiles for the host, where a stand-alone program runs it under AddressSanitizer with ops that replay the
// wave's 64-slot probe and its 64-lane word staging serially (tools/lzw_enc_body_check.cpp).
//
// Stream rules: those of lzw_encode(data, eoi=True) in tests/test_tiff_device_host.py, byte for byte - MSB-first codes of 9..12 bits,
// a Clear (256) first, the greedy longest match, a new entry after every emitted code, the early change (next >= 1 << nbits), a Clear and
// an empty table when next reaches 4094, EOI (257) after the last code (which still counts as an entry for the width of EOI), the final
// partial byte left-aligned and zero-padded; an empty input gives Clear, EOI.
//
// The dictionary is an open-addressed table of kSlots 32-bit words keyed by (prefix code, byte): word = key << 12 | code with
// key = prefix << 8 | byte < 2^20 and 258 <= code < 4094, so a used word is never 0 and 0 means free. A key lives at the first free slot
// of the probe sequence start(key), start + 1, ... (mod kSlots) at the time it was inserted, and nothing is removed before a Clear empties
// the whole table: a lookup that walks the sequence may stop at the first free slot. Ops::probe examines one window of kWindow consecutive
// slots (on the device: one slot per lane, one LDS round trip).
//
// Size bound. Every data code stands for at least one input byte, so n bytes give at most n data codes of at most 12 bits: 12 n bits. A
// Clear after the first is emitted when next reaches 4094, that is after 4094 - 258 = 3836 data codes: at most floor(n / 3836) of them,
// 12 bits each. The first Clear has 9 bits, EOI at most 12, the padding at most 7. In bytes that is at most
//   1.5 n + 1.5 floor(n / 3836) + 28 / 8 <= (3 n + 1) / 2 + floor(n / 2048) + 8 = bound(n)
// in integer arithmetic, because 1.5 n / 3836 = n / 2557.3 <= n / 2048 - 1 + 4.5 for every n >= 0.
//
// Bounds, for any input and any cap: reads of src are at i < n through Ops::byte; dictionary reads are at slots < kSlots (Ops::probe
// reduces modulo kSlots) and the one dictionary write per emitted code goes to a slot Ops::probe reported free, < kSlots; at most 3836
// of the kSlots = 8192 slots are used between two Clears, so every probe sequence meets a free slot and the window loop, which is also
// cut off after kSlots / kWindow windows, ends. A code is refused (kEshape) before it is put unless the stream with it still fits in cap
// bytes, and the stream leaves in whole 32-bit words at word index w with 4 w < cap rounded up to 4: Ops::word touches
// [0, round_up(cap, 4)) of its output only. The loop takes one input byte per iteration, so it ends after n iterations.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef HM_LZW_HD
#if defined(__HIPCC__)
#define HM_LZW_HD __host__ __device__ inline
#else
#define HM_LZW_HD inline
#endif
#endif

namespace hm_lzw_enc {

enum { kClear = 256, kEoi = 257, kFirst = 258, kFull = 4094 };
enum { kSlots = 8192, kWindow = 64 };
enum { kEshape = -6 };                           // HM_ESHAPE of hdrmerge.h (checked by a static_assert where both are visible)
constexpr int64_t kMaxInput = (1ll << 31) - 1;   // a strip: 1 .. 2^31 - 1 bytes

struct alignas(16) Dict {                        // 32 KiB: one per encoder (on the device: one per wave, in LDS, emptied with 16-byte stores)
    uint32_t slot[kSlots];
};

HM_LZW_HD int64_t bound(int64_t n) { return (3 * n + 1) / 2 + n / 2048 + 8; }        // 0 <= n <= kMaxInput: no overflow

HM_LZW_HD uint32_t start_of(uint32_t key) { return (key * 2654435761u) >> 19; }      // 13 bits: < kSlots

HM_LZW_HD uint32_t to_stream_order(uint32_t w) {                                     // MSB-first bits -> the little-endian word that holds them
    return (w >> 24) | ((w >> 8) & 0xFF00u) | ((w << 8) & 0xFF0000u) | (w << 24);
}

// save_8bit's arithmetic for one sample: around((v / divisor) * 255) as uint8 - round half to even, wrap modulo 256 (the convention of
// hm_linearize_f64's index). Non-finite samples, and results too large for an int64, give 0.
HM_LZW_HD uint8_t quantize_u8(double v, double divisor) {
    const double r = rint((v / divisor) * 255.0);
    if (!(fabs(r) < 9.0e18)) return 0;           // NaN, inf, |r| >= 2^63
    return static_cast<uint8_t>(static_cast<uint64_t>(static_cast<int64_t>(r)) & 255u);
}

// Ops is any type with
//   uint8_t byte(const uint8_t* src, int64_t i)                 src[i], 0 <= i < n (the device fetches 256 bytes at a time)
//   void clear(Dict& d)                                         every slot = 0
//   int probe(const Dict& d, uint32_t start, uint32_t key, uint32_t* free_slot)
//                                                               looks at d.slot[(start + l) % kSlots], l < kWindow, in that order:
//                                                               the code (>= kFirst) of the first slot that holds `key`, if that comes
//                                                               before the first free slot; else -1 and *free_slot = the first free
//                                                               slot's index; else (no free slot, no match) -2
//   void insert(Dict& d, uint32_t slot, uint32_t word)          d.slot[slot] = word, visible to the next probe
//   void word(uint8_t* out, int64_t w, uint32_t v)              the 4 bytes of v (little-endian) to out + 4 w; w rises by 1 per call
//   void flush(uint8_t* out, int64_t n_words)                   after the last word: everything staged has reached `out`
//
// find: the lookup of `key` over as many windows as it takes - the code (>= kFirst) if the table holds the key; -1 and *free_slot = the
// slot where it belongs if it does not; -2 if kSlots / kWindow windows hold neither (a full table, which encode never builds).
template <class Ops>
HM_LZW_HD int find(const Dict& d, uint32_t key, Ops& ops, uint32_t* free_slot) {
    uint32_t start = start_of(key);
    int r = -2;
    for (int win = 0; win < kSlots / kWindow && r == -2; ++win, start = (start + kWindow) & (kSlots - 1))
        r = ops.probe(d, start, key, free_slot);
    return r;
}

// Returns the stream's length in bytes, or kEshape if it would pass `cap`.
template <class Ops>
HM_LZW_HD int64_t encode(const uint8_t* src, int64_t n, uint8_t* out, int64_t cap, Dict& d, Ops& ops) {
    int nbits = 9, next = kFirst, have = 0;      // have < 32 pending bits in the low end of acc
    uint64_t acc = 0;
    int64_t bits = 0, w = 0;
    const int64_t cap_bits = cap > (1ll << 40) ? (8ll << 40) : cap * 8;
    if (n < 0) n = 0;
#define HM_LZW_PUT(code)                                                                                   \
    do {                                                                                                   \
        if (bits + nbits > cap_bits) return kEshape;                                                       \
        acc = (acc << nbits) | static_cast<uint32_t>(code);                                                \
        have += nbits;                                                                                     \
        bits += nbits;                                                                                     \
        if (have >= 32) {                                                                                  \
            have -= 32;                                                                                    \
            ops.word(out, w++, to_stream_order(static_cast<uint32_t>(acc >> have)));                       \
        }                                                                                                  \
    } while (0)
    ops.clear(d);
    HM_LZW_PUT(kClear);
    int cur = -1;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t b = ops.byte(src, i);
        if (cur < 0) { cur = static_cast<int>(b); continue; }
        const uint32_t key = (static_cast<uint32_t>(cur) << 8) | b;
        uint32_t free_slot = 0;
        const int r = find(d, key, ops, &free_slot);
        if (r >= 0) { cur = r; continue; }
        HM_LZW_PUT(cur);
        if (r == -1 && next < kFull - 1) ops.insert(d, free_slot, (key << 12) | static_cast<uint32_t>(next));   // entry 4093 would be cleared at once
        ++next;
        if (next >= (1 << nbits) && nbits < 12) ++nbits;           // early change
        if (next >= kFull) {
            HM_LZW_PUT(kClear);
            ops.clear(d);
            nbits = 9;
            next = kFirst;
        }
        cur = static_cast<int>(b);
    }
    if (cur >= 0) {
        HM_LZW_PUT(cur);
        ++next;
        if (next >= (1 << nbits) && nbits < 12) ++nbits;
    }
    HM_LZW_PUT(kEoi);
    if (have > 0) {
        if (bits + (8 - (bits & 7)) % 8 > cap_bits) return kEshape;
        ops.word(out, w++, to_stream_order(static_cast<uint32_t>(acc << (32 - have))));
    }
#undef HM_LZW_PUT
    ops.flush(out, w);
    return (bits + 7) / 8;
}

// The same ops with no lanes: one slot and one word at a time. The host build's encoder; the reference of the lane replays.
struct SerialOps {
    uint8_t byte(const uint8_t* src, int64_t i) { return src[i]; }
    void clear(Dict& d) { for (int k = 0; k < kSlots; ++k) d.slot[k] = 0; }
    int probe(const Dict& d, uint32_t start, uint32_t key, uint32_t* free_slot) {
        for (uint32_t l = 0; l < kWindow; ++l) {
            const uint32_t at = (start + l) & (kSlots - 1), e = d.slot[at];
            if (e == 0) { *free_slot = at; return -1; }
            if ((e >> 12) == key) return static_cast<int>(e & 0xFFFu);
        }
        return -2;
    }
    void insert(Dict& d, uint32_t slot, uint32_t word) { d.slot[slot] = word; }
    void word(uint8_t* out, int64_t w, uint32_t v) {
        uint8_t* p = out + 4 * w;
        p[0] = static_cast<uint8_t>(v); p[1] = static_cast<uint8_t>(v >> 8); p[2] = static_cast<uint8_t>(v >> 16); p[3] = static_cast<uint8_t>(v >> 24);
    }
    void flush(uint8_t*, int64_t) {}
};

}  // namespace hm_lzw_enc
