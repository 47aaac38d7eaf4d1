// hm_tiff_wide_body.h - one row of 2-, 4- or 8-byte TIFF samples turned into the row cv.imread returns, as plain C++ over pointers and a
// "lanes" object: the body of wide_rows_kernel (hm_tiff_device.hip) and of the host build's hm_tiff_decode_strips_wide
// (csrc_host/hm_host.cpp), in the manner of hm_tiff_lzw_body.h. It includes nothing of HIP, so the same text compiles for the host,
// where a stand-alone program runs it under AddressSanitizer and UBSan (tools/tiff_wide_body_check.cpp).
//
// Per pixel: load the samples (sample-wide where the row starts on a sample boundary, else unaligned-safe), byte-reverse them for a
// big-endian file, undo Predictor 2 on the SWAPPED values modulo 65536 (2-byte samples), swap R and B at sample granularity, and
// store sample-wide - or, for cv.IMREAD_COLOR on 2-byte samples, store value >> 8 as uint8 with grey replicated and alpha dropped.
//
// Lanes is any type with
//   int width()                     pixels per step: 64 for a wave, 1 for a serial loop
//   int lane()                      0 .. width() - 1
//   uint32_t scan_add(uint32_t x)   the inclusive sum of x over lanes 0 .. lane()      (serial: x)
//   uint32_t last(uint32_t x)       x of lane width() - 1                              (serial: x)
// Every lane of a step calls scan_add / last together: the loop bounds below are the same for all lanes.
//
// Bounds, for any input: reads of `in` are at [0, npx * spp * B), writes of `out` at [0, npx * ospp * B) (color_mode 0) or
// [0, npx * 3) (color_mode 1). `out` must be aligned to B in color_mode 0 (the entry's HM_EALIGN rule); `in` may have any alignment.
#pragma once
#include <stdint.h>

#ifndef HM_WIDE_HD
#if defined(__HIPCC__)
#define HM_WIDE_HD __host__ __device__ inline
#else
#define HM_WIDE_HD inline
#endif
#endif
#if defined(__clang__)
#define HM_WIDE_UNROLL _Pragma("unroll")
#else
#define HM_WIDE_UNROLL
#endif

namespace hm_tiff_wide {

template <int B> struct Sample;
template <> struct Sample<2> { typedef uint16_t type; };
template <> struct Sample<4> { typedef uint32_t type; };
template <> struct Sample<8> { typedef uint64_t type; };

HM_WIDE_HD uint16_t byte_reverse(uint16_t v) { return __builtin_bswap16(v); }
HM_WIDE_HD uint32_t byte_reverse(uint32_t v) { return __builtin_bswap32(v); }
HM_WIDE_HD uint64_t byte_reverse(uint64_t v) { return __builtin_bswap64(v); }

// the sample at p in the machine's (little-endian) order; `aligned`: p is a multiple of B
template <int B>
HM_WIDE_HD typename Sample<B>::type load_sample(const uint8_t* p, bool aligned) {
    typedef typename Sample<B>::type T;
    if (aligned) return *reinterpret_cast<const T*>(p);
    T v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    for (int k = 0; k < B; ++k) v = static_cast<T>(v | (static_cast<T>(p[k]) << (8 * k)));     // a strip at an odd file offset: byte by byte
#else
    __builtin_memcpy(&v, p, B);
#endif
    return v;
}

// cv.imread's 8-bit conversion of a 16-bit sample
HM_WIDE_HD uint8_t to_u8(uint16_t v) { return static_cast<uint8_t>(v >> 8); }

// spp: 1, 3 or 4 stored samples per pixel; predictor 2 and color_mode 1 are read with B == 2 only (the entry refuses the others)
template <int B, class Lanes>
HM_WIDE_HD void finish_row(const uint8_t* in, int npx, int spp, bool big_endian, int predictor, int color_mode, uint8_t* out, Lanes& L) {
    typedef typename Sample<B>::type T;
    const bool aligned = (reinterpret_cast<uintptr_t>(in) & (B - 1)) == 0;
    const int ospp = color_mode == 1 ? 3 : spp;
    uint32_t carry[4] = {0, 0, 0, 0};
    for (int x0 = 0; x0 < npx; x0 += L.width()) {
        const int px = x0 + L.lane();
        const bool act = px < npx;
        T v[4] = {0, 0, 0, 0};
HM_WIDE_UNROLL
        for (int c = 0; c < 4; ++c)
            if (c < spp && act) {
                const T raw = load_sample<B>(in + (static_cast<int64_t>(px) * spp + c) * B, aligned);
                v[c] = big_endian ? byte_reverse(raw) : raw;
            }
        if (B == 2 && predictor == 2) {
HM_WIDE_UNROLL
            for (int c = 0; c < 4; ++c)
                if (c < spp) {                         // the same for every lane
                    const uint32_t x = L.scan_add(static_cast<uint32_t>(v[c])) + carry[c];      // < 65 * 65536: no bit is lost
                    carry[c] = L.last(x) & 0xFFFFu;    // lanes past the row added 0: the last lane holds the running sum
                    v[c] = static_cast<T>(x);          // modulo 65536
                }
        }
        // R and B change places, grey is replicated (constant indices: v stays in registers)
        if (act && B == 2 && color_mode == 1) {
            uint8_t* q = out + static_cast<int64_t>(px) * 3;
HM_WIDE_UNROLL
            for (int c = 0; c < 3; ++c) q[c] = to_u8(static_cast<uint16_t>(spp == 1 ? v[0] : v[2 - c]));
        } else if (act) {
            T* q = reinterpret_cast<T*>(out) + static_cast<int64_t>(px) * ospp;
HM_WIDE_UNROLL
            for (int c = 0; c < 4; ++c)
                if (c < ospp) q[c] = spp == 1 ? v[0] : v[c < 3 ? 2 - c : c];
        }
    }
}

}  // namespace hm_tiff_wide
