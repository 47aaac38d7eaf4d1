// hm_tiff_wide_enc_body.h - one row of a B,G,R(,A) image packed into the row of 2- or 4-byte samples a TIFF file stores, as plain C++ over
// pointers and a "lanes" object: the body of wide_pack_rows_kernel (hm_tiff_encode.hip) and of the host build's
// hm_tiff_encode_strips_wide (csrc_host/hm_host.cpp), in the manner of hm_tiff_wide_body.h, whose writing twin it is. It includes nothing
// of HIP, so the same text compiles for the host, where a stand-alone program runs it under AddressSanitizer and UBSan
// (tools/tiff_wide_enc_body_check.cpp).
//
// Per stored sample e of the row (pixel px = e / spp, file channel c = e % spp): read the source sample of the channel that lands there
// (R and B change places at sample granularity), turn it into the stored value - uint16 as it is, float32 bit for bit, float64 narrowed
// to float32 (narrow_f32) or float64 quantised to uint16 (quantize_u16) - take, under Predictor 2 (2-byte samples), the difference to
// the stored value of the same channel of the pixel on the left modulo 65536, which is read and converted again from the source (no
// scan; pixel 0 of a row is stored as it is), and store it sample-wide at out + e * B.
//
// The lanes walk the row's SAMPLES, not its pixels: lane l of a step stores sample e0 + l, so the 64 stores of a wave's step are one
// contiguous run of 64 * B bytes whatever the pixel size (6-, 8-, 12- and 16-byte pixels included), and its loads touch the same run of
// the source, permuted inside each pixel. A wave advances 64 pixels in spp such steps.
//
// Lanes is any type with
//   int width()                     samples per step: 64 for a wave, 1 for a serial loop
//   int lane()                      0 .. width() - 1
//
// Source kinds (HM_TIFF_SRC_* of hdrmerge.h): 0 uint16, 1 float32, 2 float64 -> float32, 3 float64 -> uint16. B is the STORED sample
// width: 2 for kinds 0 and 3, 4 for kinds 1 and 2 (the entry's rule function pairs them; a mismatched pair stores zeros and reads nothing).
//
// Bounds, for any input: a row reads source samples [0, npx * spp) of `src` - Predictor 2 reads sample at - spp only for px > 0, and
// at - spp >= 0 there - and writes bytes [0, npx * spp * B) of `out`, sample-wide. `out` must be a multiple of B (stored rows start on
// one in both the payload and the workspace: row_bytes is a multiple of B and the bases are 16-byte aligned) and `src` a multiple of its
// own sample size (the entry's HM_EALIGN rule). npx * spp * B < 2^31 (the entry's strip rule), so the sample index fits an int.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef HM_WIDE_HD
#if defined(__HIPCC__)
#define HM_WIDE_HD __host__ __device__ inline
#else
#define HM_WIDE_HD inline
#endif
#endif

namespace hm_tiff_wide_enc {

enum { kSrcU16 = 0, kSrcF32 = 1, kSrcF64AsF32 = 2, kSrcF64AsU16 = 3 };

template <int B> struct Stored;
template <> struct Stored<2> { typedef uint16_t type; };
template <> struct Stored<4> { typedef uint32_t type; };

// save_16bit's arithmetic for one sample, the 16-bit twin of hm_lzw_enc::quantize_u8: around((v / divisor) * max_dn) as uint16 - round
// half to even, wrap modulo 65536. Non-finite samples, and results of 2^63 or more in magnitude, give 0.
HM_WIDE_HD uint16_t quantize_u16(double v, double divisor, int max_dn) {
    const double r = rint((v / divisor) * static_cast<double>(max_dn));
    if (!(fabs(r) < 9223372036854775808.0)) return 0;           // NaN, inf, |r| >= 2^63
    return static_cast<uint16_t>(static_cast<uint64_t>(static_cast<int64_t>(r)) & 65535u);
}

// The bits of the float32 nearest to v, ties to even: ndarray.astype(np.float32). Doubles that round into the float32 subnormal range give
// the subnormal (both builds run with float32 denormals on: the device units are compiled without flush-to-zero),
// doubles past the float32 range give +-inf, a NaN gives a NaN.
HM_WIDE_HD uint32_t narrow_f32(double v) {
    const float f = static_cast<float>(v);
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    return bits;
}

HM_WIDE_HD int file_channel(int c, int spp) { return spp >= 3 ? (c < 3 ? 2 - c : c) : 0; }

// the stored value of source sample `at`
template <int B>
HM_WIDE_HD typename Stored<B>::type stored_sample(const void* src, int kind, int64_t at, double divisor, int max_dn) {
    typedef typename Stored<B>::type T;
    if (B == 2) {
        if (kind == kSrcU16) return static_cast<T>(static_cast<const uint16_t*>(src)[at]);
        if (kind == kSrcF64AsU16) return static_cast<T>(quantize_u16(static_cast<const double*>(src)[at], divisor, max_dn));
    } else {
        if (kind == kSrcF32) return static_cast<T>(static_cast<const uint32_t*>(src)[at]);
        if (kind == kSrcF64AsF32) return static_cast<T>(narrow_f32(static_cast<const double*>(src)[at]));
    }
    return 0;
}

// SPP at compile time: px = e / SPP is a multiplication
template <int B, int SPP, class Lanes>
HM_WIDE_HD void pack_row_spp(const void* src, int kind, double divisor, int max_dn, int npx, int predictor, uint8_t* out, Lanes& L) {
    typedef typename Stored<B>::type T;
    T* q = reinterpret_cast<T*>(out);
    const int n = npx * SPP;
    for (int e0 = 0; e0 < n; e0 += L.width()) {
        const int e = e0 + L.lane();
        if (e >= n) continue;
        const int px = e / SPP;
        const int64_t at = static_cast<int64_t>(px) * SPP + file_channel(e - px * SPP, SPP);
        T v = stored_sample<B>(src, kind, at, divisor, max_dn);
        if (B == 2 && predictor == 2 && px > 0) v = static_cast<T>(v - stored_sample<B>(src, kind, at - SPP, divisor, max_dn));
        q[e] = v;
    }
}

// src: the row's first source sample; spp: 1, 3 or 4; predictor 2 is read with B == 2 only (the entry refuses it for float32 output)
template <int B, class Lanes>
HM_WIDE_HD void pack_row(const void* src, int kind, double divisor, int max_dn, int npx, int spp, int predictor, uint8_t* out, Lanes& L) {
    if (spp == 1) pack_row_spp<B, 1>(src, kind, divisor, max_dn, npx, predictor, out, L);
    else if (spp == 3) pack_row_spp<B, 3>(src, kind, divisor, max_dn, npx, predictor, out, L);
    else if (spp == 4) pack_row_spp<B, 4>(src, kind, divisor, max_dn, npx, predictor, out, L);
}

}  // namespace hm_tiff_wide_enc
