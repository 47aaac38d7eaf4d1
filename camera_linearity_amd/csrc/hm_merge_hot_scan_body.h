// hm_merge_hot_scan_body.h - the body of the hot-pixel scan, once for both dark-map DN widths. Not a header of declarations: this text is
// included as the whole body of merge_scan_hot (hm_merge_hot.hip) and of merge_u16_scan_hot (hm_merge_u16_hot.hip), after
// hm_merge_hot_scan.h.
// In scope at the point of inclusion: `a` (the MergeK arguments), `ws`, `capacity`, the type D of a dark DN (uint8_t / uint16_t) and `mask`
// (the literal 255 / 2^bit_depth - 1): frame i is hot at an element iff (dark DN & mask) >= dark_min[i].
// Included, not called (hm_de_select_body.h's reason): as an inlined function template the same text moved the 8-bit scan's register
// allocation (100 VGPRs against 99, other instruction order); included, merge_scan_hot compiles to the instructions it had when it stood
// alone (tools/kernel_asm_diff.py).
//
// The scan alone. A lane's chunk is 16 consecutive elements (sizeof(D) aligned 16-byte loads per map), a wave's span 1024 elements; a wave
// scans kScanRound consecutive spans per round (the round's loads of a map issued together), a workgroup's 16 waves 64 consecutive spans
// = 65 536 elements (a few image rows: what lands next to each other in the queue shares its neighbour rows, which the patch kernel then
// finds in the cache). The waves add up their counts through LDS and ONE atomic add per workgroup and round reserves its piece of the
// queue (an atomic per wave and span serialised on the counter: 49 000 returning atomics on one address took 365 us at a density of 1e-3,
// profiles/r03c_hot_trace.txt). Every wave runs the same number of rounds (barriers). The order of the pieces in the queue depends on the
// order of the atomics; the patched image does not (every queued element is recomputed independently).
    constexpr int L = sizeof(D);                                            // 16-byte loads per chunk
    uint32_t* const table = ws + kHotQueueHeader;
    uint32_t* const queue = table + 2u * hot_piece_slots(a.n_elems);
    __shared__ uint32_t s_tot[kScanBlock / 64];
    __shared__ uint32_t s_base, s_ok;
    constexpr uint32_t WPB = kScanBlock / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_chunks = (a.n_elems + 15) / 16;
    const int64_t n_spans = (n_chunks + 63) / 64;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * WPB;
    const int64_t wave_global = static_cast<int64_t>(blockIdx.x) * WPB + wave;
    const int64_t rounds = (n_spans + n_waves * kScanRound - 1) / (n_waves * kScanRound);
    // distinct (map, threshold) pairs: bit i set = frame i's map is read (wave-uniform, once); `wide` = every such map can be read with
    // aligned 16-byte loads (its pointer + in_off is 16-byte aligned: elem0 and the chunk starts are multiples of 16 elements)
    uint32_t distinct = 0;
    bool wide = (a.elem0 & 15) == 0;
    for (int i = 0; i < a.n_frames; ++i) {
        const D* d = dark_as<D>(a, i);
        if (!d) continue;
        HM_SKIP_REPEATED_DARK(a, i, d)
        distinct |= 1u << i;
        wide = wide && (reinterpret_cast<uintptr_t>(d + a.in_off) & 15) == 0;
    }
    const int64_t n_full = a.n_elems / 16;                                  // whole 16-element chunks; a last partial one goes the slow way
    for (int64_t r = 0; r < rounds; ++r) {
        uint32_t hb[kScanRound];
        uint32_t mine = 0;
        if (wide) {
            // no load sits behind a lane-dependent branch: the round's loads of a map are issued back to back (a chunk past the end
            // re-reads chunk 0 and is masked afterwards), then compared
            int64_t off[kScanRound];
            bool valid[kScanRound];
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                valid[k] = chunk < n_full;
                off[k] = a.in_off + a.elem0 + (valid[k] ? chunk : 0) * 16;   // in elements; < in_off + elem0 + n_full * 16 <= the tile's end
                hb[k] = 0;
            }
            if (n_full > 0) {
                for (uint32_t left = distinct; left; left &= left - 1) {    // wave-uniform loop over the distinct maps
                    const int i = __builtin_amdgcn_readfirstlane(__ffs(static_cast<int>(left)) - 1);
                    const D* d = dark_as<D>(a, i);
                    const uint32_t thr = static_cast<uint32_t>(a.dark_min[i]);
                    u32x4 v[kScanRound][L];
#pragma unroll
                    for (int k = 0; k < kScanRound; ++k)
#pragma unroll
                        for (int l = 0; l < L; ++l) v[k][l] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(d + off[k]) + l);
#pragma unroll
                    for (int k = 0; k < kScanRound; ++k) {
                        uint32_t w[4 * L];
#pragma unroll
                        for (int l = 0; l < L; ++l) { w[4 * l] = v[k][l].x; w[4 * l + 1] = v[k][l].y; w[4 * l + 2] = v[k][l].z; w[4 * l + 3] = v[k][l].w; }
                        constexpr int PER = 4 / sizeof(D);
#pragma unroll
                        for (int b = 0; b < 16; ++b) hb[k] |= (((w[b / PER] >> (8 * sizeof(D) * (b % PER))) & mask) >= thr) ? (1u << b) : 0u;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                if (!valid[k]) hb[k] = 0;
                if (chunk == n_full && chunk < n_chunks)                    // the tile's last, partial chunk (one lane of one wave)
                    hb[k] = scan_chunk_hotbits<D>(a, mask, a.elem0 + chunk * 16, static_cast<int>(a.n_elems - chunk * 16));
                mine += static_cast<uint32_t>(__popc(hb[k]));
            }
        } else {
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                hb[k] = 0;
                if (chunk < n_chunks) {
                    const int64_t e0 = a.elem0 + chunk * 16;
                    const int64_t left = a.elem0 + a.n_elems - e0;
                    hb[k] = scan_chunk_hotbits<D>(a, mask, e0, left < 16 ? static_cast<int>(left) : 16);
                }
                mine += static_cast<uint32_t>(__popc(hb[k]));
            }
        }
        uint32_t incl = mine;                                               // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= static_cast<uint32_t>(d)) incl += up;
        }
        if (lane == 63u) s_tot[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (uint32_t w = 0; w < WPB; ++w) total += s_tot[w];
            uint32_t base = 0, ok = 1;
            if (total) {
                base = atomicAdd(&ws[0], total);
                if (base + total > capacity || base + total < base) {       // queue full: flag it, the patch kernel goes over the whole tile instead
                    atomicOr(&ws[1], 1u);
                    ok = 0;
                }
            }
            s_base = base; s_ok = ok;
            const uint32_t piece = static_cast<uint32_t>(r * gridDim.x + blockIdx.x);          // image order
            table[2u * piece] = ok ? base : 0u;
            table[2u * piece + 1u] = ok ? total : 0u;
            if (blockIdx.x == 0 && r == 0) ws[2] = static_cast<uint32_t>(rounds * gridDim.x);
        }
        __syncthreads();
        if (s_ok && mine) {
            uint32_t off = s_base + (incl - mine);
            for (uint32_t w = 0; w < wave; ++w) off += s_tot[w];
            uint32_t* q = queue + off;                                      // off + mine <= base + total <= capacity
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                uint32_t bits = hb[k];
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                const uint32_t first = static_cast<uint32_t>(a.elem0 + chunk * 16);   // < 2^32 (host check)
                while (bits) {
                    const int b = __ffs(static_cast<int>(bits)) - 1;
                    bits &= bits - 1;
                    *q++ = first + static_cast<uint32_t>(b);
                }
            }
        }
        __syncthreads();                                                    // s_tot / s_base are rewritten in the next round
    }
