// hm_energy_pixel_body.h - the body of the pixel-major energy kernel (N <= 8 frames): a thread owns pixels and evaluates all N(N-1)/2
// pairs of a pixel from registers. Not a header of declarations: hm_energy.hip includes this text twice, as the body of
// k_energy_pixel<N, STD> and as the body of energy_pixel_body<N, STD> (which k_energy_pixel_batch calls on its problem's stack), and
// hm_energy_u16.hip twice, as the body of k_energy_pixel_u16<N, STD, LUT> and of k_energy_pixel_u16_batch<N, STD, LUT>.
// In scope at the point of inclusion: `a` (the unit's kernel arguments), `pr` (the EnergyPairs ratios) and the template parameters N and STD;
// wave_sum, rcp_second_order, rsqrt_third_order and HM_ENERGY_RCP from hm_energy_dev.h; and the unit's placement of the candidate's row:
// HM_ENERGY_ROW_DECL (its declarations), HM_ENERGY_ROW_FILL(b) (made readable by the whole workgroup), HM_ENERGY_ROW(dn) (the entry of a DN).
// Included, not called: routing the single-stack kernel through a shared inlined function moved its register allocation in every form
// tried - an occupancy step for k_energy_pixel<5, false> - and the single-stack path must not pay for the batch. One
// text keeps the two forms to the same arithmetic; tools/kernel_asm_diff.py shows that an edit here left the kernels it was not meant
// to change as they were.
// The stack a kernel reads is HM_ENERGY_DN / HM_ENERGY_SD: the arguments' own unless the including unit names another before the
// inclusion (hm_energy_u16.hip's batched kernels: their problem's; see hm_energy_partial_body.h).
#ifndef HM_ENERGY_DN
#define HM_ENERGY_DN a.dn
#define HM_ENERGY_SD a.sd
#endif
    constexpr int P = N * (N - 1) / 2;
    HM_ENERGY_ROW_DECL
    __shared__ double red[4][2 * P];
    const int b = blockIdx.y;
    const int pairs = P;
    auto out_of = [&](int p) { return a.partial + ((static_cast<int64_t>(b) * pairs + p) * a.chunks + blockIdx.x) * 2; };
    if (a.valid && !a.valid[b]) {
        if (threadIdx.x < P) { double* o = out_of(threadIdx.x); o[0] = 0.0; o[1] = 0.0; }
        return;
    }
    HM_ENERGY_ROW_FILL(b)
    const double lo = HM_ENERGY_ROW(a.lower), hi = HM_ENERGY_ROW(a.upper);
    const bool rel = a.relative != 0;
    double num[P], den[P];
#pragma unroll
    for (int p = 0; p < P; ++p) { num[p] = 0.0; den[p] = 0.0; }

    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t px = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; px < a.P; px += stride) {
        const auto* q = HM_ENERGY_DN + px * N;
        double v[N], rv[N], s[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double x = HM_ENERGY_ROW(q[i]);
            if (x < lo || x > hi) x = __builtin_nan("");                       // :96-97
            v[i] = x;
            rv[i] = HM_ENERGY_RCP ? rcp_second_order(x) : 1.0 / x;
            s[i] = STD ? HM_ENERGY_SD[px * N + i] : 0.0;
        }
        int p = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
            for (int j = i + 1; j < N; ++j, ++p) {
                const double ratio = pr.ratio[p];
                const double scaled = v[j] * ratio;                             // :111
                double d = v[i] - scaled;                                        // :114
                double inv_s = 0.0;
                if (rel) { inv_s = rv[j] * pr.inv_ratio[p]; d = d * inv_s; }     // :117  d / scaled
                const double ad = fabs(d);                                       // :120
                if (STD) {
                    double qq;
                    if (rel) {
                        const double u = s[i] * inv_s;                           // s_i / scaled
                        const double w2 = ((v[i] * s[j]) * inv_s) * rv[j];       // (v_i s_j) / (ratio v_j^2)        :127
                        qq = u * u + w2 * w2;
                    } else {
                        const double w2 = ratio * s[j];
                        qq = s[i] * s[i] + w2 * w2;                              // :129
                    }
                    const double w = rsqrt_third_order(qq);                      // 1 / sigma
                    const bool ok = isfinite(ad) && qq != 0.0 && w == w;         // :133-134, general_functions.py:164
                    if (ok) { num[p] += ad * w; den[p] += w; }
                } else {
                    if (ad == ad) { num[p] += ad; den[p] += 1.0; }               // :138
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double s0 = wave_sum(num[p]), s1 = wave_sum(den[p]);
        if (lane == 0) { red[wave][2 * p] = s0; red[wave][2 * p + 1] = s1; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * P) {
        const int p = threadIdx.x >> 1, k = threadIdx.x & 1;
        out_of(p)[k] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
