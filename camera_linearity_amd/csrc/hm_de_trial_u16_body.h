// hm_de_trial_u16_body.h - the body of the trial kernel of hm_de_u16.hip: the trial components of member i (hm_de_trial_component_body.h)
// and the walk over its candidate row of R = 2^bits entries, with the range / monotonicity verdict. Not a header of declarations:
// hm_de_u16.hip includes this text twice, as the body of k_de_trial_u16<U, SLAB> and as the body of k_de_trial_u16_batch<U, SLAB>, which
// first narrows its arguments to problem blockIdx.z of a batch - so a problem's rows, trials and verdicts are the same bits alone or in a
// batch.
// In scope at the point of inclusion: `a` (the DeK arguments of ONE problem), `bits`, `slab_bad` (SLAB: that problem's (S, gridDim.y)
// verdict bytes) and the template parameters U and SLAB; mix64 / de_uniform (hm_producer_math.h). The member is blockIdx.x, the slab
// blockIdx.y.
// Included, not called: hm_de_select_body.h's reason - k_de_trial_u16 must stay the code it was (tools/kernel_asm_diff.py shows it).
    __shared__ double x[HM_DE_MAX_PARAMS];
    __shared__ double last;
    __shared__ double edge[2][U][4];                                      // [trip parity][segment of the trip][wave]: lane 63's row
    __shared__ int bad[4];
    if (a.status[HM_DE_STOP] != 0) return;                                // uniform: the whole generation is a no-op
    const int i = blockIdx.x;
    const int lane = threadIdx.x, P = a.P, S = a.S;
    const int64_t g = a.status[HM_DE_GENERATION];

#include "hm_de_trial_component_body.h"
    __syncthreads();

    const int R = 1 << bits;
    if (lane == 255) {
        const int d = R - 1;
        double row = 0.0;
        for (int j = 0; j < P; ++j) row += a.pca[d * P + j] * x[j];       // PCA @ x, DN R - 1: the expression of the walk below
        row = a.mean_icrf[d] + row;
        last = row;
    }
    __syncthreads();
    const double shift = 1.0 - last;                                      // :166
    double* const out = a.icrf + static_cast<int64_t>(i) * R;             // S * R * 8 bytes reach 512 MiB
    const int w = lane >> 6;
    bool wrong = false;
    const int s_count = SLAB ? (R >> 8) / static_cast<int>(gridDim.y) : R >> 8;   // segments of this workgroup
    const int s_begin = SLAB ? static_cast<int>(blockIdx.y) * s_count : 0;
    double carry = 0.0;                                                   // the previous trip's last row (lane 255): DN d - 1 of lane 0
    if (SLAB && s_begin > 0) {                                            // a later slab's left neighbour: the same expression (d > 0: not row 0)
        const int d = (s_begin << 8) - 1;
        double row = 0.0;
        for (int j = 0; j < P; ++j) row += a.pca[d * P + j] * x[j];
        row = a.mean_icrf[d] + row;
        carry = row + shift;
    }
    for (int s = s_begin, trip = 0; s < s_begin + s_count; s += U, ++trip) {
        const int d0 = (s << 8) + lane;
        double row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = 0.0;
#pragma unroll 4
        for (int j = 0; j < P; ++j) {
            const double xj = x[j];
#pragma unroll
            for (int u = 0; u < U; ++u) row[u] += a.pca[(d0 + (u << 8)) * P + j] * xj;
        }
        double (*e)[4] = edge[trip & 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + (u << 8);
            row[u] = a.mean_icrf[d] + row[u];
            row[u] += shift;
            if (d == 0) row[u] = 0.0;                                     // :167
            out[d] = row[u];
            if ((lane & 63) == 63) e[u][w] = row[u];
        }
        __syncthreads();
        // range (:173-175) and strict monotonicity (:177-179)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + (u << 8);
            double prev = __shfl_up(row[u], 1, 64);
            if ((lane & 63) == 0) prev = lane > 0 ? e[u][w - 1] : (u > 0 ? e[u - 1][3] : carry);
            wrong |= row[u] > 1.0 || row[u] < 0.0 || (d > 0 && !(row[u] > prev));
        }
        carry = e[U - 1][3];                                              // (this buffer is next written two trips on, behind the next barrier)
    }
    const unsigned long long any = __ballot(wrong);
    if ((lane & 63) == 0) bad[w] = any != 0ull;
    __syncthreads();
    if (lane == 0) {
        if (SLAB) slab_bad[static_cast<int64_t>(i) * gridDim.y + blockIdx.y] = (bad[0] | bad[1] | bad[2] | bad[3]) != 0;
        else a.valid[i] = !(bad[0] | bad[1] | bad[2] | bad[3]);
    }
