// hm_energy_partial_body.h - the body of the pair-major energy kernel: one workgroup reduces one frame pair of one candidate over one
// pixel chunk. Not a header of declarations: hm_energy.hip includes this text twice, as the body of k_energy_partial<STD> and as the
// body of energy_partial_body<STD> (which k_energy_partial_batch calls on its problem's stack), and hm_energy_u16.hip once, as the body of
// k_energy_partial_u16<STD, LUT> and of k_energy_partial_u16_batch<STD, LUT>.
// In scope at the point of inclusion: `a` (the unit's kernel arguments) and the template parameter STD; wave_sum and pair_of from
// hm_energy_dev.h; and the unit's placement of the candidate's row: HM_ENERGY_ROW_DECL, HM_ENERGY_ROW_FILL(b), HM_ENERGY_ROW(dn).
// Included, not called: routing the single-stack kernel through a shared inlined function moved its register allocation in every form
// tried, and the single-stack path must not pay for the batch. One text keeps the two forms to the same arithmetic;
// tools/kernel_asm_diff.py shows that an edit here left the kernels it was not meant to change as they were.
// The stack a kernel reads is HM_ENERGY_DN / HM_ENERGY_SD: the arguments' own unless the including unit names another before the
// inclusion - hm_energy_u16.hip's batched kernels name their problem's, without copying the arguments (a copy of `a` put its exposure
// array, which the pair indexes, into scratch memory).
#ifndef HM_ENERGY_DN
#define HM_ENERGY_DN a.dn
#define HM_ENERGY_SD a.sd
#endif
    HM_ENERGY_ROW_DECL
    __shared__ double red[4][2];
    const int b = blockIdx.z;
    double* out = a.partial + ((static_cast<int64_t>(b) * gridDim.y + blockIdx.y) * a.chunks + blockIdx.x) * 2;
    if (a.valid && !a.valid[b]) {                     // uniform per workgroup
        if (threadIdx.x == 0) { out[0] = 0.0; out[1] = 0.0; }
        return;
    }
    HM_ENERGY_ROW_FILL(b)
    int i, j;
    pair_of(blockIdx.y, a.N, i, j);
    const double lo = HM_ENERGY_ROW(a.lower), hi = HM_ENERGY_ROW(a.upper);
    const double ratio = a.t[i] / a.t[j];
    const int N = a.N;

    double num = 0.0, den = 0.0;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < a.P; p += stride) {
        const auto* px = HM_ENERGY_DN + p * N;
        double vi = HM_ENERGY_ROW(px[i]), vj = HM_ENERGY_ROW(px[j]);
        if (vi < lo || vi > hi) vi = __builtin_nan("");
        if (vj < lo || vj > hi) vj = __builtin_nan("");
        const double scaled = vj * ratio;
        double d = vi - scaled;
        if (a.relative) d = d / scaled;
        const double ad = fabs(d);
        if (STD) {
            const double si = HM_ENERGY_SD[p * N + i], sj = HM_ENERGY_SD[p * N + j];
            double sigma;
            if (a.relative) {
                const double u = si / scaled;
                const double v = (vi * sj) / (ratio * (vj * vj));
                sigma = sqrt(u * u + v * v);
            } else {
                const double v = ratio * sj;
                sigma = sqrt(si * si + v * v);
            }
            const bool finite = isfinite(ad) && sigma != 0.0;
            const double w = 1.0 / sigma;
            if (finite && w == w) { num += ad * w; den += w; }
        } else {
            if (ad == ad) { num += ad; den += 1.0; }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double s0 = wave_sum(num), s1 = wave_sum(den);
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        out[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
