// hm_welford_finalize_body.h - the body of k_welford_finalize (hm_welford.hip, uint8 outputs) and k_welford_finalize_u16 (hm_welford_u16.hip):
// mean -> around(mean * scale), std -> around(sqrt(m2 / (n - 1)) / sqrt(n)) (as written upstream: not rescaled). In scope: the kernels'
// parameters mean, m2, count, out_mean, out_std, n and HM_WELFORD_SCALE (255.0 there, the argument max_dn here; undefined again below).
// Included, not called: as a shared function template k_welford_finalize_u16 came out with two address registers exchanged (DESIGN.md
// 4.4.7); tools/kernel_asm_diff.py is the check.
    using Out = std::remove_reference_t<decltype(out_mean[0])>;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const double denom = count - 1.0, root_n = sqrt(count);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        if (out_mean) out_mean[e] = round_to_dn<Out>(mean[e] * HM_WELFORD_SCALE);              // :210-211
        if (out_std) out_std[e] = round_to_dn<Out>(sqrt(m2[e] / denom) / root_n);             // :214-215
    }
#undef HM_WELFORD_SCALE
