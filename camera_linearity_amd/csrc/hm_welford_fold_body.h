// hm_welford_fold_body.h - the second half of the units' group functions (welford_group, welford_u16_group): the G gathered frame values
// of a lane's two elements folded into their state with the fast division (hm_welford_dev.h), one text for both units. In scope: M2, G,
// `a` (rcp[]), k0, f[G][2], cnt, m[2], q[2] and HM_WELFORD_TEST_GATHERED (undefined again below): true where nobody has seen the whole
// table, so that every gathered value is tested here. -> false when one is outside the range. Included, not called: with the five
// operations in a shared function all six k_welford_u16 kernels moved; tools/kernel_asm_diff.py is the check.
    bool ok = true;
    if constexpr (HM_WELFORD_TEST_GATHERED) {
#pragma unroll
        for (int k = 0; k < G; ++k) ok = ok && !welford_entry_odd(f[k][0]) && !welford_entry_odd(f[k][1]);
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
        cnt += 1.0;
        const double r = a.rcp[k0 + k];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double delta = f[k][j] - m[j];                                  // :205
            const double q0 = delta * r;
            const double quot = fma(fma(-q0, cnt, delta), r, q0);                 // == delta / cnt
            m[j] = m[j] + quot;                                                   // :206
            if (M2) q[j] = q[j] + delta * (f[k][j] - m[j]);                       // :208
        }
    }
    return ok;
#undef HM_WELFORD_TEST_GATHERED
