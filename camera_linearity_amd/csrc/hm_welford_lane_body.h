// hm_welford_lane_body.h - the lane loop of the Welford update kernels: per lane two elements' state loaded once (16-byte nontemporal
// accesses under the pair rule, scalar ones otherwise) and tested against the fast division's range (hm_welford_dev.h), the frames folded
// in groups of kWelfordGroup, the exact redo of a lane outside the range, the state stored once; then the one-thread odd tail. Not a header
// of declarations: hm_welford.hip includes this text as the rest of k_welford<M2> after its table fill, hm_welford_u16.hip as the rest of
// k_welford_u16<M2, PLACE> after its placement's setup.
// In scope at the point of inclusion: `a` (the unit's kernel arguments), M2, `table_ok` (false when the workgroup's table has an entry
// outside the range), `C` (the channel count with the type the unit gives it, int or uint32_t: how e % C widens is part of the instruction
// stream) and four macros, undefined again at the end: HM_WELFORD_PAIR_ALIGN (bytes a frame is aligned to for one load of two DNs),
// HM_WELFORD_OFFSET(c) (what the unit's functions take for channel c), HM_WELFORD_GROUP(G, VEC) (its group function on G frames from k0:
// e, off0, off1, cnt, m, q) and HM_WELFORD_EXACT(e0, count) (its exact function for `count` elements from e0 into m, q).
// Included, not called: as a shared inlined function template the loop moved the register allocation of all eight update kernels
// (DESIGN.md 4.4.7), and k_welford is FP64-VALU bound. tools/kernel_asm_diff.py shows that an edit here left the kernels as they were.
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t units = a.n / 2;
    bool vec_ok = aligned_dev(a.mean, 16) && (!M2 || aligned_dev(a.m2, 16));
    for (int k = 0; k < a.n_frames; ++k) vec_ok = vec_ok && aligned_dev(a.frame[k], HM_WELFORD_PAIR_ALIGN);

    for (int64_t u = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; u < units; u += stride) {
        const int64_t e = 2 * u;
        const uint32_t c0 = static_cast<uint32_t>(e % C), c1 = (c0 + 1u) % static_cast<uint32_t>(C);
        const uint32_t off0 = HM_WELFORD_OFFSET(c0), off1 = HM_WELFORD_OFFSET(c1);
        double m[2], q[2] = {0.0, 0.0};
        if (vec_ok) {
            const f64x2 mv = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(a.mean + e));
            m[0] = mv.x; m[1] = mv.y;
            if (M2) { const f64x2 qv = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(a.m2 + e)); q[0] = qv.x; q[1] = qv.y; }
        } else {
            m[0] = a.mean[e]; m[1] = a.mean[e + 1];
            if (M2) { q[0] = a.m2[e]; q[1] = a.m2[e + 1]; }
        }
        bool ok = table_ok && welford_mean_ok(m[0]) && welford_mean_ok(m[1]) && welford_m2_ok(q[0]) && welford_m2_ok(q[1]);
        double cnt = a.count0;
        int k0 = 0;
        if (vec_ok) {
            for (; k0 + kWelfordGroup <= a.n_frames; k0 += kWelfordGroup) ok = HM_WELFORD_GROUP(kWelfordGroup, true) && ok;
            for (; k0 < a.n_frames; ++k0) ok = HM_WELFORD_GROUP(1, true) && ok;
        } else {
            for (; k0 < a.n_frames; ++k0) ok = HM_WELFORD_GROUP(1, false) && ok;
        }
        if (__builtin_expect(!ok, 0)) {                // the state in memory is still the launch's input
            HM_WELFORD_EXACT(e, 2);
        }
        if (vec_ok) {
            f64x2 mv; mv.x = m[0]; mv.y = m[1];
            __builtin_nontemporal_store(mv, reinterpret_cast<f64x2*>(a.mean + e));
            if (M2) { f64x2 qv; qv.x = q[0]; qv.y = q[1]; __builtin_nontemporal_store(qv, reinterpret_cast<f64x2*>(a.m2 + e)); }
        } else {
            a.mean[e] = m[0]; a.mean[e + 1] = m[1];
            if (M2) { a.m2[e] = q[0]; a.m2[e + 1] = q[1]; }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (a.n & 1)) {
        const int64_t e = a.n - 1;
        double m[1], q[1];
        HM_WELFORD_EXACT(e, 1);
        a.mean[e] = m[0];
        if (M2) a.m2[e] = q[0];
    }
#undef HM_WELFORD_PAIR_ALIGN
#undef HM_WELFORD_OFFSET
#undef HM_WELFORD_GROUP
#undef HM_WELFORD_EXACT
