// hm_de_trial_component_body.h - trial component j of member i of one differential-evolution generation (mutation, binomial crossover
// with the fill point, SciPy's _ensure_constraint redraw) and its physical parameter x[j]. Not a header of declarations: one text,
// included as the `lane < P` part of de_trial_body (hm_de.hip), of k_de_trial_u16 (hm_de_u16.hip) and, inside a loop over `lane`, of the
// host build's hm_de_generation_u16 - so the `trial` array of a generation is the same bits whichever of them wrote it.
// In scope at the point of inclusion: `a` (the DeK arguments), `i` (the member), `lane`, `P`, `S`, `g` (the generation), `x` (P doubles),
// mix64 / de_uniform (hm_producer_math.h), min / max / floor.
// Included, not called: hm_de_select_body.h's reason - k_de_trial must stay the code it was.
    if (lane < P) {
        const int j = lane;
        const double ui = a.pop[static_cast<int64_t>(i) * P + j];
        double tr = ui;                                                   // generation 0 evaluates the initial population: no draws
        if (g > 0) {
            const uint64_t key = mix64(a.seed ^ mix64(static_cast<uint64_t>(g)));
            const double F = a.m_lo + (a.m_hi - a.m_lo) * de_uniform(key, S, 0);
            // (the clamps never bind for U < 1 and a status block this library wrote: they keep a corrupted one inside the buffers)
            const int b = min(max(static_cast<int>(a.status[HM_DE_BEST_INDEX]), 0), S - 1);
            const int pick = min(static_cast<int>(floor(de_uniform(key, i, 0) * (S - 1))), S - 2);
            const int r0 = pick + (pick >= i);
            int c = min(static_cast<int>(floor(de_uniform(key, i, 1) * (S - 2))), S - 3);
            const int lo2 = i < r0 ? i : r0, hi2 = i < r0 ? r0 : i;
            c += (c >= lo2);
            c += (c >= hi2);
            const int r1 = c;
            const int fill = static_cast<int>(floor(de_uniform(key, i, 2) * P));
            if (de_uniform(key, i, 3 + j) < a.cr || j == fill) {
                const double ub = a.pop[static_cast<int64_t>(b) * P + j];
                const double u0 = a.pop[static_cast<int64_t>(r0) * P + j];
                const double u1 = a.pop[static_cast<int64_t>(r1) * P + j];
                tr = ui + F * (((ub - ui) + u0) - u1);
                if (!(tr >= 0.0 && tr <= 1.0)) tr = de_uniform(key, i, 3 + P + j);   // SciPy's _ensure_constraint
            }
        }
        a.trial[static_cast<int64_t>(i) * P + j] = tr;
        x[j] = a.lo[j] + tr * (a.hi[j] - a.lo[j]);
    }
