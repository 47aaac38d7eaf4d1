// hm_de_select_body.h - the body of the differential evolution's select stage, ONE workgroup per problem: deferred selection, best index /
// mean / std by fixed-order LDS trees, the stop flag and - as the last store of the generation - the generation counter. Not a header
// of declarations: hm_de.hip includes this text twice, as the body of k_de_select and as the body of de_select_body (which
// k_de_select_batch calls on its problem's slices of the state).
// In scope at the point of inclusion: `a` (the DeK arguments; the kernel holds them by value, the function by reference); tree_sum
// from hm_de.hip.
// Included, not called: routing the single-problem kernel through a shared inlined function moved its register allocation (DESIGN.md
// 4.4.3), and the single-problem path must not pay for the batch. One text keeps the two forms to the same arithmetic;
// tools/kernel_asm_diff.py shows that an edit here left the kernels it was not meant to change as they were.
    __shared__ double e[HM_DE_MAX_POP];
    __shared__ double v[HM_DE_MAX_POP];
    __shared__ int idx[HM_DE_MAX_POP];
    if (a.status[HM_DE_STOP] != 0) return;
    const int S = a.S, P = a.P;
    const int64_t g = a.status[HM_DE_GENERATION];
    int n = 1;
    while (n < S) n <<= 1;

    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        double ei = __builtin_inf();
        if (i < S) {
            const double et = a.trial_energy[i];
            ei = a.energy[i];
            if (g == 0 || et <= ei) {                                     // deferred updating: every trial saw the old population
                ei = et;
                a.energy[i] = et;
                for (int j = 0; j < P; ++j) a.pop[static_cast<int64_t>(i) * P + j] = a.trial[static_cast<int64_t>(i) * P + j];
            }
        }
        e[i] = ei;
        v[i] = i < S ? ei : 0.0;
        idx[i] = i;
    }
    __syncthreads();
    tree_sum(v, n);
    const double mean = v[0] / S;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double d = e[i] - mean;
        v[i] = i < S ? d * d : 0.0;
    }
    __syncthreads();
    tree_sum(v, n);
    const double sd = sqrt(v[0] / S);
    // lowest energy, ties to the lowest index (the padding is +inf with an index >= S, so it never wins a tie)
    for (int s = n >> 1; s > 0; s >>= 1) {
        for (int t = threadIdx.x; t < s; t += blockDim.x) {
            const double x0 = e[t], x1 = e[t + s];
            const int i0 = idx[t], i1 = idx[t + s];
            if (x1 < x0 || (x1 == x0 && i1 < i0)) { e[t] = x1; idx[t] = i1; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double best = e[0];
        int64_t stop = 0;
        if (g > 0 && (g & 1) == 0) {                                      // the reference loop advances two generations per pass (:351)
            if (isfinite(mean) && sd == sd && sd <= a.tol * fabs(mean)) stop |= HM_DE_STOP_CONVERGED;   // mean finite <=> every E finite
            if (best < a.energy_limit) stop |= HM_DE_STOP_ENERGY;
        }
        if (g >= a.max_generations) stop |= HM_DE_STOP_MAX;
        a.status[HM_DE_BEST_INDEX] = idx[0];
        a.status[HM_DE_BEST_ENERGY] = __double_as_longlong(best);
        a.status[HM_DE_MEAN] = __double_as_longlong(mean);
        a.status[HM_DE_STD] = __double_as_longlong(sd);
        a.status[HM_DE_EVALUATIONS] += S;
        a.status[HM_DE_STOP] = stop;
        a.status[HM_DE_GENERATION] = g + 1;
    }
