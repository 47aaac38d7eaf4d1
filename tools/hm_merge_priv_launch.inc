// hm_merge_priv_launch.inc - host-side launchers of merge_u8_priv; included by hm_merge_nf.h inside namespace hm, tuning builds only.
template <int NF, int U, int MODE, int BLOCK>
static int launch_priv_cfg(const MergeK& k, hipStream_t st) {
    static bool attr_set = false;
    if (describe_only("merge_u8_priv<N=%d,U=%d,MODE=%d,BLOCK=%d>", NF, U, MODE, BLOCK)) return HM_OK;
    constexpr int lds = MODE == 0 ? static_cast<int>(kPrivLds) : 16 * 768;
    if (!attr_set && lds > 48 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(merge_u8_priv<NF, U, MODE, BLOCK>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return HM_ELAUNCH;
        attr_set = true;
    }
    const int64_t groups = k.n_elems / (U * static_cast<int>(kPrivChunk));
    const int per_cu = MODE == 0 ? 2 : 2048 / BLOCK;           // MODE 0: two 64 KB workgroups per CU
    int64_t grid = (groups + BLOCK / 64 - 1) / (BLOCK / 64);
    if (grid > static_cast<int64_t>(cu_count()) * per_cu) grid = static_cast<int64_t>(cu_count()) * per_cu;
    hipLaunchKernelGGL((merge_u8_priv<NF, U, MODE, BLOCK>), dim3(static_cast<unsigned>(grid)), dim3(BLOCK), lds, st, k);
    return launch_status();
}
// (the 8UMB variant code is decoded by priv_variant(), camera_linearity_amd/csrc/hm_merge_host.h: the dispatcher needs it too)
template <int NF>
static int launch_priv(const MergeK& k, hipStream_t st) {
    const int u = (k.variant / 100) % 10, m = (k.variant / 10) % 10, bcode = k.variant % 10;
    if (m == 0) {
        if (bcode == 2) return u == 2 ? launch_priv_cfg<NF, 2, 0, 1024>(k, st) : launch_priv_cfg<NF, 4, 0, 1024>(k, st);
        if (bcode == 1) return u == 2 ? launch_priv_cfg<NF, 2, 0, 768>(k, st) : launch_priv_cfg<NF, 4, 0, 768>(k, st);
        return u == 2 ? launch_priv_cfg<NF, 2, 0, 256>(k, st) : launch_priv_cfg<NF, 4, 0, 256>(k, st);
    }
    if (bcode == 2) return u == 2 ? launch_priv_cfg<NF, 2, 1, 1024>(k, st) : launch_priv_cfg<NF, 4, 1, 1024>(k, st);
    return u == 2 ? launch_priv_cfg<NF, 2, 1, 256>(k, st) : launch_priv_cfg<NF, 4, 1, 256>(k, st);
}

