/*
 * hdrmerge.h - C ABI of the MI355X-native HDR-merge / linearization engine (libhdrmerge.so).
 *
 * This is the drop-in boundary for ONE path of samivout/camera_linearity: per-pixel ICRF-LUT
 * linearization -> Gaussian-weighted HDR merge -> first-order uncertainty propagation, with
 * dark-frame hot-pixel filtering and flat-field correction. The reference has no FFI of its own;
 * its extension point is the array-backend protocol of AbstractMeasurand
 * (modules/measurand.py:26-32, modules/cupy_measurand.py:28-39, modules/measurand_factory.py:10-14).
 * A maintainer binds these entry points with ctypes from a third backend class next to
 * NumpyMeasurand / CupyMeasurand; each declaration below cites the reference
 * function whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.Tensor.data_ptr()) unless marked [host];
 *     buffers are caller-owned, contiguous, and never retained after the call returns;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is
 *     asynchronous on that stream and performs no allocation and no host synchronisation, so it may
 *     be captured in a hipGraph;
 *   - images are row-major H x W x C with the channel innermost (OpenCV BGR order,
 *     modules/global_settings.py:32); "n" counts ELEMENTS (H*W*C), element e has channel e % C;
 *   - 8-bit frames are digital numbers (DN) 0..255; their value is DN / 255.0
 *     (modules/image_set.py:223); BITS = 256, MAX_DN = 255 (modules/global_settings.py:35-37);
 *   - return value: HM_OK (0) or a negative HM_E* code; nothing throws. hm_strerror() names it.
 *
 * Two libraries export this ABI. libhdrmerge.so (the .hip files under csrc/) is the MI355X build described above. libhdrmerge_host.so
 * (csrc_host/hm_host.cpp, plain C++) is the HOST build behind Measurand(use_cupy=False) - the slot of the reference's NumpyMeasurand
 * (modules/measurand_factory.py:10-14): every pointer is then a HOST pointer, `stream` is ignored, calls are synchronous and workspaces
 * may be NULL; the hm_tiff_* decoders are not exported (the two strip decoders are host code of libhdrmerge.so already;
 * hm_tiff_decode_strips / hm_tiff_decode_strips_wide, the device path of the same files, and hm_tiff_encode_strips / hm_tiff_encode_strips_wide, their writing twins, are in both builds).
 * The device build never calls or falls back to the host build.
 */
#ifndef HDRMERGE_H
#define HDRMERGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history. 1: first release (hm_merge_args 264 bytes), later grown by hot_workspace / hot_workspace_bytes (280 bytes) without a bump.
 * 2: frames_workspace / frames_workspace_bytes (296 bytes), hm_merge_frames_workspace_bytes(), stacks of more than HM_MAX_FRAMES
 *    frames; hm_merge still accepts the 264- and 280-byte layouts (the missing tail reads as "no workspace").
 *    Later grown by the hm_noise_profile_* and hm_kde_* entry points without a bump (additions only), and likewise by
 *    hm_merge_std_table* and hm_merge_std_f32* (new entry points beside hm_merge; hm_merge_args keeps its 296 bytes), and by
 *    hm_merge_u16*, hm_linearize_u16 and hm_gaussian_weight_lut_bits_host (uint16 DN frames of 9- to 16-bit cameras; HM_BITS below is
 *    the table size of the 8-bit entry points only), and by hm_merge_u16_darks* (uint16 dark maps for those frames), and by
 *    hm_linearity_energy_u16*, hm_welford_*_u16* and hm_noise_moments_* (the calibration energy, the mean / std producer and the per-DN STD
 *    table for those frames), and by hm_merge_u16_std_table* (that table inside the merge of those frames), and by
 *    hm_de_generation_u16 (the differential-evolution generation on those stacks), and by hm_de_generation_u16_batch (several such
 *    problems per call).                                                                  */
#define HM_ABI_VERSION 2
#define HM_BITS 256
#define HM_MAX_FRAMES 32     /* frames per merge LAUNCH; hm_merge takes any number of frames (32 per launch, see frames_workspace) */
#define HM_MAX_CHANNELS 4

enum {
    HM_OK = 0,
    HM_EINVAL = -1,        /* bad argument (null pointer, non-positive size, bad enum)        */
    HM_EUNSUPPORTED = -2,  /* valid request this build cannot serve (C > 4; N > HM_MAX_FRAMES without frames_workspace / out_sum_w) */
    HM_EALIGN = -3,        /* a float64 buffer is not 8-byte aligned (a float32 output: not 4-byte aligned) */
    HM_ELAUNCH = -4,       /* the HIP runtime rejected the launch (hipGetLastError != success) */
    HM_ENODEVICE = -5,     /* no usable gfx950 device                                          */
    HM_ESHAPE = -6         /* geometry inconsistent (tile outside image, halo too small, ...)  */
};

int hm_version(void);                 /* HM_ABI_VERSION of the loaded library          */
const char* hm_strerror(int code);    /* static string, never NULL                     */
int hm_device_info(int* n_devices, int* cu_count, int* lds_bytes, char* arch, int arch_len);
/* (diagnostic probes - clock, copy rate, address translation - are declared in hdrmerge_debug.h: they replace nothing in the reference) */

/* ------------------------------------------------------------------------------------------
 * Row 3 - AbstractMeasurand.apply_gaussian_weight (modules/measurand.py:606-618)
 *   w = e**(-30 (v-0.5)^2), dw = -60 (v-0.5) w.
 * hm_gaussian_weight_f64 evaluates it analytically on float64 values; hm_gaussian_weight_u8 looks
 * the DN up in the caller's 256-entry tables (bit-identical to NumPy when the caller built the
 * tables with NumPy). Either output may be NULL.
 * ------------------------------------------------------------------------------------------ */
int hm_gaussian_weight_f64(const double* v, double* w, double* dw, int64_t n, void* stream);
int hm_gaussian_weight_u8(const uint8_t* dn, const double* w_lut, const double* dw_lut,
                          double* w, double* dw, int64_t n, void* stream);
/* [host] helper for C callers: fills w_lut/dw_lut (256 each) with libm pow(); may differ from
 * NumPy's `np.e ** x` in the last ulp. */
int hm_gaussian_weight_lut_host(double* w_lut /*[host]*/, double* dw_lut /*[host]*/);

/* ------------------------------------------------------------------------------------------
 * Row 1 - ImageSet.load_value_image arithmetic (modules/image_set.py:223): out = dn / 255.0
 * ------------------------------------------------------------------------------------------ */
int hm_u8_to_unit_f64(const uint8_t* dn, double* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row 4 - AbstractMeasurand.linearize / _linearize_channel / _linearize_single
 *         (modules/measurand.py:471-541)
 *   idx  = dn                       (integer input, :505/:533)
 *        = uint8(rint(v * 255))     (float input, round-half-even then wrap mod 256, :503/:531)
 *   out_val[e] = icrf[idx[e] * lut_stride + (e % C) * (lut_stride > 1)]
 *   out_std[e] = icrf_diff[...same...] * std[e]    only when std, icrf_diff and out_std are given
 * icrf / icrf_diff are (256, C) row-major (lut_stride == C) or 1-D (256,) applied to every channel
 * (lut_stride == 1, the `_linearize_single` form used by ImageSet.calculate_numerical_STD,
 * modules/image_set.py:383). out_idx (nullable) exposes the uint8 index for the bit-exact check.
 * ------------------------------------------------------------------------------------------ */
int hm_linearize_u8(const uint8_t* dn, const double* std, const double* icrf, const double* icrf_diff,
                    double* out_val, double* out_std, int64_t n, int C, int lut_stride, void* stream);
int hm_linearize_f64(const double* v, const double* std, const double* icrf, const double* icrf_diff,
                     double* out_val, double* out_std, uint8_t* out_idx,
                     int64_t n, int C, int lut_stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rows 5-9 fused - ExposureSeries._precalculate_sum_of_weights + _compute_HDR_image_set
 * (modules/exposure_series.py:317-397) with the optional hot-pixel prologue
 * (ImageSet.bad_pixel_filter -> filter_larger_than_by_map, modules/measurand.py:543-557) and the
 * optional flat-field epilogue (normalize_by_map, modules/measurand.py:559-604).
 *
 *   S      = sum_i w(v_i)                                                       (:340)
 *   val    = sum_i (w_i g_i) / (S t_i)                                          (:388)
 *   var    = sum_i ( ((dw_i g_i + w_i dg_i)/S - (dw_i w_i g_i)/S^2) dg_i/t_i )^2 (:389)
 *   std    = var ** (1/2)                                                       (:394)
 * with v_i the frame value BEFORE linearization, g_i = icrf[idx_i, c], dg_i = icrf_diff[idx_i, c] * std_i.
 * One streaming launch reads every frame / std / flat byte once and writes every output byte once; when dark
 * maps are given a second, stream-ordered launch reads each dark byte once and recomputes the (rare) elements
 * that have a hot frame with the k x k medians substituted. Results do not depend on how the image is tiled.
 *
 * Tiling: a call produces image rows [row0, row0 + rows) of an H x W x C image.
 * Input frame / std / dark pointers address image row `buf_row0` (<= row0) and hold `buf_rows`
 * rows, so a row-tile shard passes its slice plus the median halo; the median uses scipy 'reflect'
 * only at the true image edges (0 and H). Output and flat pointers address row0.
 * ------------------------------------------------------------------------------------------ */
typedef struct hm_merge_args {
    uint32_t struct_size;         /* sizeof(hm_merge_args), for ABI evolution                       */
    int32_t  n_frames;            /* N >= 1, ascending exposure (N > HM_MAX_FRAMES: see frames_workspace) */
    int32_t  channels;            /* C, 1..HM_MAX_CHANNELS                                          */
    int32_t  variant;             /* 0 = library default; >0 selects a tuning variant (tools/tune_merge.py), -1 forces the generic kernel,
                                     <= -2 forces the chunked path with -variant frames per launch (tests);
                                     32 with out_kind = HM_OUT_F32: the default dispatch with merge_u8_val3's pair stores forced (A/B
                                     of the float32 store shape, tools/bench_merge_f32.py) */
    int64_t  height;              /* H of the full image                                            */
    int64_t  width;               /* W                                                              */
    int64_t  row0, rows;          /* output rows of this call                                       */
    int64_t  buf_row0, buf_rows;  /* image rows covered by the input buffers                        */
                                  /* (the streaming kernels read element pairs: they need the call's first input element,
                                     (row0 - buf_row0) * W * C elements into every frame buffer, at an EVEN offset - and float64
                                     frames / stds / outputs / flat buffers 16-byte aligned there; otherwise the call runs in the
                                     one-element-per-thread generic kernel: same bits, 3-4 x slower. Only an odd W * C with an odd
                                     number of halo rows above the tile breaks this: give such a tile one more row above.
                                     With out_kind = HM_OUT_F32 the same rule holds with float32 out_val / out_std 8-byte aligned
                                     there - the streaming kernels store element pairs, 8 bytes per lane; float32 outputs that are
                                     only 4-byte aligned run in the generic kernel. out_sum_w is float64 and keeps its 16 bytes.
                                     The val-only kernel merge_u8_val3 stores FOUR float32 elements per lane where it can: uint8
                                     frames / flat field 4-byte aligned and out_val 16-byte aligned at the first element; calls that
                                     only meet the pair rule run the same kernel with pair stores.
                                     With float32 std frames (hm_merge_std_f32) the lane's two stds are one 8-byte load: the call's
                                     first input element must sit at an even element offset and every std buffer must be 8-byte
                                     aligned at that element; otherwise the call runs in the generic kernel, same bits.)            */

    const uint8_t* const* frames_u8;   /* [host] N device pointers to uint8 DN frames, or NULL       */
    const double*  const* frames_f64;  /* [host] N device pointers to float64 value frames, or NULL  */
    const double*  const* stds;        /* [host] N device pointers to float64 std frames, or NULL    */
    const double*  exposures;          /* [host] N exposure times in seconds (features['exposure'])  */

    const double* icrf;           /* (256, C) float64                                               */
    const double* icrf_diff;      /* (256, C) float64; required when stds != NULL                   */
    const double* w_lut;          /* (256,) weight table on the DN grid (u8 frames)                 */
    const double* dw_lut;         /* (256,) weight derivative table (u8 frames with stds)           */

    /* hot-pixel prologue: frame i is filtered where dark_u8[i][e] >= dark_min_dn[i]                 */
    const uint8_t* const* darks_u8;    /* [host] N device pointers (NULL entries = no filter), or NULL */
    const int32_t* dark_min_dn;        /* [host] N thresholds in DN (1..256)                         */
    int32_t  median_k;            /* odd kernel size (gs.MEDIAN_FILTER_KERNEL_SIZE), 3..7           */
    int32_t  out_kind;            /* HM_OUT_F64 (0) or HM_OUT_F32: element type of out_val / out_std. Read only when struct_size ==
                                     sizeof(hm_merge_args): the 264- and 280-byte layouts always mean float64. Other values: HM_EINVAL.
                                     All arithmetic is float64 either way; HM_OUT_F32 rounds the float64 result once, to nearest even,
                                     at the store ((float)x) and writes 4-byte elements: out_val / out_std are then `float` arrays, 4-byte
                                     aligned. HM_EUNSUPPORTED with HM_OUT_F32, before any launch: n_frames > HM_MAX_FRAMES or variant <= -2
                                     (the chunked path keeps float64 running sums in out_val / out_std) and a tile of 2^32 elements
                                     or more.                                                                                       */

    /* flat-field epilogue (all NULL = off)                                                          */
    const uint8_t* flat_u8;       /* flat value as DN (value = DN/255), or                          */
    const double*  flat_f64;      /* flat value as float64                                          */
    const double*  flat_std;      /* flat uncertainty, float64 (required when std output is on)     */
    double ff_mean[HM_MAX_CHANNELS];     /* per-channel ROI mean of flat value  (measurand.py:582)  */
    double ff_std_mean[HM_MAX_CHANNELS]; /* per-channel ROI mean of flat std    (measurand.py:583)  */

    double* out_val;              /* rows x W x C float64 (float with HM_OUT_F32), or NULL (sum-of-weights only) */
    double* out_std;              /* rows x W x C float64 (float with HM_OUT_F32); required iff stds != NULL */
    double* out_sum_w;            /* optional S (rows x W x C), float64 in both kinds, NULL to skip */

    /* hot-pixel queue (optional; used when darks_u8 is set). With a workspace the dark maps are scanned into a queue of hot
     * element indices and a balanced second kernel patches one queued element per lane - its cost follows the number of
     * hot elements, dense maps included. NULL: the scan recomputes hot elements one at a time per wave (sparse maps only).
     * Device memory, 16-byte aligned, hm_merge_hot_workspace_bytes(rows * W * C) bytes recommended (down to
     * hm_merge_hot_workspace_min_bytes() is legal: a queue that overflows makes the patch kernel test every element itself;
     * anything smaller selects the NULL path); owned by this call until it has completed on `stream`.                      */
    void*    hot_workspace;
    size_t   hot_workspace_bytes;

    /* Stacks of more than HM_MAX_FRAMES frames (the reference's loop has no limit, modules/exposure_series.py:334,372) are merged
     * HM_MAX_FRAMES frames per launch with the running sums in memory: the numerator in out_val, the variance in out_std, and the sum
     * of weights in out_sum_w when the call has one, else HERE: device memory, 16-byte aligned, hm_merge_frames_workspace_bytes()
     * bytes (one float64 per output element), owned by the call until it has completed on `stream`. NULL with N > HM_MAX_FRAMES and
     * no out_sum_w: HM_EUNSUPPORTED. Same operation sequence per element as the one-launch kernels (bit-identical for any chunking).  */
    void*    frames_workspace;
    size_t   frames_workspace_bytes;
} hm_merge_args;

enum { HM_OUT_F64 = 0, HM_OUT_F32 = 1 };   /* hm_merge_args.out_kind */
int hm_merge(const hm_merge_args* args /*[host]*/, void* stream);
/* Recommended / smallest accepted size of hm_merge_args.hot_workspace for a call with n_elems = rows * W * C output elements
 * (counters + a table of 8 bytes per 65 536 elements + the queue: a quarter of the elements / one entry). */
size_t hm_merge_hot_workspace_bytes(int64_t n_elems);
size_t hm_merge_hot_workspace_min_bytes(int64_t n_elems);
/* Bytes of hm_merge_args.frames_workspace for a call with n_frames frames and n_elems = rows * W * C output elements: 0 up to
 * HM_MAX_FRAMES frames or when the call has an out_sum_w, else 8 * n_elems. */
size_t hm_merge_frames_workspace_bytes(int n_frames, int64_t n_elems, int has_out_sum_w);

/* Algorithmic HBM bytes one hm_merge call moves: every input byte once, every output
 * byte once (4 bytes per out_val / out_std element with HM_OUT_F32), LUTs excluded. Used by bench.py for roofline.achieved. */
int64_t hm_merge_algorithmic_bytes(const hm_merge_args* args /*[host]*/);
/* The kernels hm_merge() would launch for these arguments, in launch order, as text ("merge_u8_val3<N=7,...> +
 * merge_fixup_hot<...>"): the same dispatch code runs with launching switched off. Same status codes as hm_merge.
 * With HM_OUT_F32 every listed kernel that stores val / std carries "out=f32" in its name. */
int hm_merge_describe(const hm_merge_args* args, char* buf, int buf_len);

/* hm_merge with the per-frame uncertainty taken from a per-DN table instead of N float64 std frames (the reference's default for
 * captures without "<name> STD.tif" files: ImageSet.calculate_numerical_STD, modules/image_set.py:365-385):
 *     std_i[h, w, c] = std_table[idx_i * C + c],
 * idx_i the index linearize forms (the DN of a uint8 frame, rint(v * 255) & 255 of a float64 frame). The result equals hm_merge on the
 * same arguments plus stds[i] = hm_linearize_u8 / hm_linearize_f64(frame_i, icrf = std_table).val, bit for bit, without those frames ever
 * existing: the table sits in LDS next to the ICRF tables. For a frame that is hot at an element (dark maps) the std is the k x k median
 * of the MAPPED neighbourhood, median_j(std_table[idx_j * C + c]), as the reference filters the std image on its own
 * (modules/measurand.py:553-555) - not std_table[median DN].
 * std_table: (256, C) float64, [device] (host memory on the host build), 8-byte aligned (else HM_EALIGN). args->stds must be NULL.
 * HM_EINVAL: NULL args (returned before anything else is read), args->stds set, NULL std_table, no icrf_diff, no dw_lut (uint8 frames),
 * out_val without out_std. A call without out_val (sum of weights only) behaves as hm_merge. Everything else - out_kind, flat field,
 * out_sum_w, row tiles, the older struct_size values - as hm_merge, except: more than HM_MAX_FRAMES frames and variant <= -2 (the chunked
 * path) are HM_EUNSUPPORTED, before any launch. float64 frames with a table stream through merge_generic only (merge_f64_std reads std frames).
 * hm_merge_std_table_describe: as hm_merge_describe; every listed kernel that forms a std carries "std=lut".
 * hm_merge_std_table_algorithmic_bytes: hm_merge_algorithmic_bytes for the same call with std frames, minus their 8 N bytes per element
 * (both outputs counted, the table excluded like the other LUTs). */
int hm_merge_std_table(const hm_merge_args* args /*[host]*/, const double* std_table, void* stream);
int hm_merge_std_table_describe(const hm_merge_args* args, const double* std_table, char* buf, int buf_len);
int64_t hm_merge_std_table_algorithmic_bytes(const hm_merge_args* args /*[host]*/);

/* hm_merge with the per-frame uncertainty read from N FLOAT32 std frames as they are (what ImageSet.save_32bit writes and a float32
 * Measurand keeps), instead of widening each into a float64 copy first: 4 N bytes per element less to read, and no second copy to hold.
 *   - The result equals hm_merge on the same arguments with stds[i] set to the float64 widening of stds_f32[i], bit for bit in out_val,
 *     out_std and out_sum_w: for both out_kind values, with or without flat field, dark maps (with or without hot_workspace), out_sum_w
 *     and row tiles (row0 / rows / buf_row0 / buf_rows), for uint8 and float64 frames, C = 1..4, and the 264- / 280-byte layouts.
 *   - Each float32 std is converted to float64 once, in registers (exact); all arithmetic stays float64 in the operation sequence every
 *     kernel of the merge shares, so the result does not depend on which kernel or tiling produced it.
 *   - For a frame that is hot at an element (dark maps) the std is the k x k median of the std neighbourhood, as in hm_merge: widening is
 *     monotone and exact, so the median may be taken on either side of the conversion.
 * stds_f32: [host] N device pointers (host memory on the host build) to float32 frames with the frames' geometry, each 4-byte aligned
 * (else HM_EALIGN). args->stds must be NULL; flat_std stays float64.
 * HM_EINVAL, in this order: NULL args (returned before anything else is read), args->stds set, NULL stds_f32 or a NULL entry, no icrf_diff,
 * no dw_lut (uint8 frames), out_val without out_std. Then HM_EALIGN: a std pointer that is not 4-byte aligned. A call without out_val (sum
 * of weights only) behaves as hm_merge. Everything else as hm_merge, except: more than HM_MAX_FRAMES frames and variant <= -2 (the chunked
 * path) are HM_EUNSUPPORTED, before any launch. uint8 frames stream (compile-time-N kernels for colour stacks of 7 and 15 frames,
 * merge_u8_loop_std at run-time N for every other shape); float64 frames with float32 stds run in merge_generic only.
 * The streaming kernels' pair rule for float32 stds is stated at hm_merge_args.buf_row0.
 * hm_merge_std_f32_describe: as hm_merge_describe; every listed kernel that reads stds carries "std=f32" (merge_scan_hot reads none).
 * hm_merge_std_f32_algorithmic_bytes: hm_merge_algorithmic_bytes of the same call with float64 std frames, minus 4 N bytes per element. */
int hm_merge_std_f32(const hm_merge_args* args /*[host]*/, const float* const* stds_f32 /*[host] N device pointers*/, void* stream);
int hm_merge_std_f32_describe(const hm_merge_args* args, const float* const* stds_f32, char* buf, int buf_len);
int64_t hm_merge_std_f32_algorithmic_bytes(const hm_merge_args* args /*[host]*/);

/* hm_merge for 9- to 16-bit cameras: N frames of uint16 DNs with an explicit bit depth. With M = 2^bit_depth - 1 a frame element DN has
 * the value DN / M; the kernels never form it: everything per-DN comes from the caller's tables of 2^bit_depth rows - icrf, icrf_diff:
 * (2^bit_depth, C); w_lut, dw_lut: (2^bit_depth,) (hm_gaussian_weight_lut_bits_host) - at the index idx = DN & M, the package's wrap
 * convention. The mask is applied before EVERY table access, so stray high bits never read outside a table. The arithmetic per output
 * element is hm_merge's operation sequence: a result does not depend on which kernel or tiling produced it, and a stack whose DNs and
 * tables embed an 8-bit stack (DN16 = DN8 << (bit_depth - 8)) gives hm_merge's bits.
 * frames_u16: [host] array of N device pointers (host memory on the host build), 2-byte aligned, addressing image row buf_row0.
 * args->frames_u8 and args->frames_f64 must be NULL. Statuses, an earlier rule wins:
 *   1. HM_EINVAL: NULL args or a bad struct_size; frames_u8 / frames_f64 set; NULL frames_u16 or a NULL entry; bit_depth outside 9..16;
 *      no w_lut; with stds: no icrf_diff or no dw_lut.
 *   2. HM_EALIGN: a frame pointer that is not 2-byte aligned.
 *   3. Every remaining rule of hm_merge; then HM_EINVAL for a variant above 3.
 *   4. HM_EUNSUPPORTED, before any launch: darks_u8, flat_u8, more than HM_MAX_FRAMES frames or variant <= -2, variant 1 with tables
 *      that do not fit in LDS, variant 3 where not even the per-DN tables fit.
 * Supported: value-only merges and float64 std frames (args->stds), out_sum_w, the sum-of-weights-only call, both out_kind values,
 * flat_f64 with flat_std, row tiles, C = 1..4, the 264- and 280-byte layouts.
 * variant: 0 the library's choice; -1 the one-element-per-thread kernel; 1 the streaming kernel with its tables in LDS; 2 the streaming
 * kernel with its tables read from global memory; 3 the streaming kernel with the largest PART of its tables that fits in LDS.
 * Tables in LDS - the fit rule, n = 2^bit_depth: value-only calls hold w[n] and (w g)[n C], 8 (1 + C) n bytes; std calls hold {w, dw}[n]
 * and {g, d}[n C], 16 (1 + C) n bytes; the tables live in LDS when that is at most 160 KiB (a gfx950 workgroup's maximum). Where it is
 * more, the largest of these parts that fits does ("tab=mixed-..."): std calls {w, dw}[n] and g[n C], 8 (2 + C) n bytes, with icrf_diff
 * gathered from global memory; else the per-DN tables alone, w[n] (8 n bytes) or {w, dw}[n] (16 n bytes), with the per-(DN, channel)
 * tables gathered from global memory; else nothing (every gather from global memory: value-only from 15 bits, with std from 14).
 * The streaming kernels' pair rule (two elements per lane, one 4-byte load per frame): frame pointers 4-byte aligned at the first input
 * element, float64 outputs / flat field / std frames 16-byte aligned there (float32 outputs: 8-byte). Calls that break it run in the
 * one-element-per-thread kernel with the same bits.
 * hm_merge_u16_describe: as hm_merge_describe; the kernel names say where the tables live ("merge_u16_stream<tab=lds,...>", "tab=global",
 * "tab=mixed-wdwg", "tab=mixed-wdw", "tab=mixed-w").
 * hm_merge_u16_algorithmic_bytes: 2 N bytes per element for the frames; the rest as hm_merge. */
int hm_merge_u16(const hm_merge_args* args /*[host]*/, const uint16_t* const* frames_u16 /*[host] N device pointers*/, int bit_depth, void* stream);
int hm_merge_u16_describe(const hm_merge_args* args, const uint16_t* const* frames_u16, int bit_depth, char* buf, int buf_len);
int64_t hm_merge_u16_algorithmic_bytes(const hm_merge_args* args /*[host]*/);

/* hm_merge_u16 with the hot-pixel prologue: per frame a uint16 dark DN map with the frames' geometry, or NULL ("no filter for this frame").
 * With M = 2^bit_depth - 1, frame i is hot at element e iff (darks_u16[i][e] & M) >= args->dark_min_dn[i] - the wrap convention applied to
 * dark DNs too; thresholds are 1 .. 2^bit_depth, and 2^bit_depth means that no DN is hot (as 256 does for hm_merge). Where a frame is hot
 * its DN is replaced by the k x k median (k = args->median_k: 3, 5 or 7) of the masked DNs (DN & M) of its spatial neighbourhood - same
 * channel, scipy 'reflect' at the true image edges - and, with std frames, its std by the k x k median of the std neighbourhood: hm_merge's
 * pass (modules/measurand.py:543-557). out_val, out_std and out_sum_w (either out_kind, with or without the float64 flat field, the
 * sum-of-weights-only call included) are bit for bit those of hm_merge_u16 on the frames filtered that way beforehand.
 * darks_u16: [host] array of N device pointers (host memory on the host build), each NULL or 2-byte aligned, addressing image row
 * buf_row0. args->darks_u8 must be NULL. args->hot_workspace / hot_workspace_bytes: optional, sized by hm_merge_hot_workspace_bytes /
 * hm_merge_hot_workspace_min_bytes as for hm_merge; NULL, too small, not 16-byte aligned or a tile of 2^32 elements or more: the patch
 * kernel tests every element's dark DNs itself (same bits). Row tiles follow hm_merge's halo rule: the buffers cover median_k / 2 rows
 * beyond the tile except at the image edges. Statuses, an earlier rule wins:
 *   1. HM_EINVAL: hm_merge_u16's rule 1; then NULL darks_u16, args->darks_u8 set, no dark_min_dn.
 *   2. HM_EALIGN: a frame pointer, then a dark map pointer, that is not 2-byte aligned.
 *   3. Every remaining rule of hm_merge, with its hot-pixel checks in their place when at least one map is given: HM_EINVAL for a median_k
 *      other than 3, 5, 7; HM_ESHAPE for a missing halo; then HM_EINVAL for a threshold outside 1 .. 2^bit_depth of a frame that has a
 *      map. Then HM_EINVAL for a variant above 3.
 *   4. HM_EUNSUPPORTED: hm_merge_u16's rule 4 (flat_u8, more than HM_MAX_FRAMES frames or variant <= -2, variants 1 / 3 that do not fit).
 * With every entry of darks_u16 NULL the call runs exactly as hm_merge_u16 does (same kernels, same describe string); hm_merge_u16 itself
 * keeps refusing args->darks_u8 with HM_EUNSUPPORTED.
 * hm_merge_u16_darks_describe: hm_merge_u16's names, then " + merge_u16_scan_hot + merge_u16_patch_hot<bits=b,std=s,k=K>" with a usable
 * workspace or " + merge_u16_patch_hot<bits=b,std=s,k=K,queue=0>" without one.
 * hm_merge_u16_darks_algorithmic_bytes: hm_merge_u16's count plus 2 bytes per element for every DISTINCT (map, threshold). */
int hm_merge_u16_darks(const hm_merge_args* args /*[host]*/, const uint16_t* const* frames_u16 /*[host] N device pointers*/,
                       const uint16_t* const* darks_u16 /*[host] N device pointers or NULLs*/, int bit_depth, void* stream);
int hm_merge_u16_darks_describe(const hm_merge_args* args, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth,
                                char* buf, int buf_len);
int64_t hm_merge_u16_darks_algorithmic_bytes(const hm_merge_args* args /*[host]*/, const uint16_t* const* darks_u16 /*[host]*/);

/* hm_merge_u16 / hm_merge_u16_darks with the per-frame stds taken from the per-DN STD table of the camera (hm_noise_moments_*): frame i's
 * std at element e, channel c is std_table[(DN_i & M) * C + c], M = 2^bit_depth - 1, formed inside the kernels - no std frame exists.
 * std_table: device pointer (host memory on the host build), (2^bit_depth, C) float64, 8-byte aligned. args->stds must be NULL.
 * darks_u16: NULL for no hot-pixel pass, else as for hm_merge_u16_darks; a hot frame's std is the k x k median of the mapped neighbourhood,
 * median_j(std_table[(DN_j & M) * C + c]) - the median of the std frame the table stands for - and its DN the median of the masked DNs.
 * out_val, out_std and out_sum_w are bit for bit those of hm_merge_u16 / hm_merge_u16_darks given stds[i] = hm_linearize_u16(frame_i,
 * icrf = std_table).val: both out_kind values, out_sum_w, flat_f64 with flat_std, row tiles, C = 1..4, N = 1..HM_MAX_FRAMES, every variant.
 * Without out_val the call is hm_merge_u16's sum-of-weights call. Statuses, an earlier rule wins:
 *   1. HM_EINVAL: hm_merge_u16's rule 1; then args->stds set, NULL std_table, no icrf_diff, no dw_lut; out_val without out_std; with
 *      darks_u16: args->darks_u8 set or no dark_min_dn.
 *   2. HM_EALIGN: a frame pointer, then a dark map pointer, that is not 2-byte aligned; then a std_table that is not 8-byte aligned.
 *   3. / 4. hm_merge_u16_darks's rules 3 and 4; the fit rule of variants 1 and 3 is that of a std call (with out_val).
 * Tables in LDS, n = 2^bit_depth: "tab=lds" holds {w, dw}[n] and {g, d * std_table}[n C]; "tab=mixed-wdwdg" - the std calls' 8 (2 + C) n
 * bytes - holds {w, dw}[n] and (d * std_table)[n C] with icrf gathered from global memory; "tab=mixed-wdw" and "tab=global" gather icrf,
 * icrf_diff and std_table from global memory at the masked index. The pair rule is hm_merge_u16's without the std frames.
 * hm_merge_u16_std_table_describe: hm_merge_u16_darks_describe's names with "std=lut" in place of "std=1".
 * hm_merge_u16_std_table_algorithmic_bytes: hm_merge_u16_darks's count of a std call without the 8 N bytes per element of std frames. */
int hm_merge_u16_std_table(const hm_merge_args* args /*[host]*/, const uint16_t* const* frames_u16 /*[host] N device pointers*/,
                           const uint16_t* const* darks_u16 /*[host] N device pointers or NULLs, or NULL*/, const double* std_table,
                           int bit_depth, void* stream);
int hm_merge_u16_std_table_describe(const hm_merge_args* args, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                                    const double* std_table, int bit_depth, char* buf, int buf_len);
int64_t hm_merge_u16_std_table_algorithmic_bytes(const hm_merge_args* args /*[host]*/, const uint16_t* const* darks_u16 /*[host] or NULL*/);
/* hm_linearize_u8 for uint16 DNs: idx = dn & (2^bit_depth - 1), tables of 2^bit_depth rows gathered from global memory; out_idx
 * (nullable, 2-byte aligned) receives the masked DN. bit_depth outside 9..16: HM_EINVAL; dn / out_idx not 2-byte aligned: HM_EALIGN. */
int hm_linearize_u16(const uint16_t* dn, const double* std, const double* icrf, const double* icrf_diff,
                     double* out_val, double* out_std, uint16_t* out_idx, int64_t n, int C, int lut_stride, int bit_depth, void* stream);
/* [host] hm_gaussian_weight_lut_host's formula on the grid v = k / (2^bit_depth - 1), 2^bit_depth entries each (bit_depth 8..16). */
int hm_gaussian_weight_lut_bits_host(int bit_depth, double* w_lut /*[host]*/, double* dw_lut /*[host]*/);

/* ------------------------------------------------------------------------------------------
 * Row 8 standalone - AbstractMeasurand.filter_larger_than_by_map (modules/measurand.py:543-557):
 * out = where(map >= min / map > thr, median_kxk(x, axes=(0,1), mode='reflect'), x), one call per array
 * (val: uint8 or float64; std: float64). map_f64 is compared with `> thr` in value units,
 * map_u8 with `>= min_dn` in DN.
 * ------------------------------------------------------------------------------------------ */
int hm_hot_pixel_filter_u8(const uint8_t* x, const uint8_t* map_u8, const double* map_f64,
                           int min_dn, double thr, int median_k, uint8_t* out,
                           int64_t H, int64_t W, int C, void* stream);
int hm_hot_pixel_filter_f64(const double* x, const uint8_t* map_u8, const double* map_f64,
                            int min_dn, double thr, int median_k, double* out,
                            int64_t H, int64_t W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row 9 standalone - flat-field ROI mean (modules/measurand.py:561-583) and normalize_by_map
 * (modules/measurand.py:585-604).
 * hm_roi_mean: per-channel mean over rows [x0,x1) x cols [y0,y1) of an H x W x C image, two-stage
 * deterministic reduction; `workspace` needs hm_roi_mean_workspace_bytes() bytes (the host build does not look at it); out_mean is C
 * float64 on the device.
 * ------------------------------------------------------------------------------------------ */
size_t hm_roi_mean_workspace_bytes(void);
int hm_roi_mean_u8(const uint8_t* img, int64_t H, int64_t W, int C,
                   int64_t x0, int64_t x1, int64_t y0, int64_t y1,
                   double* out_mean, void* workspace, void* stream);
int hm_roi_mean_f64(const double* img, int64_t H, int64_t W, int C,
                    int64_t x0, int64_t x1, int64_t y0, int64_t y1,
                    double* out_mean, void* workspace, void* stream);
int hm_normalize_by_map(const double* val, const double* std,
                        const uint8_t* flat_u8, const double* flat_f64, const double* flat_std,
                        const double* ff_mean /*[host] C*/, const double* ff_std_mean /*[host] C*/,
                        double* out_val, double* out_std, int64_t n, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row 10 - Measurand operators with first-order uncertainty propagation
 * (modules/measurand.py:106-279). Operands broadcast NumPy-style: `shape` is the broadcast result
 * shape (ndim <= 6), strides are in ELEMENTS with 0 on broadcast axes. s1 / s2 may be NULL (treated
 * as zeros, :121-124); out_std must be NULL iff both are NULL. Strides are non-negative and need not be dense (an operand may be a
 * strided slice of a larger allocation); a negative stride or extent, ndim outside 1..HM_MAX_DIMS and an unknown op are HM_EINVAL;
 * an extent of 0 returns HM_OK and writes nothing.
 * hm_unary_op LOG_10: std = s / (x * ln10) with ln10 = 0x1.26bb1bbb55515p+1, the float64 sum log(5) + log(2) of :277, as a literal.
 * ------------------------------------------------------------------------------------------ */
enum { HM_OP_ADD = 0, HM_OP_SUB = 1, HM_OP_MUL = 2, HM_OP_DIV = 3, HM_OP_POW = 4 };
enum { HM_UOP_NEG = 0, HM_UOP_LOG_E = 1, HM_UOP_LOG_10 = 2 };
#define HM_MAX_DIMS 6
int hm_binary_op(int op, const double* x1, const double* s1, const double* x2, const double* s2,
                 double* out_val, double* out_std, int ndim, const int64_t* shape /*[host]*/,
                 const int64_t* strides1 /*[host]*/, const int64_t* strides2 /*[host]*/, void* stream);
int hm_unary_op(int op, const double* x, const double* s, double* out_val, double* out_std,
                int64_t n, void* stream);

/* Measurand.__pow__ with a plain scalar exponent (modules/measurand.py:217-241; `S ** 2`, `** (1/2)` of the merge loop,
 * modules/exposure_series.py:343,394): out = x ** exponent, out_std = |exponent * x ** (exponent - 1)| * s (the exponent
 * has no uncertainty; its term of :237-238 is evaluated only where it is not +0). Exponents 2, 0.5, 1 and integers in
 * [-8, 8] avoid pow(). Exponent 0.5 is sqrt(x), the correctly rounded value, except where NumPy's pow() answers otherwise:
 * x = -inf gives +inf (x ** -0.5 of the std: +0) and x = -0.0 gives +0.0 (x ** -0.5: +inf). s / out_std are NULL together. */
int hm_pow_scalar(const double* x, const double* s /*nullable*/, double exponent, double* out_val, double* out_std /*nullable*/,
                  int64_t n, void* stream);

/* Measurand.extract (modules/measurand.py:352-373, `lib.take(val, dims, axis)`): out[o, k, i] = in[o, indices[k], i]
 * for the dense (outer, axis_len, inner) view of the array; axis=None in the reference is outer = inner = 1 on the
 * flattened array. std (nullable, with out_std) is taken with the same indices. Negative indices count from the end;
 * an index out of range returns HM_ESHAPE (np.take raises IndexError). At most HM_TAKE_MAX indices per call (more: HM_EUNSUPPORTED; the
 * host build takes any number). */
#define HM_TAKE_MAX 16
int hm_take_axis(const double* x, const double* s, double* out_val, double* out_std, int64_t outer, int64_t axis_len,
                 int64_t inner, const int64_t* indices /*[host]*/, int n_indices, void* stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY.md 8(f)-1 - linearity statistics (ExposureSeries.process_linearity, modules/exposure_series.py:421-446)
 *   hm_apply_thresholds     apply_thresholds (modules/measurand.py:375-428), in place: elements with
 *                           val < lower[c] or val > upper[c] become NaN in val and std; pass -inf / +inf for "none".
 *   hm_compute_difference   compute_difference (:620-655): abs = x - m*y, rel = abs / (m*y) and their std.
 *   hm_interpolate          interpolate (:657-681), std formula as written.
 *   hm_channel_statistics   compute_dimension_statistics (:318-350) over every axis but the last (the
 *                           axis=(0,1) call of exposure_series.py:446): NaN-ignoring mean / std per channel,
 *                           weighted by 1/std when std is given, plus error = nanmean(std). out is 3*C
 *                           float64 on the device: [mean | std | error]; error is NaN without std.
 * ------------------------------------------------------------------------------------------ */
#define HM_THRESHOLD_MAX_CHANNELS 32   /* hm_apply_thresholds: channels on the last axis (a slower one-element-per-thread kernel above HM_MAX_CHANNELS); more: HM_EUNSUPPORTED */
int hm_apply_thresholds(double* val, double* std /*nullable*/, const double* lower /*[host] C*/,
                        const double* upper /*[host] C*/, int64_t n, int C, void* stream);
int hm_compute_difference(const double* x, const double* sx, const double* y, const double* sy, double multiplier,
                          double* out_abs, double* out_abs_std, double* out_rel, double* out_rel_std,
                          int64_t n, void* stream);
int hm_interpolate(const double* x0, const double* s0, const double* x1, const double* s1,
                   double y0, double y1, double y, double* out, double* out_std, int64_t n, void* stream);
 /* hm_pair_statistics: ExposurePair.compute_difference + compute_stats(axis=(0,1)) fused
 * (modules/exposure_series.py:33-54, the per-pair body of process_linearity :443-446): the statistics of
 * the absolute and relative difference of two frames without writing the difference images.
 * out is 6*C float64 on the device: [abs mean | abs std | abs error | rel mean | rel std | rel error]. */
/* Status codes of the statistics entry points below, the same on both builds: n counts the elements of whole pixels, so n % C != 0 is
 * HM_EINVAL, as are n < 1, C outside 1..HM_MAX_CHANNELS, an extent < 1 or a product of extents above 2^48, a NULL val / out / workspace
 * (hm_axis_statistics: a NULL workspace only where hm_axis_statistics_workspace_bytes() is not 0; the host build, which needs none,
 * refuses a NULL workspace only in hm_channel_statistics, hm_pair_statistics and the all-pairs entries), n_pairs < 1, n_frames outside
 * 1..HM_MAX_FRAMES, a pair index outside the frames and `lower` without `upper`; a value or std buffer that is not 8-byte aligned is
 * HM_EALIGN. Every one of them returns before anything is launched or written.
 * The stds of one reduction line are expected to have one sign: all negative gives the reference's mean and (positive) std with
 * error = nanmean(std) < 0; with mixed signs sum(1 / std) can cancel and nothing is promised. */
size_t hm_pair_statistics_workspace_bytes(void);
int hm_pair_statistics(const double* x, const double* sx, const double* y, const double* sy, double multiplier,
                       int64_t n, int C, double* out, void* workspace, void* stream);

/* ExposureSeries.process_linearity (modules/exposure_series.py:421-446) for ALL pairs of a stack at once: pair p compares
 * frame pair_i[p] (short) with frame pair_j[p] (long) scaled by multipliers[p] (their exposure ratio) and gets the six
 * statistics of hm_pair_statistics at out[p * 6C ...]. One launch per HM_PAIRS_MAX pairs: a workgroup owns a run of elements,
 * each of its waves one pair, so a frame is read from HBM once per launch instead of once per pair it takes part in.
 * vals / stds: [host] arrays of n_frames device pointers (stds NULL = unweighted); pair_i / pair_j / multipliers: [host].
 * lower / upper: [host] C limits each, or both NULL. When given, hm_apply_thresholds(lower, upper) is applied to EVERY frame (and its
 * std) IN PLACE before it is compared - the apply_thresholds loop of process_linearity (modules/exposure_series.py:437-441), which leaves
 * the series' image sets thresholded - fused into the first launch's loads where the frames are staged through LDS (no separate pass
 * over the frames), by thresholding kernels otherwise; the result is the same either way. */
#define HM_PAIRS_MAX 16
size_t hm_pairs_statistics_workspace_bytes(int n_pairs);
int hm_pairs_statistics(const double* const* vals, const double* const* stds /*nullable*/, int n_frames,
                        const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                        int64_t n, int C, const double* lower /*nullable*/, const double* upper /*nullable*/,
                        double* out /*n_pairs * 6C*/, void* workspace, void* stream);
/* hm_pairs_statistics_dn: the same statistics straight from DN frames, without float64 value and std frames in memory. frames: [host] array
 * of n_frames device pointers to uint8 frames (bit_depth 8) or uint16 frames (bit_depth 9..16). For element e of a frame, channel
 * c = e % C and idx = DN & (2^bit_depth - 1):
 *     v = icrf[idx * C + c]
 *     s = icrf_diff[idx * C + c] * std_table[idx * C + c]         (only with a std_table: the weighted statistics)
 *     with lower / upper: v < lower[c] or v > upper[c] makes v (and s) NaN       (apply_thresholds, modules/measurand.py:375-428)
 * and the six statistics per pair and channel are hm_pairs_statistics' on these values: out as there, error NaN without a std_table, the
 * same bits as hm_pairs_statistics gives on frames hm_linearize_u8 / hm_linearize_u16 wrote. icrf, icrf_diff (nullable), std_table
 * (nullable; needs icrf_diff): device, (2^bit_depth, C) float64. The frames are NOT modified.
 * A small kernel writes the thresholded table into the workspace first; nothing is allocated and nothing synchronises (capturable).
 * variant: 0 the library's choice; 1 the staged kernel keeps the table in LDS beside its three stages; 2 it gathers from the workspace
 * table in global memory; -1 the per-wave kernel without staging for every launch. The staged kernel takes a launch (HM_PAIRS_MAX pairs)
 * when every frame is item-aligned (uint8: 2 bytes, uint16: 4 bytes), n_frames * 64 <= 2 * 64 * pairs and there are at most 21 streams
 * (n_frames, doubled with a std_table); the per-wave kernel takes every other launch, whatever the variant. Variant 0 puts the table in
 * LDS where table bytes (8 or 16 * 2^bit_depth * C) + 63 KiB <= 160 KiB.
 * Statuses, an earlier one winning: HM_EINVAL for hm_pairs_statistics' own rules (NULLs, n < 1, n % C, C, n_frames outside
 * 1..HM_MAX_FRAMES, n_pairs < 1, lower without upper), bit_depth outside 8..16, variant outside -1..2, std_table without icrf_diff, a NULL
 * frame; HM_EALIGN for a table that is not 8-byte aligned, then for a uint16 frame that is not 2-byte aligned; HM_EINVAL for a pair index
 * outside the frames; HM_EUNSUPPORTED for variant 1 with a table that does not fit. Every one returns before anything is launched or written.
 * hm_pairs_statistics_dn_describe writes the statistics kernel of each launch, joined by " + ", e.g.
 * "pairs_stats_dn_lds<dn=u16,bits=12,tab=global,std=1,ni=1>" or "pairs_stats_dn_wave<dn=u8,bits=8,std=0>" (the host build: a host name),
 * and launches nothing; frames_aligned: whether every frame is item-aligned. The statuses above that look at no pointer; HM_EINVAL for a
 * NULL or empty buf. */
size_t hm_pairs_statistics_dn_workspace_bytes(int n_pairs, int C, int bit_depth);
int hm_pairs_statistics_dn(const void* const* frames /*[host] n_frames device ptrs: uint8 (bit_depth 8) or uint16 (9..16)*/,
                           int n_frames, int bit_depth, const double* icrf, const double* icrf_diff /*nullable*/,
                           const double* std_table /*nullable; needs icrf_diff*/,
                           const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                           int64_t n, int C, const double* lower /*nullable*/, const double* upper /*nullable*/, int variant,
                           double* out /*n_pairs * 6C*/, void* workspace, void* stream);
int hm_pairs_statistics_dn_describe(int64_t n, int n_frames, int n_pairs, int C, int with_std, int bit_depth, int variant,
                                    int frames_aligned, char* buf, int buf_len);
/* hm_channel_histogram: compute_channel_histogram (modules/measurand.py:430-469) = np.histogram per channel on
 * [lo, hi] with `bins` equal-width bins (edges = np.linspace(lo, hi, bins + 1) on the device), non-finite values
 * skipped, optional weights 1/std with zero stds skipped. out is (C, bins) float64; channels not in
 * channel_mask stay 0. hm_channel_minmax gives the default range (min / max of the counted values). */
size_t hm_histogram_workspace_bytes(int bins, int C);
int hm_channel_minmax(const double* val, const double* std /*nullable*/, int64_t n, int C, double* out /*2*C*/,
                      void* workspace, void* stream);
int hm_channel_histogram(const double* val, const double* std /*nullable*/, int64_t n, int C, int channel_mask,
                         const double* edges, int bins, double lo, double hi, double* out, void* workspace, void* stream);
/* ExposurePair.process_linearity_distribution (modules/exposure_series.py: compute_difference, then compute_channel_histogram of the
 * absolute and of the relative difference) for ALL pairs of a stack at once, without the difference images: arguments as
 * hm_pairs_statistics. Kind 0 is the absolute, kind 1 the relative difference. For pair p, kind k and channel c the histogram equals
 * hm_compute_difference(vals[pair_i[p]], ..., vals[pair_j[p]], ..., multipliers[p]) followed by hm_channel_histogram of that difference
 * image (with stds: and of its std image) on edges[p][k][c][0 .. bins], lo the first and hi the last edge: the same difference
 * expressions, the same counting rule. A (pair, kind, channel) whose last edge is not above its first counts nothing.
 * edges: device, (n_pairs, 2, C, bins + 1) float64; out: device, (n_pairs, 2, C, bins) float64, channels outside channel_mask 0.0.
 * lower / upper: [host] C limits each, or both NULL: apply_thresholds on the values AS READ - a value outside its channel's limits counts
 * as NaN together with its std. The frames are NOT modified (hm_pairs_statistics stays the one entry point that thresholds in place).
 * hm_pairs_minmax: np.histogram's default range, the min and max hm_channel_minmax would give on each difference image, out (n_pairs, 2,
 * C, 2) = min, max; (+inf, -inf) where nothing counts.
 * One launch per group of pairs whose histograms fit the 160 KiB of LDS of a CU (2 * C * bins * 8 bytes per pair; at most HM_PAIRS_MAX).
 * Status codes: those of the statistics block above; in addition bins < 1, bins > HM_PAIRS_HIST_MAX_BINS, channel_mask with bits at or
 * above C (or negative) and a NULL edges are HM_EINVAL. Every check returns before anything is launched, written or dereferenced.
 * The workspace covers both calls. */
#define HM_PAIRS_HIST_MAX_BINS 2048
size_t hm_pairs_histogram_workspace_bytes(int n_pairs, int bins, int C);
int hm_pairs_minmax(const double* const* vals, const double* const* stds /*nullable*/, int n_frames,
                    const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                    int64_t n, int C, const double* lower /*nullable*/, const double* upper /*nullable*/,
                    double* out /* device: (n_pairs, 2 kinds, C, 2) = min, max */, void* workspace, void* stream);
int hm_pairs_histogram(const double* const* vals, const double* const* stds /*nullable*/, int n_frames,
                       const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                       int64_t n, int C, int channel_mask, const double* lower /*nullable*/, const double* upper /*nullable*/,
                       const double* edges /* device: (n_pairs, 2, C, bins + 1) */, int bins,
                       double* out /* device: (n_pairs, 2, C, bins) */, void* workspace, void* stream);
/* hm_pairs_minmax_dn / hm_pairs_histogram_dn: the same distributions straight from DN frames, without float64 value and std frames in
 * memory. frames, bit_depth, icrf, icrf_diff, std_table, lower / upper and the per-element semantics are hm_pairs_statistics_dn's:
 * idx = DN & (2^bit_depth - 1), v = icrf[idx * C + c], s = icrf_diff[idx * C + c] * std_table[idx * C + c], a value outside
 * lower[c]..upper[c] NaN together with its std; the frames are NOT modified. Per pair, kind and channel the histogram and the min / max
 * are those hm_pairs_histogram / hm_pairs_minmax give on frames hm_linearize_u8 / hm_linearize_u16 wrote from the same tables, with the
 * same thresholds: the same difference expressions, the same counting rule, the same bounded bin index; a (pair, kind, channel) whose
 * last edge is not above its first counts nothing. A std_table means weighted histograms (weights of the same float64 bits), none means
 * unweighted ones. edges, out, channel_mask: as hm_pairs_histogram.
 * One small kernel writes the thresholded table into the workspace behind the partials; nothing is allocated and nothing synchronises
 * (capturable). The workspace (hm_pairs_histogram_dn_workspace_bytes) covers both calls. The DN loads are per element: any frame
 * alignment hm_pairs_statistics_dn accepts is served by the one kernel form.
 * variant: 0 the library's choice; 1 the table in LDS beside the histograms; 2 gathered from the workspace table in global memory.
 * With per_pair = 2 * C * bins * 8 bytes and T = (8, with a std_table 16) * 2^bit_depth * C bytes a launch takes
 * min(HM_PAIRS_MAX, (160 KiB - (table in LDS ? T : 0)) / per_pair) pairs, the launches of a call of equal size. Variant 0 takes the LDS
 * table only where it costs the histograms nothing: the call's pairs need no more launches with it, and a CU holds as many workgroups of
 * the launch with it as without (min(160 KiB / LDS of the workgroup, 32 / waves of the workgroup, 4)). hm_pairs_minmax_dn holds
 * nothing else in LDS: its table goes there whenever T <= 160 KiB, unless variant 2.
 * Statuses, an earlier one winning: hm_pairs_statistics_dn's up to and including the pair indices, with a variant outside 0..2
 * HM_EINVAL; then (histogram) bins < 1, bins > HM_PAIRS_HIST_MAX_BINS, channel_mask with bits at or above C (or negative), NULL edges:
 * HM_EINVAL; then HM_EUNSUPPORTED for variant 1 where not one pair's histograms fit beside the table (min / max: T > 160 KiB). Every
 * one returns before anything is launched, written or dereferenced.
 * hm_pairs_histogram_dn_describe writes the histogram kernel of each launch, joined by " + ", e.g.
 * "pairs_hist_dn<dn=u16,bits=12,tab=global,std=1,np=8,wpp=2>" (np pairs, wpp waves per pair; the host build: a host name) and launches
 * nothing. The statuses above that look at no pointer; HM_EINVAL for a NULL or empty buf. */
size_t hm_pairs_histogram_dn_workspace_bytes(int n_pairs, int bins, int C, int bit_depth);
int hm_pairs_minmax_dn(const void* const* frames /*[host] n_frames device ptrs: uint8 (bit_depth 8) or uint16 (9..16)*/,
                       int n_frames, int bit_depth, const double* icrf, const double* icrf_diff /*nullable*/,
                       const double* std_table /*nullable; needs icrf_diff*/,
                       const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                       int64_t n, int C, const double* lower /*nullable*/, const double* upper /*nullable*/, int variant,
                       double* out /* device: (n_pairs, 2 kinds, C, 2) = min, max */, void* workspace, void* stream);
int hm_pairs_histogram_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff /*nullable*/,
                          const double* std_table /*nullable; needs icrf_diff*/,
                          const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                          int64_t n, int C, int channel_mask, const double* lower /*nullable*/, const double* upper /*nullable*/,
                          const double* edges /* device: (n_pairs, 2, C, bins + 1) */, int bins, int variant,
                          double* out /* device: (n_pairs, 2, C, bins) */, void* workspace, void* stream);
int hm_pairs_histogram_dn_describe(int64_t n, int n_frames, int n_pairs, int C, int with_std, int bit_depth, int bins, int variant,
                                   char* buf, int buf_len);
size_t hm_channel_statistics_workspace_bytes(void);
int hm_channel_statistics(const double* val, const double* std /*nullable*/, int64_t n, int C,
                          double* out, void* workspace, void* stream);
/* compute_dimension_statistics over ANY axis (modules/measurand.py:318-350 pass `axis` to NumPy's nan-reductions): the array is the
 * dense (outer, axis_len, inner) block and is reduced over its middle dimension; out_mean / out_std / out_err are outer * inner
 * float64 each (out_err nullable; NaN without std). Several reduced axes = their product when adjacent (two separate groups:
 * hm_axis_statistics2; three or more: the caller brings them together with a layout copy). workspace: hm_axis_statistics_workspace_bytes() bytes (0 = none needed). */
size_t hm_axis_statistics_workspace_bytes(int64_t outer, int64_t axis_len, int64_t inner);
int hm_axis_statistics(const double* val, const double* std /*nullable*/, int64_t outer, int64_t axis_len, int64_t inner,
                       double* out_mean, double* out_std, double* out_err /*nullable*/, void* workspace, void* stream);
/* The same over TWO separate groups of reduced axes (e.g. axis = (0, 2) of an H x W x C image: statistics per column over rows and
 * channels): the array is the dense (outer, a1, mid, a2, inner) block, reduced over a1 AND a2 in place - no layout copy; outputs are
 * outer * mid * inner float64 each. workspace: hm_axis_statistics2_workspace_bytes() bytes, always required on the device build. */
size_t hm_axis_statistics2_workspace_bytes(int64_t outer, int64_t a1, int64_t mid, int64_t a2, int64_t inner);
int hm_axis_statistics2(const double* val, const double* std /*nullable*/, int64_t outer, int64_t a1, int64_t mid, int64_t a2, int64_t inner,
                        double* out_mean, double* out_std, double* out_err /*nullable*/, void* workspace, void* stream);
/* compute_difference / interpolate on operands that BROADCAST against each other (the reference applies NumPy broadcasting,
 * modules/measurand.py:621-681): `shape` is the broadcast result shape (ndim <= HM_MAX_DIMS), strides are in ELEMENTS with 0 on
 * broadcast axes (as hm_binary_op, with the same HM_EINVAL for negative strides or extents and HM_OK for an extent of 0); an operand
 * and its std share strides. Outputs are dense arrays of that shape. */
int hm_compute_difference_bcast(const double* x, const double* sx, const double* y, const double* sy, double multiplier,
                                double* out_abs, double* out_abs_std, double* out_rel, double* out_rel_std,
                                int ndim, const int64_t* shape /*[host]*/, const int64_t* strides_x /*[host]*/,
                                const int64_t* strides_y /*[host]*/, void* stream);
int hm_interpolate_bcast(const double* x0, const double* s0, const double* x1, const double* s1, double y0, double y1, double y,
                         double* out, double* out_std, int ndim, const int64_t* shape /*[host]*/, const int64_t* strides0 /*[host]*/,
                         const int64_t* strides1 /*[host]*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Upstream producer: welford_algorithm, modules/video_processing.py:161-219.
 *   hm_welford_update    folds n_frames uint8 frames (each n_elems = H*W*C, HWC) into the running float64
 *                        mean / m2 (m2 nullable = use_std False), in frame order:
 *                          f = icrf[dn, c] (:200-201; icrf (256, C) float64, nullable) or dn / 255 (:203);
 *                          delta = f - mean; mean += delta / n; m2 += delta * (f - mean)   (:205-208)
 *                        count_before = frames already folded (the caller keeps the count). mean / m2 must be
 *                        zero-initialised by the caller before the first call (:181-184).
 *   hm_welford_finalize  mean frame = around(mean * 255) as uint8 (:210-211); std frame =
 *                        around(sqrt(m2 / (count - 1)) / sqrt(count)) as uint8 (:214-215, as written).
 *                        out_std needs count >= 2 (HM_EINVAL otherwise).
 *   hm_welford_algorithmic_bytes   n_elems * (n_frames + 16 or 32): each frame byte read once, the state
 *                        read and written once per launch.
 * ------------------------------------------------------------------------------------------ */
int hm_welford_update(const void* const* frames /*[host] n_frames device ptrs*/, int n_frames, int64_t count_before,
                      const double* icrf /*nullable*/, double* mean, double* m2 /*nullable*/,
                      int64_t n_elems, int C, void* stream);
int hm_welford_finalize(const double* mean, const double* m2 /*nullable*/, int64_t count,
                        uint8_t* out_mean /*nullable*/, uint8_t* out_std /*nullable*/, int64_t n_elems, void* stream);
int64_t hm_welford_algorithmic_bytes(int n_frames, int with_m2, int64_t n_elems);

/* ... on uint16 frames of 9- to 16-bit cameras, M = 2^bit_depth - 1. Everything not named here is hm_welford_update's /
 * hm_welford_finalize's: the layouts, the running-state convention, the operation sequence, no allocation, no host synchronisation.
 *   frames     n_frames uint16 HWC frames, 2-byte aligned. A DN's value is f = icrf[DN & M, c] (icrf (2^bit_depth, C) float64) or, with a
 *              NULL icrf, (DN & M) / M with the IEEE division; the mask is applied before every table access (hm_merge_u16's convention).
 *              The device build folds two elements per lane when every frame is 4-byte aligned and mean / m2 are 16-byte aligned, and one
 *              per lane otherwise: the same bits.
 *   variant    where the device kernel takes f from - 0: the library's choice; 1: a table in LDS (the ICRF, 8 * 2^bit_depth * C bytes, or
 *              without an ICRF the column DN / M, 8 * 2^bit_depth bytes); 2: computed in the lane, without an ICRF only; 3: gathered from
 *              the ICRF in global memory, with an ICRF only. Fit rule: the LDS table may take 128 KiB - with an ICRF C = 1 up to 14 bits,
 *              C = 2 up to 13, C = 3 and 4 up to 12; without one up to 14 bits. The library's choice is LDS where the table fits, else
 *              2 (no ICRF) or 3 (ICRF). The placements give the same bits. The host build checks variant and ignores it.
 *   Statuses of hm_welford_update_u16, an earlier one winning: HM_EINVAL for n_frames outside 0..HM_MAX_FRAMES, a negative count_before or
 *   n_elems, bit_depth outside 9..16 or variant outside 0..3; HM_EUNSUPPORTED for count_before beyond 2^40; HM_ESHAPE for C outside
 *   1..HM_MAX_CHANNELS, then for n_elems no multiple of C; n_frames == 0 or n_elems == 0 returns HM_OK with no pointer looked at;
 *   HM_EUNSUPPORTED for a forced variant that does not exist for the call or whose table does not fit; HM_EINVAL for NULL frames, mean or
 *   frames[k]; HM_EALIGN for a frame that is not 2-byte aligned.
 *   hm_welford_finalize_u16   out_mean = around(mean * M) as uint16; out_std = around(sqrt(m2 / (count - 1)) / sqrt(count)) as uint16 (as
 *              written: not rescaled); both nullable. Rounding as np.around(x).astype(uint16) where that is defined; NaN and |x| >= 9.2e18
 *              give 0, anything else the low 16 bits of the rounded 64-bit integer. hm_welford_finalize's statuses, bit_depth outside
 *              9..16 with the first (HM_EINVAL), and last HM_EALIGN for an output that is not 2-byte aligned.
 *   hm_welford_u16_algorithmic_bytes   n_elems * (2 * n_frames + 16 or 32).
 *   hm_welford_update_u16_describe writes the name of the kernel such a call would launch, e.g. "k_welford_u16<m2=1,tab=lds,bits=12>"
 *   (tab = lds, computed or global; the host build: a host name), and launches nothing; hm_welford_update_u16's statuses up to the
 *   second HM_EUNSUPPORTED, an empty name where there is nothing to do, HM_EINVAL for a NULL or empty buf. */
int hm_welford_update_u16(const void* const* frames /*[host] n_frames device ptrs*/, int n_frames, int64_t count_before,
                          const double* icrf /*nullable, (2^bit_depth, C)*/, double* mean, double* m2 /*nullable*/,
                          int64_t n_elems, int C, int bit_depth, int variant, void* stream);
int hm_welford_finalize_u16(const double* mean, const double* m2 /*nullable*/, int64_t count, int bit_depth,
                            uint16_t* out_mean /*nullable*/, uint16_t* out_std /*nullable*/, int64_t n_elems, void* stream);
int64_t hm_welford_u16_algorithmic_bytes(int n_frames, int with_m2, int64_t n_elems);
int hm_welford_update_u16_describe(int64_t n_elems, int n_frames, int C, int with_icrf, int with_m2, int bit_depth, int variant,
                                   char* buf, int buf_len);

/* ------------------------------------------------------------------------------------------
 * Camera noise profiles and the per-DN STD table: compute_noise_profiles, _calculate_STD and clean_data_edges,
 * modules/video_processing.py:12-133 (the input of ImageSet.calculate_numerical_STD, modules/image_set.py).
 *   profiles   (256, 256, C) int64: profiles[m, f, c] counts the elements of channel c whose mean-frame DN is m and
 *              whose frame DN is f (:77-106, np.add.at); the caller zero-initialises it before the first update and
 *              every update adds to it (the running-state convention of hm_welford_update)
 *   hm_noise_profile_update   adds n_frames uint8 frames (each n_elems = H*W*C, HWC) against the uint8 mean frame
 *              `mean` (n_elems). workspace: hm_noise_profile_workspace_bytes() bytes (0 at this version: NULL is fine).
 *              C > HM_MAX_CHANNELS -> HM_EUNSUPPORTED.
 *   hm_noise_profile_algorithmic_bytes   n_elems * (n_frames + 1) + 2 * 256 * 256 * C * 8: each frame byte and the mean
 *              read once, the profile read and written once.
 *   hm_noise_profile_std      out_std (256, C) float64 [level][c]: for each row, over its non-zero bins h with the edges
 *              `edges` (256 float64, the caller's np.linspace(0, 1, 256)), mean = sum(h edges) / sum(h) and
 *              std = sqrt(sum((edges - mean)^2 h) / sum(h)) (:109-133); NaN for a row without counts.
 *   hm_noise_profile_clean_edges   the reference's four integer passes over every (row, channel) distribution, centred
 *              at the row's level (:12-74), in place; bit-exact.
 * ------------------------------------------------------------------------------------------ */
size_t hm_noise_profile_workspace_bytes(int64_t n_elems, int C);
int64_t hm_noise_profile_algorithmic_bytes(int n_frames, int64_t n_elems, int C);
int hm_noise_profile_update(const void* const* frames /*[host] n_frames device ptrs*/, int n_frames, const uint8_t* mean,
                            int64_t n_elems, int C, int64_t* profiles, void* workspace /*nullable when 0 bytes*/,
                            int64_t workspace_bytes, void* stream);
int hm_noise_profile_std(const int64_t* profiles, int C, const double* edges, double* out_std, void* stream);
int hm_noise_profile_clean_edges(int64_t* profiles, int C, void* stream);

/* ... the per-DN STD table of 9- to 16-bit cameras, M = 2^bit_depth - 1. The (2^b, 2^b, C) joint histogram does not scale to these depths
 * (96 GiB at 16 bits); _calculate_STD reduces each of its rows to a count, a mean and a centred second moment, and three integers per
 * (mean level, channel) carry exactly that.
 *   moments    (2^bit_depth, C, 3) int64, indexed [level][c][k]. With m = mean[e] & M, f = frame[e] & M (the mask first: hm_merge_u16's
 *              convention), c = e % C and d = f - m, every frame and element e adds 1 to [m][c][0], d to [m][c][1] and d * d to [m][c][2].
 *              The caller zero-initialises it before the first update and every update adds to it (hm_noise_profile_update's running-state
 *              convention). The sums are integers modulo 2^64: exact, and independent of the order of the adds, while count * D * D < 2^63
 *              for every level, |d| <= D (D <= M; D = 65535 allows 2^31 frame-elements on one level, D = 1023 allows 2^43).
 *   hm_noise_moments_update_u16   adds n_frames uint16 frames (each n_elems = H*W*C, HWC, 2-byte aligned) against the uint16 mean frame
 *              `mean`. No allocation, no host synchronisation, no workspace; capturable.
 *   variant    where the device kernel keeps the triples of a launch - 0: the library's choice; 1: every workgroup privatises the whole
 *              table in LDS (a u32 element count, an i64 sum of d and a u64 sum of d * d: 20 bytes per level and channel) and flushes its
 *              non-zero entries once per launch; 2: every lane adds its triples to `moments` with 8-byte global atomics; 3: a hashed
 *              window of 4096 (level, channel) slots in LDS over the levels a workgroup meets, flushed after every pass over 8192 elements,
 *              a triple whose slot another level holds going to the global atomics - any depth. Fit rule: the LDS table,
 *              20 * 2^bit_depth * C bytes, may take 128 KiB - C = 1 up to 12 bits, C = 2 and 3 up to 11, C = 4 up to 10. The library's
 *              choice is 1 where the table fits, else 3. The placements give the same integers. The host build checks variant and
 *              ignores it.
 *   Statuses of hm_noise_moments_update_u16, an earlier one winning (hm_noise_profile_update's order): HM_EINVAL for n_frames outside
 *   0..HM_MAX_FRAMES, a negative n_elems, C < 1, bit_depth outside 9..16 or variant outside 0..3; HM_EUNSUPPORTED for C > HM_MAX_CHANNELS;
 *   HM_ESHAPE for n_elems no multiple of C; HM_EUNSUPPORTED for a forced variant 1 whose table does not fit; HM_EINVAL for NULL frames,
 *   mean, moments or frames[k]; HM_EALIGN for a frame or a mean that is not 2-byte aligned; then n_frames == 0 or n_elems == 0 returns HM_OK.
 *   hm_noise_moments_algorithmic_bytes   2 * n_elems * (n_frames + 1) + 2 * 24 * 2^bit_depth * C: each frame and the mean read once, the
 *              moments read and written once.
 *   hm_noise_moments_update_u16_describe writes the name of the kernel such a call would launch, e.g. "k_noise_moments_u16<C=3,tab=lds,bits=11>"
 *   (tab = lds, global or window; the host build: a host name), and launches nothing; the statuses above up to the second HM_EUNSUPPORTED, an empty
 *   name where there is nothing to do, HM_EINVAL for a NULL or empty buf.
 *   hm_noise_moments_std      out_std (2^bit_depth, C) float64 [level][c]: with n, S1, S2 of a level, std = sqrt(n * S2 - S1 * S1) / n / M.
 *              The numerator is formed exactly in 128-bit integers and converted to FP64 half by half; the value is at most five FP64
 *              roundings from the exact one. n == 0 gives NaN (hm_noise_profile_std's row without counts); so do moments that no data
 *              set has (n < 0, n * S2 < S1 * S1). On the DN grid k / M this is hm_noise_profile_std's quantity. HM_EINVAL for a NULL
 *              pointer, C < 1 or bit_depth outside 9..16, then HM_EUNSUPPORTED for C > HM_MAX_CHANNELS. */
int64_t hm_noise_moments_algorithmic_bytes(int n_frames, int64_t n_elems, int C, int bit_depth);
int hm_noise_moments_update_u16(const void* const* frames /*[host] n_frames device ptrs*/, int n_frames, const uint16_t* mean,
                                int64_t n_elems, int C, int bit_depth, int64_t* moments, int variant, void* stream);
int hm_noise_moments_update_u16_describe(int64_t n_elems, int n_frames, int C, int bit_depth, int variant, char* buf, int buf_len);
int hm_noise_moments_std(const int64_t* moments, int C, int bit_depth, double* out_std, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weighted Gaussian kernel density estimates: NumpyMeasurand.compute_kernel_density_estimate, modules/measurand.py:716-761
 * (and CupyMeasurand's, modules/cupy_measurand.py:88-137): scipy.stats.gaussian_kde(values, 'silverman', weights).evaluate(x_range)
 * for ONE channel `channel` of HWC float64 data `val` (n_elems = n * C, any C >= 1), `std` nullable (same layout).
 *   counted    elements with a finite value and, with std, std != 0 (:741-749); weight w = 1 / std, or 1 without std
 *   workspace  device memory of hm_kde_workspace_bytes(n_elems, C, m) bytes, owned by the caller, shared by both calls (the host
 *              build needs none: 0 bytes, NULL is fine). No allocation, no host synchronisation, no float atomics: the
 *              reductions run in a fixed order, so the same inputs give the same bits on every run and under graph replay.
 *   hm_kde_moments   moments[0..10] (device, 11 float64): count, sum w, sum w^2, sum w x, min x, max x, #non-finite w, #w > 0,
 *              #w < 0, x_bar = sum w x / sum w, sum w (x - x_bar)^2 - all over the counted elements. Two stream-ordered passes;
 *              the second reads x_bar from moments[9] on the device.
 *   hm_kde_evaluate  out[j] = scale * sum_i w_i exp(-(x_i / h - y_j / h)^2 / 2) for the m grid points y = grid (device);
 *              the caller passes h = sqrt(cov) * silverman_factor and scale = (2 pi)^(-1/2) / h / sum w (scipy's norm and
 *              weight normalisation). h must be > 0 and finite, scale finite.
 * ------------------------------------------------------------------------------------------ */
#define HM_KDE_MOMENTS 11
size_t hm_kde_workspace_bytes(int64_t n_elems, int C, int m);
int hm_kde_moments(const double* val, const double* std /*nullable*/, int64_t n_elems, int C, int channel, double* moments,
                   void* workspace, int64_t workspace_bytes, void* stream);
int hm_kde_evaluate(const double* val, const double* std /*nullable*/, int64_t n_elems, int C, int channel, double h, double scale,
                    const double* grid, int m, double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * ICRF-calibration energy function: _energy_function + analyze_linearity,
 * modules/ICRF_calibration_exposure.py:66-145,148-201, for n_candidates ICRFs of one channel per launch.
 *   dn         (n_pixels, n_frames) uint8: the reference's (X, Y, N) channel stack (:257-277), frames ascending
 *              in exposure; std (same shape, float64) nullable = use_std False
 *   exposures  [host] n_frames exposure values (:282)
 *   icrf       (n_candidates, 256) float64 on the device: each row already shifted to ICRF[255] = 1, ICRF[0] = 0
 *              (:166-167); valid (n_candidates uint8, nullable): 0 marks a candidate the host rejected
 *              (range / monotonicity tests :173-179): its energy is +inf and no pixel work is done
 *   lower, upper   DN limits (:181-182): values outside [icrf[lower], icrf[upper]] are ignored (:96-97)
 *   use_relative   analyze_linearity's flag (the energy function passes True, :192-193)
 *   out_pairs  (n_candidates, n_frames (n_frames-1)/2) float64, nullable: the per-pair results in
 *              np.triu_indices(N, 1) order (:141-143); out_energy (n_candidates): nanmean over the pairs,
 *              +inf where that is NaN (:196-198)
 * ------------------------------------------------------------------------------------------ */
size_t hm_linearity_energy_workspace_bytes(int64_t n_pixels, int n_frames, int n_candidates);
int hm_linearity_energy(const uint8_t* dn, const double* std /*nullable*/, const double* exposures /*[host]*/,
                        const double* icrf, const uint8_t* valid /*nullable*/, int n_candidates,
                        int lower, int upper, int use_relative, int64_t n_pixels, int n_frames,
                        double* out_pairs /*nullable*/, double* out_energy, void* workspace, void* stream);

/* ... on uint16 DN stacks of 9- to 16-bit cameras: candidate ICRFs of 2^bit_depth rows. Everything not named here is
 * hm_linearity_energy's: the layouts, the `valid` convention, pair order, +inf and NaN behaviour, no allocation, no host synchronisation;
 * hm_linearity_energy_workspace_bytes(n_pixels, n_frames, n_candidates) sizes the workspace.
 *   dn         (n_pixels, n_frames) uint16, 2-byte aligned; a DN's table index is DN & (2^bit_depth - 1), applied before every
 *              table access (hm_merge_u16's convention)
 *   icrf       (n_candidates, 2^bit_depth) float64; lower, upper: DNs of that depth, 0 .. 2^bit_depth - 1
 *   variant    where a workgroup reads the candidate's row from - 0: the library's choice; 1: a copy in LDS (the row of 8 * 2^bit_depth
 *              bytes and the kernels' reduction scratch must fit the CU's 160 KiB: up to 14 bits); 2: gathered from global memory
 *              (every depth). The placements give the same bits. The host build checks it and ignores it.
 *   The sums are formed in hm_linearity_energy's order: an 8-bit problem embedded at depth b (DN << (b - 8), the 256 entries at rows
 *   k << (b - 8), limits shifted alike) gives hm_linearity_energy's out_energy and out_pairs bit for bit.
 *   Statuses, an earlier one winning: HM_EINVAL for a negative count, bit_depth outside 9..16 or variant outside 0..2; HM_ESHAPE for
 *   n_frames outside 2..HM_MAX_FRAMES; HM_EINVAL for a limit outside 0 .. 2^bit_depth - 1; n_candidates == 0 returns HM_OK with no pointer
 *   looked at; HM_EUNSUPPORTED for more than 65535 candidates and for variant 1 where the row does not fit; HM_EINVAL for NULL dn,
 *   exposures, icrf or out_energy; HM_EALIGN for a dn that is not 2-byte aligned; (device build) HM_EINVAL for a NULL workspace.
 *   hm_linearity_energy_u16_describe writes the name of the pixel kernel such a call would launch, e.g.
 *   "k_energy_pixel_u16<N=7,std=1,lut=lds,bits=12>" or "k_energy_partial_u16<std=0,lut=global,bits=16>(N=9)" (the host build: a host
 *   name), and launches nothing; the same statuses up to HM_EUNSUPPORTED, HM_EINVAL for a NULL or empty buf. */
int hm_linearity_energy_u16(const uint16_t* dn, const double* std /*nullable*/, const double* exposures /*[host]*/,
                            const double* icrf /*(n_candidates, 2^bit_depth)*/, const uint8_t* valid /*nullable*/, int n_candidates,
                            int lower, int upper, int use_relative, int64_t n_pixels, int n_frames, int bit_depth, int variant,
                            double* out_pairs /*nullable*/, double* out_energy, void* workspace, void* stream);
int hm_linearity_energy_u16_describe(int64_t n_pixels, int n_frames, int n_candidates, int with_std, int bit_depth, int variant,
                                     char* buf, int buf_len);

/* ------------------------------------------------------------------------------------------
 * ICRF-calibration differential evolution, one generation per call: the solver loop of calibration(),
 * modules/ICRF_calibration_exposure.py:288-369 (SciPy's DifferentialEvolutionSolver with strategy 'currenttobest1bin',
 * mutation (0, 1.95), recombination 0.4, tol 0.01, deferred updating), restated so that it needs no generator state:
 * every random number is a pure function of (seed, generation, member, draw index).
 *
 *   mix64(z)   the splitmix64 step: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *              z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31                       (uint64, wrapping)
 *   key_g      mix64(seed ^ mix64(g))
 *   U(g, i, k) (mix64(key_g + ((i + 1) << 20) + k) >> 11) * 2^-53                               in [0, 1)
 *
 * Member i of the S members holds P parameters u in SciPy's scaled coordinates [0, 1]; x = lo + u (hi - lo).
 * Generation 0 evaluates the population as it is (the trial IS the member, no draws) and accepts every energy.
 * Generation g >= 1, with b the best member (lowest energy, ties to the lowest index) of the population before it:
 *   dither     F = mutation_lo + (mutation_hi - mutation_lo) U(g, S, 0)
 *   picks      a = floor(U(g,i,0) (S-1)), r0 = a + (a >= i);  c = floor(U(g,i,1) (S-2)), lo2 < hi2 the sorted {i, r0},
 *              c += (c >= lo2), then c += (c >= hi2), r1 = c          (r0, r1 distinct, both different from i)
 *   trial      v = u_i + F (u_b - u_i + u_r0 - u_r1);  fill = floor(U(g,i,2) P);  component j is v_j where
 *              U(g,i,3+j) < recombination or j == fill, else u_i[j];  a component outside [0, 1] becomes U(g,i,3+P+j)
 *   candidate  row = mean_icrf + pca @ x, row += 1 - row[255], row[0] = 0 (:166-167); valid unless an entry is > 1 or < 0
 *              or the row is not strictly increasing (:173-179); the energy of an invalid row is +inf
 *   energy     hm_linearity_energy on the S trial rows (use_relative = 1)
 *   selection  the trial replaces member i where E_trial <= E_i (all members see the population of before: deferred)
 *   statistics best index, mean(E), population std(E) (ddof 0) - fixed-order tree reductions
 *   stop       after every EVEN generation g >= 2 (the reference loop advances two generations per pass, :351):
 *              HM_DE_STOP_CONVERGED  all E finite and std(E) <= tol |mean(E)|        (solver.converged(), :356)
 *              HM_DE_STOP_ENERGY     E_best < energy_limit                           (:356)
 *              and after any generation g >= max_generations: HM_DE_STOP_MAX
 *   Once status[HM_DE_STOP] != 0 a call changes nothing any more: calls may be issued (or replayed from a graph) in
 *   batches of any size without the result depending on the batch size.
 *
 * State, all caller-owned device memory (host memory in the host build), nothing else is kept between calls:
 *   population (S, P), energies (S), trial (S, P), trial_energies (S), icrf (S, 256) float64; valid (S) uint8;
 *   status     HM_DE_STATUS_WORDS 64-bit words, zeroed by the caller before generation 0: int64 in GENERATION (the
 *              generation the NEXT call runs; advanced by the last kernel of a call), BEST_INDEX, STOP, EVALUATIONS;
 *              float64 bit patterns in BEST_ENERGY, MEAN, STD
 *   mean_icrf (256), pca (256, P) row-major, lower_limits (P), upper_limits (P): float64 on the device
 *   dn, std, exposures [host], n_pixels, n_frames, lower, upper: as for hm_linearity_energy
 *   workspace  hm_de_workspace_bytes(n_pixels, n_frames, pop_size) bytes
 * 4 <= pop_size <= HM_DE_MAX_POP, 1 <= n_params <= HM_DE_MAX_PARAMS, 0 <= mutation_lo <= mutation_hi < 2,
 * 0 <= recombination <= 1, tol >= 0. No allocation, no host synchronisation, no float atomics: the same state gives
 * the same bits on every run, launched eagerly or replayed from a graph.
 * ------------------------------------------------------------------------------------------ */
#define HM_DE_MAX_POP 1024
#define HM_DE_MAX_PARAMS 32
#define HM_DE_STATUS_WORDS 8
#define HM_DE_GENERATION 0
#define HM_DE_BEST_INDEX 1
#define HM_DE_STOP 2
#define HM_DE_EVALUATIONS 3
#define HM_DE_BEST_ENERGY 4
#define HM_DE_MEAN 5
#define HM_DE_STD 6
#define HM_DE_STOP_CONVERGED 1
#define HM_DE_STOP_ENERGY 2
#define HM_DE_STOP_MAX 4
size_t hm_de_workspace_bytes(int64_t n_pixels, int n_frames, int pop_size);
int hm_de_generation(double* population, double* energies, double* trial, double* trial_energies, double* icrf,
                     uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca,
                     const double* lower_limits, const double* upper_limits, const uint8_t* dn,
                     const double* std /*nullable*/, const double* exposures /*[host]*/, int64_t n_pixels, int n_frames,
                     int lower, int upper, int pop_size, int n_params, int64_t seed, int64_t max_generations,
                     double mutation_lo, double mutation_hi, double recombination, double tol, double energy_limit,
                     void* workspace, void* stream);

/* ... on a uint16 DN stack of a 9- to 16-bit camera: hm_de_generation's specification - the status block, the stop rule, the random
 * numbers U(g, i, k), deferred selection, evaluation at generation 0, the contract - with three differences:
 *   rows       R = 2^bit_depth entries: mean_icrf (R), pca (R, P) row-major, icrf (S, R); candidate: row = mean_icrf + pca @ x,
 *              row += 1 - row[R - 1], row[0] = 0; valid unless an entry is > 1 or < 0 or the row is not strictly increasing
 *   limits     lower, upper are DNs of that depth, 0 .. R - 1; dn is (n_pixels, n_frames) uint16, 2-byte aligned, indexed DN & (R - 1)
 *   energy     hm_linearity_energy_u16 on the S trial rows (use_relative = 1), `variant` handed to it unchanged (0: the library's choice,
 *              1: the row in LDS, 2: gathered from global memory; the result does not depend on it)
 * The `trial` array a call writes is bit for bit what hm_de_generation writes from the same population, status block, seed and
 * settings: the mutation stage does not look at a row. workspace: hm_de_workspace_bytes(n_pixels, n_frames, pop_size) bytes.
 * Statuses, an earlier one winning, all before any launch: hm_de_generation's in its order (but for its limit rule); HM_EINVAL for
 * bit_depth outside 9..16 or variant outside 0..2; HM_EINVAL for a limit outside 0 .. R - 1; HM_EUNSUPPORTED for variant 1 where the row
 * does not fit LDS (15 and 16 bits); HM_EALIGN for a dn that is not 2-byte aligned; (device build) HM_EINVAL for a NULL workspace.
 * One problem per call; hm_de_generation_u16_batch below advances several such problems per call. */
int hm_de_generation_u16(double* population, double* energies, double* trial, double* trial_energies,
                         double* icrf /*(S, 2^bit_depth)*/, uint8_t* valid, int64_t* status,
                         const double* mean_icrf /*(2^b)*/, const double* pca /*(2^b, P) row-major*/,
                         const double* lower_limits, const double* upper_limits,
                         const uint16_t* dn, const double* std /*nullable*/, const double* exposures /*[host]*/,
                         int64_t n_pixels, int n_frames, int lower, int upper, int pop_size, int n_params,
                         int64_t seed, int64_t max_generations, double mutation_lo, double mutation_hi,
                         double recombination, double tol, double energy_limit,
                         int bit_depth, int variant, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same generation for n_problems independent problems of identical shape - the channels of a calibration, or
 * restarts of one channel with other seeds - advanced by ONE call: one linear chain of launches on one stream, no
 * allocation, no host synchronisation, no float atomics (the contract of hm_de_generation).
 *
 * Specification: problem k of a batch evolves exactly as hm_de_generation would evolve it alone with the same inputs and
 * seed - BIT FOR BIT, in every state array and every status word, after every call. In particular
 *   - the random numbers of a problem depend on its own seed, the generation, the member and the draw index only
 *     (U(g, i, k) above with seed = seeds[k]); never on the problem's position in the batch or on n_problems;
 *   - the energy of a candidate is summed in the order hm_linearity_energy uses for pop_size candidates on n_pixels
 *     pixels (the launch geometry is chosen from the per-problem pop_size, not from n_problems * pop_size);
 *   - each problem has its own status block and stop flag. Once status[k][HM_DE_STOP] != 0 no kernel of a later call
 *     stores anything for problem k (its energy workgroups return at once: a converged problem costs no pixel work
 *     while the others run); the other problems go on. The caller stops issuing calls when every flag is set.
 *
 * Shared by all problems: pop_size S, n_params P, n_pixels, n_frames, exposures [host], lower, upper, lower_limits (P),
 * upper_limits (P) on the device, max_generations, mutation range, recombination, tol, energy_limit.
 * Per problem, as HOST arrays of n_problems entries read at call time (they travel in the kernel arguments, so a
 * recorded graph holds them by value):
 *   dn     device pointers to the uint8 (n_pixels, n_frames) stacks; problems may name the same stack
 *   std    NULL (no problem has a std stack), or device pointers to float64 stacks for ALL problems
 *   seeds  the problems' seeds
 * Per-problem state, caller-owned device memory (host memory in the host build), contiguous with the problem outermost:
 *   population (K, S, P), energies (K, S), trial (K, S, P), trial_energies (K, S), icrf (K, S, 256) float64;
 *   valid (K, S) uint8; status (K, HM_DE_STATUS_WORDS) zeroed before generation 0; mean_icrf (K, 256), pca (K, 256, P)
 *   workspace  hm_de_batch_workspace_bytes(n_pixels, n_frames, pop_size, n_problems) bytes (0 for arguments the call
 *              would reject)
 * Returns, before any launch and before any pointer is read: HM_EINVAL for n_problems < 1 or a NULL required pointer
 * (array or entry), HM_ESHAPE for n_problems > HM_DE_MAX_PROBLEMS, HM_EUNSUPPORTED for n_problems * pop_size > 65535
 * (the candidate limit of the energy grid); every other argument as hm_de_generation.
 * ------------------------------------------------------------------------------------------ */
#define HM_DE_MAX_PROBLEMS 64
size_t hm_de_batch_workspace_bytes(int64_t n_pixels, int n_frames, int pop_size, int n_problems);
int hm_de_generation_batch(int n_problems, double* population, double* energies, double* trial, double* trial_energies,
                           double* icrf, uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca,
                           const double* lower_limits, const double* upper_limits, const uint8_t* const* dn /*[host]*/,
                           const double* const* std /*[host], nullable*/, const int64_t* seeds /*[host]*/,
                           const double* exposures /*[host]*/, int64_t n_pixels, int n_frames, int lower, int upper,
                           int pop_size, int n_params, int64_t max_generations, double mutation_lo, double mutation_hi,
                           double recombination, double tol, double energy_limit, void* workspace, void* stream);

/* ... for n_problems problems on uint16 DN stacks of ONE shape and ONE bit depth (9..16): hm_de_generation_batch's text with rows of
 * R = 2^bit_depth entries in place of 256. Specification: problem k evolves exactly as hm_de_generation_u16 would evolve it alone with
 * the same inputs, seeds[k], bit_depth and variant - BIT FOR BIT, in every state array and every status word, after every call.
 *   state      contiguous with the problem outermost: population (K, S, P), energies (K, S), trial (K, S, P), trial_energies (K, S),
 *              icrf (K, S, R), valid (K, S), status (K, HM_DE_STATUS_WORDS) zeroed before generation 0; mean_icrf (K, R), pca (K, R, P)
 *   dn, std, seeds   HOST arrays of n_problems entries that travel in the kernel arguments (a recorded graph holds them by value): device
 *              pointers to the uint16 (n_pixels, n_frames) stacks, 2-byte aligned (problems may name the same stack); std NULL or
 *              given for ALL problems; random numbers depend on (seeds[k], generation, member, draw) only
 *   stop       each problem has its own stop flag. Once it is set no kernel of a later call stores anything for that problem - the row
 *              walk, the verdict kernel, the energy kernels (its workgroups return before the row fill) and the selection included
 *   energy     the launch geometry (pixel- or pair-major, the chunk count) and, with variant 0, the row's placement are chosen as
 *              hm_linearity_energy_u16 chooses them for pop_size candidates on n_pixels pixels - per problem, never from K x S
 *   workspace  hm_de_batch_workspace_bytes(n_pixels, n_frames, pop_size, n_problems) bytes: the 8-bit batch's function (K times
 *              hm_de_workspace_bytes, which does not depend on the depth; 0 for arguments the call would reject)
 * One linear chain of launches on one stream; no allocation, no host synchronisation, no atomics of any kind.
 * Statuses, an earlier one winning, all before any launch and before any device pointer is read: hm_de_generation_batch's in its order
 * (but for its 8-bit limit rule) - HM_EINVAL for n_problems < 1, HM_ESHAPE for n_problems > HM_DE_MAX_PROBLEMS, the counts and shapes,
 * HM_EUNSUPPORTED for n_problems * pop_size > 65535, the ranges, HM_EINVAL for a NULL array or a NULL entry of dn / std; then
 * hm_de_generation_u16's additions - HM_EINVAL for bit_depth outside 9..16, variant outside 0..2 or a limit outside 0 .. R - 1,
 * HM_EUNSUPPORTED for variant 1 where the row does not fit LDS; HM_EALIGN for a dn[k] that is not 2-byte aligned; (device build)
 * HM_EINVAL for a NULL workspace. */
int hm_de_generation_u16_batch(int n_problems, double* population, double* energies, double* trial, double* trial_energies,
                               double* icrf /*(K, S, 2^bit_depth)*/, uint8_t* valid, int64_t* status,
                               const double* mean_icrf /*(K, 2^b)*/, const double* pca /*(K, 2^b, P)*/,
                               const double* lower_limits, const double* upper_limits, const uint16_t* const* dn /*[host]*/,
                               const double* const* std /*[host], nullable*/, const int64_t* seeds /*[host]*/,
                               const double* exposures /*[host]*/, int64_t n_pixels, int n_frames, int lower, int upper,
                               int pop_size, int n_params, int64_t max_generations, double mutation_lo, double mutation_hi,
                               double recombination, double tol, double energy_limit, int bit_depth, int variant,
                               void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * On-disk formats: host-side strip decoders for the TIFF files the reference exchanges with
 * OpenCV (modules/image_set.py:214-243 cv.imread, :264-363 cv.imwrite). HOST pointers, no device work, re-entrant.
 * Return the number of bytes written to dst, HM_EINVAL for a corrupt stream, HM_ESHAPE if dst_cap is too small.
 *   hm_tiff_lzw_decode       TIFF 6.0 LZW (Compression 5), MSB-first 9..12-bit codes, libtiff's early change
 *   hm_tiff_packbits_decode  PackBits (Compression 32773)
 * ------------------------------------------------------------------------------------------ */
int64_t hm_tiff_lzw_decode(const uint8_t* src, int64_t src_len, uint8_t* dst, int64_t dst_cap);
int64_t hm_tiff_packbits_decode(const uint8_t* src, int64_t src_len, uint8_t* dst, int64_t dst_cap);

/* ------------------------------------------------------------------------------------------
 * The same strips decoded ON THE DEVICE (csrc/hm_tiff_device.hip; the host build carries the same entry point with host pointers and
 * a serial loop, so that it exports the whole ABI - tiff_io.imread does not use it): the file's bytes go
 * up as they are, and one call turns them into the frame cv.imread returns - LZW decode (one strip per wave, string table in LDS),
 * Predictor 2 undone, R and B swapped at sample granularity, cv.imread's flag applied. Opt-in (tiff_io.imread_device); the host
 * decoders above stay the default path.
 *   file, file_len      the whole file in device memory
 *   strip_offsets / strip_counts   (n_strips) int64 in device memory: StripOffsets / StripByteCounts. n_strips must be
 *                       ceil(height / min(rows_per_strip, height)). Strip s holds min(rows_per_strip, height - s * rows_per_strip) rows of
 *                       width * samples * bytes_per_sample bytes: its expected size. Strips, chunky layout, little-endian samples.
 *   compression         1 (none: strips are read straight from `file`) or 5 (LZW, the stream rules of hm_tiff_lzw_decode)
 *   predictor           1, or 2 (horizontal differencing) with 1-byte samples
 *   samples             1, 3 or 4 per pixel; bytes_per_sample 1 (uint8) or 8 (float64)
 *   color_mode          0 = cv.IMREAD_UNCHANGED: dst is (height, width, samples) in B,G,R(,A) order (samples == 1: (height, width));
 *                       1 = cv.IMREAD_COLOR, 1-byte samples only: dst is (height, width, 3) B,G,R - grey replicated, alpha dropped
 *   strip_status        (n_strips) int64 in device memory, written by the call: the number of bytes strip s produced (compression 1:
 *                       min(count, expected size)), or the negative code hm_tiff_lzw_decode returns for that stream - HM_EINVAL for a
 *                       corrupt one, HM_ESHAPE for one that runs past the expected size - and HM_EINVAL for a strip whose
 *                       [offset, offset + count) does not lie inside [0, file_len): nothing of such a strip is read. A strip with a
 *                       negative status leaves its rows of dst untouched and does not disturb the others; one that produced fewer
 *                       bytes than expected fills the whole pixels it holds.
 *   workspace           hm_tiff_decode_workspace_bytes(n_strips, strip_bytes, compression) bytes of device memory, with strip_bytes =
 *                       min(rows_per_strip, height) * width * samples * bytes_per_sample; 0 (NULL is fine) for compression 1
 * Returns, before any HIP call: HM_EINVAL for a NULL file / strip_offsets / strip_counts / dst / strip_status (or workspace with
 * compression 5), file_len < 0, n_strips / rows_per_strip / height / width < 1, a predictor other than 1 or 2 and a color_mode other
 * than 0 or 1; HM_EUNSUPPORTED for a compression other than 1 or 5, samples other than 1, 3 or 4, bytes_per_sample other than 1 or 8,
 * and 8-byte samples with predictor 2 or color_mode 1; HM_ESHAPE for an n_strips that does not match the geometry and for strips of
 * more than 2^31 bytes. The return value speaks of the call; the strips speak through strip_status, valid once `stream` has run.
 * ------------------------------------------------------------------------------------------ */
size_t hm_tiff_decode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression);
int hm_tiff_decode_strips(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts, int n_strips,
                          int compression, int predictor, int rows_per_strip, int height, int width, int samples, int bytes_per_sample,
                          int color_mode, void* dst, int64_t* strip_status, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same call for the wider sample types, in either byte order (csrc/hm_tiff_device.hip; the host build carries it with host
 * pointers, and both run one text for the row, csrc/hm_tiff_wide_body.h): uint16 frames of 9- to 16-bit cameras, the float32
 * " STD.tif" companions ImageSet.save_32bit writes, and big-endian float64. Opt-in (tiff_io.imread_device(wide_samples=True)).
 * Everything not named here is as in hm_tiff_decode_strips: the strips and their range check against file_len, the LZW decode,
 * strip_status, the workspace (hm_tiff_decode_workspace_bytes with this call's bytes_per_sample in strip_bytes), failed strips that
 * leave their rows alone. A short strip fills the whole pixels it holds: a stream that ends inside a sample or a pixel does not write
 * that pixel.
 *   bytes_per_sample    2 (uint16), 4 (float32) or 8 (float64); 4- and 8-byte samples are moved as bit patterns
 *   big_endian          0 or 1; 1: every sample is byte-reversed as it is read (an MM file), so dst is in native order either way
 *   predictor           1, or 2 with 2-byte samples: the differences are undone on sample values modulo 65536 - for a big-endian file
 *                       after the reversal, like tiff_io.imread
 *   samples             1, 3 or 4 per pixel
 *   color_mode          0 = cv.IMREAD_UNCHANGED: dst is (height, width, samples) of the sample type in B,G,R(,A) order (samples == 1:
 *                       (height, width)); 1 = cv.IMREAD_COLOR, 2-byte samples only: dst is (height, width, 3) uint8 B,G,R with
 *                       each sample >> 8 - grey replicated, alpha dropped (cv.imread's conversion)
 *   dst                 aligned to bytes_per_sample in color_mode 0. Strips may sit at any file offset, odd ones included: rows that
 *                       start on a sample boundary are loaded sample-wide, the others byte by byte
 * Returns, before any HIP call: HM_EINVAL for a NULL file / strip_offsets / strip_counts / dst / strip_status (or workspace with
 * compression 5), file_len < 0, n_strips / rows_per_strip / height / width < 1, a predictor other than 1 or 2, a color_mode or a
 * big_endian other than 0 or 1; HM_EUNSUPPORTED for a compression other than 1 or 5, samples other than 1, 3 or 4, bytes_per_sample
 * other than 2, 4 or 8 (1 is hm_tiff_decode_strips), and 4- or 8-byte samples with predictor 2 or color_mode 1; HM_ESHAPE for an
 * n_strips that does not match the geometry and for strips of more than 2^31 bytes; HM_EALIGN for a misaligned dst. An earlier code
 * wins over a later one.
 * ------------------------------------------------------------------------------------------ */
int hm_tiff_decode_strips_wide(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts,
                               int n_strips, int compression, int predictor, int rows_per_strip, int height, int width, int samples,
                               int bytes_per_sample, int big_endian, int color_mode, void* dst, int64_t* strip_status,
                               void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The writing twin (csrc/hm_tiff_encode.hip; the host build carries the same entry points with host pointers, one strip per OpenMP
 * iteration, and tiff_io.imwrite writes its LZW files through that): one call turns an image in device memory into the strips of a
 * TIFF file - float64 optionally quantised to uint8 with save_8bit's arithmetic, B,G,R(,A) turned into file order R,G,B(,A),
 * Predictor 2 applied, every strip LZW-encoded by one wave with its dictionary in LDS, and the strips compacted into one payload that
 * is copied down once. Opt-in (tiff_io.imwrite_device); tiff_io.imwrite stays the default path.
 *   src                 (height, width, samples) in B,G,R(,A) order, dense, in device memory
 *   src_kind            0 = uint8, stored as it is; 1 = float64, stored as it is (little-endian 8-byte words); 2 = float64 stored as
 *                       uint8: q = rint((v / divisor) * 255.0) in exactly that order, round half to even, wrapped modulo 256 (the
 *                       convention of hm_linearize_f64's index); non-finite samples give 0. A divisor of 1.0 is "no scaling"
 *   divisor             read with src_kind 2 only
 *   rows_per_strip      strip s holds min(rows_per_strip, height - s * rows_per_strip) rows of width * samples * (1 or 8) bytes;
 *                       n_strips = ceil(height / min(rows_per_strip, height)), strip_bytes = min(rows_per_strip, height) * row bytes
 *   compression         1 (none) or 5 (LZW: the stream rules of hm_tiff_lzw_decode, a Clear first and when the table is full, EOI last)
 *   predictor           1, or 2 (horizontal differencing modulo 256 within a row) with 1-byte output
 *   payload             payload_cap >= hm_tiff_encode_payload_bytes(n_strips, strip_bytes, compression) bytes, 16-byte aligned.
 *                       Compression 1: strip s at s * strip_bytes, no gaps. Compression 5: strip s at strip_offsets[s], a multiple of
 *                       16; the bytes between the end of a stream and the next strip are zeros. Every byte of
 *                       payload[0, strip_offsets[n_strips]) is written by the call
 *   strip_offsets       (n_strips + 1) int64, written by the call: offsets into payload; the last entry is the payload's size
 *   strip_counts        (n_strips) int64, written by the call: StripByteCounts. Each is at most hm_tiff_encode_bound(strip_bytes) =
 *                       (3 n + 1) / 2 + n / 2048 + 8, which no LZW stream of n bytes passes (derivation: csrc/hm_tiff_lzw_enc_body.h);
 *                       every code is checked against it before it is emitted, and a strip that would pass it gets HM_ESHAPE here
 *   workspace           hm_tiff_encode_workspace_bytes(n_strips, strip_bytes, compression) bytes, 16-byte aligned; 0 (NULL is fine)
 *                       for compression 1
 * Returns, before any HIP call: HM_EINVAL for a NULL src / payload / strip_offsets / strip_counts (or workspace with compression 5),
 * height / width / rows_per_strip < 1, a predictor other than 1 or 2 and, with src_kind 2, a divisor that is not finite and positive;
 * HM_EUNSUPPORTED for a compression other than 1 or 5, samples other than 1, 3 or 4, an unknown src_kind and predictor 2 with 8-byte
 * output; HM_ESHAPE for strips of 2^31 bytes or more and a payload_cap below hm_tiff_encode_payload_bytes; HM_EALIGN for a payload or
 * workspace that is not 16-byte aligned and tables or float64 sources that are not 8-byte aligned. The two size helpers return 0, and
 * hm_tiff_encode_bound a negative code, for sizes below 1 and strips of 2^31 bytes or more.
 * ------------------------------------------------------------------------------------------ */
int64_t hm_tiff_encode_bound(int64_t strip_bytes);
size_t hm_tiff_encode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression);
size_t hm_tiff_encode_payload_bytes(int n_strips, int64_t strip_bytes, int compression);
int hm_tiff_encode_strips(const void* src, int src_kind, double divisor, int height, int width, int samples, int rows_per_strip,
                          int compression, int predictor, void* payload, int64_t payload_cap, void* strip_offsets /* n_strips + 1 int64 */,
                          void* strip_counts /* n_strips int64 */, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same call for the wider stored samples (csrc/hm_tiff_encode.hip; the host build carries it with host pointers, and both run one
 * text for the row, csrc/hm_tiff_wide_enc_body.h): the uint16 DN frames of 9- to 16-bit cameras, the float32 images ImageSet.save_32bit
 * writes, and float64 images stored as float32 or quantised to uint16 (ImageSet.save_16bit). The writing twin of
 * hm_tiff_decode_strips_wide; opt-in (tiff_io.imwrite_device(wide_samples=True), tiff_io.imwrite(wide_samples=True) through the host
 * build). Everything not named here is as in hm_tiff_encode_strips: little-endian samples in R,G,B(,A) order with the R/B swap at sample
 * granularity, the strips, the LZW stage, payload, strip_offsets, strip_counts, the 16-byte rounding with zeroed gaps and the workspace
 * (hm_tiff_encode_bound / _workspace_bytes / _payload_bytes with this call's strip bytes).
 *   src_kind            HM_TIFF_SRC_U16        (0) uint16, stored as it is
 *                       HM_TIFF_SRC_F32        (1) float32, stored bit for bit
 *                       HM_TIFF_SRC_F64_AS_F32 (2) float64 stored as float32: IEEE round-to-nearest-even narrowing, what
 *                                                  ndarray.astype(np.float32) gives - subnormal results kept, overflow to +-inf, a NaN
 *                                                  stays a NaN (its payload bits are not pinned)
 *                       HM_TIFF_SRC_F64_AS_U16 (3) float64 stored as uint16: q = rint((v / divisor) * max_dn) in exactly that order,
 *                                                  round half to even, wrapped modulo 65536; non-finite samples and |q| >= 2^63 give 0
 *   divisor, max_dn     read with src_kind 3 only: divisor finite and positive, max_dn in 1 .. 65535 (2^bit_depth - 1)
 *   predictor           1, or 2 with uint16 output (kinds 0 and 3): the difference, modulo 65536, of the STORED values (for kind 3 the
 *                       quantised ones) to the same channel of the pixel on the left; the first pixel of every row is stored as it is
 *   src                 aligned to its own sample size: 2 (kind 0), 4 (kind 1) or 8 (kinds 2 and 3)
 * Returns, before any HIP call and in this order (an earlier code wins over a later one): HM_EINVAL for a NULL src / payload /
 * strip_offsets / strip_counts, height / width / rows_per_strip < 1 and a predictor other than 1 or 2; HM_EINVAL for, with src_kind 3, a
 * divisor that is not finite and positive or a max_dn outside 1 .. 65535, and for a NULL workspace with compression 5; HM_EUNSUPPORTED
 * for a compression other than 1 or 5, samples other than 1, 3 or 4, a src_kind outside 0 .. 3 and predictor 2 with float32 output;
 * HM_ESHAPE for strips of 2^31 bytes or more and a payload_cap below hm_tiff_encode_payload_bytes; HM_EALIGN for a payload or workspace
 * that is not 16-byte aligned, tables that are not 8-byte aligned and a src that is not aligned to its sample size.
 * ------------------------------------------------------------------------------------------ */
#define HM_TIFF_SRC_U16 0
#define HM_TIFF_SRC_F32 1
#define HM_TIFF_SRC_F64_AS_F32 2
#define HM_TIFF_SRC_F64_AS_U16 3
int hm_tiff_encode_strips_wide(const void* src, int src_kind, double divisor, int max_dn, int height, int width, int samples,
                               int rows_per_strip, int compression, int predictor, void* payload, int64_t payload_cap,
                               void* strip_offsets /* n_strips + 1 int64 */, void* strip_counts /* n_strips int64 */, void* workspace,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDRMERGE_H */
