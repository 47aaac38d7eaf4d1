"""ExposureSeries / ExposurePair - mirror of modules/exposure_series.py:18-495 on the HIP backend.

The reference's merge is two Python loops over the frames (exposure_series.py:334-341 and :372-392),
each iteration a couple of dozen whole-image NumPy temporaries plus disk reads. Here
`process_HDR_image` hands the whole stack to ONE fused HIP launch (engine.plan_merge -> hm_merge):
sum of weights, linearization, weighted radiance, variance propagation, hot-pixel filtering and the
flat-field step happen per pixel in registers, every input byte is read once.

Deviations: C/D - accumulators are plain zero-initialised arrays and S, S**2 are arrays;
E - the caller passes ICRF (and optionally ICRF_diff, else it is derived with the reference's
gradient convention); G - the corrections are applied; J - frames are taken from memory (they are
loaded from `path` only when an ImageSet holds no pixels yet).
"""
from __future__ import annotations

import math

from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native as nat
from . import settings as gs
from .image_set import ImageSet, _std_path, read_STD_file


def icrf_derivative(ICRF, bits: int = None):
    """ICRF_diff[:, c] = np.gradient(ICRF[:, c], 2 / (BITS - 1)) - the convention of
    modules/general_functions.py:268-272 and tests/unit/test_measurand.py:21 (host, 256 x C numbers)."""
    bits = gs.BITS if bits is None else bits
    icrf = ICRF.cpu().numpy() if isinstance(ICRF, torch.Tensor) else np.asarray(ICRF, dtype=np.float64)
    dx = 2 / (bits - 1)
    if icrf.ndim == 1:
        return np.gradient(icrf, dx)
    out = np.zeros_like(icrf)
    for c in range(icrf.shape[1]):
        out[:, c] = np.gradient(icrf[:, c], dx)
    return out


def _roi_means(flat_set, eng, t: torch.Tensor, bounds, which: str) -> np.ndarray:
    """Per-channel ROI means of a flat field (modules/measurand.py:570-583) as host numbers - remembered on the flat's ImageSet: one flat
    serves many exposure series, and each evaluation is a small reduction kernel plus a device-to-host copy that the merge would wait
    for. The key holds the tensor's identity and version (an in-place edit or a new image computes again)."""
    cache = flat_set.__dict__.setdefault("_roi_mean_cache", {})       # which ("val" / "std") -> (key, means): one image and one ROI each
    key = (t.data_ptr(), t._version, tuple(t.shape), str(t.device), tuple(bounds))
    if cache.get(which, (None, None))[0] != key:
        cache[which] = (key, eng.roi_mean(t, *bounds).cpu().numpy())
    return cache[which][1]


def read_ICRF_file(file_path, return_derivative: bool = True):
    """modules/general_functions.py:254-277 with the intended return value (the derivative, not the ICRF twice)."""
    icrf = np.loadtxt(file_path, dtype=float)
    return (icrf, icrf_derivative(icrf)) if return_derivative else (icrf, None)


class ExposurePair(object):
    """modules/exposure_series.py:18-76."""

    def __init__(self, short_exposure: ImageSet, long_exposure: ImageSet):
        self.short_exposure = short_exposure
        self.long_exposure = long_exposure
        self.exposure_ratio = short_exposure.features["exposure"] / long_exposure.features["exposure"]
        self.absolute_difference = None
        self.relative_difference = None
        self.absolute_stats = None
        self.relative_stats = None

    def compute_difference(self):
        self.absolute_difference, self.relative_difference = ImageSet.compute_difference(self.short_exposure, self.long_exposure)

    def compute_stats(self, axis=None, release_memory_after: Optional[bool] = True):
        self.absolute_stats = self.absolute_difference.measurand.compute_dimension_statistics(axis=axis)
        self.relative_stats = self.relative_difference.measurand.compute_dimension_statistics(axis=axis)
        if release_memory_after:
            self.absolute_difference = None
            self.relative_difference = None

    def compute_difference_stats(self):
        """compute_difference() + compute_stats(axis=(0, 1), release_memory_after=True) in one fused HIP reduction
        (hm_pair_statistics): the two difference images are never written to HBM."""
        xs, ys = self.short_exposure.measurand, self.long_exposure.measurand
        ab, rel = xs._eng().pair_statistics(xs._f64(), xs._std, ys._f64(), ys._std, self.exposure_ratio)
        self.absolute_stats = {k: xs._export(v) for k, v in ab.items()}
        self.relative_stats = {k: xs._export(v) for k, v in rel.items()}
        self.absolute_difference = None
        self.relative_difference = None

    def process_linearity_distribution(self, bins: int, included_range=None, channels=None, use_std: Optional[bool] = False):
        return (self.absolute_difference.measurand.compute_channel_histogram(bins, included_range, channels, use_std),
                self.relative_difference.measurand.compute_channel_histogram(bins, included_range, channels, use_std))


class ExposureSeries(object):
    """modules/exposure_series.py:79-476."""

    def __init__(self, merged_image_set: Optional[ImageSet] = None, directory_path: Optional[Path] = None,
                 input_image_sets: Optional[List[ImageSet]] = None, use_cupy: Optional[bool] = True):
        self.merged_image_set = merged_image_set
        self.input_image_sets = input_image_sets if input_image_sets is not None else []
        if isinstance(directory_path, Path) and directory_path.suffix != "":
            self.directory_path = directory_path.parent
        else:
            self.directory_path = directory_path
        self.exposure_pairs = None
        self._use_cupy = use_cupy if not input_image_sets else input_image_sets[0].use_cupy

    @property
    def use_cupy(self):
        return self._use_cupy

    @use_cupy.setter
    def use_cupy(self, new_value):
        raise AttributeError("use_cupy is a read-only attribute, managing the state of the used array backend.")

    # ---- constructors (exposure_series.py:117-203)
    @classmethod
    def from_image_set(cls, reference_image_set: ImageSet, directory_path: Optional[Path] = None):
        search_path = reference_image_set.path.parent if directory_path is None else directory_path
        found = [s for s in ImageSet.multiple_from_path(search_path, use_cupy=reference_image_set.use_cupy) if reference_image_set.is_exposure_match(s)]
        found.sort(key=lambda s: s.features["exposure"])
        return cls(directory_path=search_path, input_image_sets=found)

    @classmethod
    def from_dir_path(cls, directory_path: Path, use_cupy: Optional[bool] = False):
        """exposure_series.py:148-160; `use_cupy` (an addition) picks the backend of the ImageSets it creates - the reference's
        ImageSet default, the host backend, unless asked for the device."""
        return cls.from_multiple_image_sets(ImageSet.multiple_from_path(directory_path, use_cupy=use_cupy))

    @classmethod
    def from_multiple_image_sets(cls, list_of_image_sets: List[ImageSet]):
        sublists: List[List[ImageSet]] = []
        for image_set in list_of_image_sets:
            for sub in sublists:
                if sub[0].is_exposure_match(image_set):
                    sub.append(image_set)
                    break
            else:
                sublists.append([image_set])
        out = []
        for sub in sublists:
            sub.sort(key=lambda s: s.features["exposure"])
            out.append(cls(input_image_sets=sub))
        return out

    def load_value_images(self, bit_64: Optional[bool] = False, device_decode: Optional[bool] = False):
        """`device_decode=True` (an addition): the TIFFs are decoded on the GPU, ImageSet.load_value_image - 16-bit and big-endian
        files and, in load_std_images, float32 ' STD.tif' files included (tiff_io.imread_device(wide_samples=True))."""
        for image_set in self.input_image_sets:
            image_set.load_value_image(bit64=bit_64, device_decode=device_decode)

    def load_std_images(self, bit_64: Optional[bool] = False, device_decode: Optional[bool] = False):
        for image_set in self.input_image_sets:
            image_set.load_std_image(bit64=bit_64, device_decode=device_decode)

    def linearize(self, ICRF, ICRF_diff=None, release_memory: Optional[bool] = False):
        """exposure_series.py:226-250."""
        new_sets = []
        for s in self.input_image_sets or []:
            new_sets.append(s.linearize(ICRF, ICRF_diff))
            if release_memory:
                s.measurand.val = None
                s.measurand.std = None
        return ExposureSeries(merged_image_set=self.merged_image_set, directory_path=self.directory_path, input_image_sets=new_sets)

    def extract(self, channels=None, release_memory: Optional[bool] = False):
        new_merged = self.merged_image_set.extract(channels) if self.merged_image_set is not None else None
        new_sets = []
        for s in self.input_image_sets or []:
            new_sets.append(s.extract(channels))
            if release_memory:
                s.measurand.val = None
                s.measurand.std = None
        return ExposureSeries(merged_image_set=new_merged, directory_path=self.directory_path, input_image_sets=new_sets)

    def initialize_exposure_pairs(self):
        """exposure_series.py:283-304."""
        pairs = []
        for i, x in enumerate(self.input_image_sets):
            for j, y in enumerate(self.input_image_sets):
                if i >= j or x.features["exposure"] / y.features["exposure"] < 0.1:
                    continue
                pairs.append(ExposurePair(x, y))
        self.exposure_pairs = pairs

    # ---- the merge (exposure_series.py:317-419)
    def _eng(self):
        """The engine of this series' backend (the first image's: HIP library, or the host build inside nat.host_mode())."""
        return self.input_image_sets[0].measurand._eng()

    def _stack_inputs(self, list_of_dark_fields, dark_threshold, with_std):
        """Collect the tensors for the fused launch: frames (all uint8 DNs or all float64 values), stds, per-frame dark DN maps + DN
        thresholds - in HBM on the HIP backend, host tensors on the host backend. A dark frame held by the other backend is moved over."""
        from . import engine
        sets = self.input_image_sets
        for s in sets:
            if s.measurand.shape is None:
                s.load_value_image()
        all_dn = all(s.measurand._dn_t() is not None for s in sets)
        frames = [s.measurand._dn_t() if all_dn else s.measurand._f64() for s in sets]
        dev = frames[0].device
        stds = None
        if with_std:
            for s in sets:
                if s.measurand._std is None:
                    s.load_std_image()
                if s.measurand._std is None:
                    raise ValueError("uncertainty propagation needs a std image for every frame")
            stds = [s.measurand._std for s in sets]
        thr = gs.DARK_THRESHOLD if dark_threshold is None else dark_threshold
        darks, mins = None, None
        if list_of_dark_fields:
            darks, mins = [], []
            for s in sets:
                dark, scale = s.select_dark_field(list_of_dark_fields)    # exposure gate: gs.DARK_THRESHOLD (image_set.py:173); `thr` is the PIXEL threshold (:387)
                if dark is None:
                    darks.append(None)
                    mins.append(gs.BITS)
                    continue
                if dark.measurand.shape is None:
                    dark.load_value_image()
                if dark.measurand._dn_t() is not None:
                    darks.append(dark.measurand._dn_t().to(dev))
                    mins.append(engine.dark_min_dn(scale, thr))
                else:                                   # float-valued dark: 0/1 map, hot iff value*scale > thr
                    darks.append(((dark.measurand._tv() * scale) > thr).to(torch.uint8).to(dev))
                    mins.append(1)
        return frames, stds, darks, mins

    def _precalculate_sum_of_weights(self, list_of_dark_fields: Optional[List[ImageSet]] = None,
                                     dark_threshold: Optional[float] = None):
        """exposure_series.py:317-345 -> (S, S**2) device arrays."""
        frames, _, darks, mins = self._stack_inputs(list_of_dark_fields, dark_threshold, with_std=False)
        exp = self.input_image_sets[0].measurand._export
        S, S2 = self._eng().sum_of_weights(frames, darks=darks, dark_min=mins, median_k=gs.MEDIAN_FILTER_KERNEL_SIZE)
        return exp(S), exp(S2)

    def _compute_HDR_image_set(self, list_of_dark_fields, sum_of_weights, square_sum_of_weights, ICRF, ICRF_diff,
                               flat_set: Optional[ImageSet] = None, dark_threshold: Optional[float] = None,
                               use_std: Optional[bool] = None, out_dtype=None, STD_data=None):
        """exposure_series.py:347-397. The fused kernel recomputes the sum of weights in registers, so the
        two precalculated arrays are accepted for signature compatibility and not read.
        out_dtype: None / torch.float64, or torch.float32 - the merged measurand then holds float32 arrays (engine.plan_merge).
        STD_data: the (BITS, C) per-DN STD table of ImageSet.calculate_numerical_STD (None: settings.STD_FILE_NAME, when set). The
        reference's rule per frame (image_set.py:228-243): '<name> STD.tif', else the table. When NO frame has a std - in memory or on
        disk - the table goes into the fused kernel as it is (engine.plan_merge(std_table=...)) and no std image is materialised; when
        some frames have one, the others' are made from the table and the merge reads std frames. Without a table nothing changes."""
        from . import engine
        eng = self._eng()
        sets = self.input_image_sets
        std_table = None
        if use_std is None or use_std:
            if STD_data is None:
                STD_data = read_STD_file()
            if STD_data is not None:
                for s in sets:
                    if s.measurand.shape is None:
                        s.load_value_image()
                have = [s.measurand._std is not None or (s.path is not None and _std_path(s.path).exists()) for s in sets]
                table = np.asarray(STD_data.cpu() if isinstance(STD_data, torch.Tensor) else STD_data, dtype=np.float64)
                n_ch = sets[0].measurand.shape[-1]
                fusable = table.shape == (gs.BITS, n_ch) and len(sets) <= nat.HM_MAX_FRAMES and len(sets[0].measurand.shape) == 3
                if not any(have) and fusable:
                    std_table, use_std = table, False       # (no std FRAMES: _stack_inputs collects values only)
                else:
                    for s in sets:
                        if s.measurand._std is None:
                            s.load_std_image(STD_data)      # the file, else the table: image_set.py:228-243
                    use_std = True
        if use_std is None:
            for s in sets:                                  # the reference loads every frame's std image (:377),
                if s.measurand._std is None and s.path is not None:     # whether or not its value image is in memory yet
                    s.load_std_image()
            have = [s.measurand._std is not None for s in sets]
            if any(have) and not all(have):
                raise ValueError("some frames have a std image and some do not: uncertainty propagation needs one for every frame "
                                 "(pass use_std=False to merge values only)")
            use_std = all(have)
        frames, stds, darks, mins = self._stack_inputs(list_of_dark_fields, dark_threshold, with_std=use_std)
        use_std = use_std or std_table is not None          # from here on: the merge produces a std image
        dev = frames[0].device
        if ICRF_diff is None and use_std:
            ICRF_diff = icrf_derivative(ICRF)
        kw = {}
        if flat_set is not None:                                   # exposure_series.py:415-417
            if flat_set.measurand.shape is None:
                flat_set.load_value_image()
            fm = flat_set.measurand
            fval = (fm._dn_t() if fm._dn_t() is not None else fm._f64()).to(dev)
            size_x = gs.IM_SIZE_X or fval.shape[0]
            size_y = gs.IM_SIZE_Y or fval.shape[1]
            x0, x1, y0, y1 = engine.flat_roi_bounds(size_x, size_y, gs.FF_MID_PERCENTAGE)
            kw.update(flat=fval, ff_mean=_roi_means(flat_set, eng, fval, (x0, x1, y0, y1), "val"))
            if use_std:
                if fm._std is None:
                    flat_set.load_std_image()
                if fm._std is None:
                    raise ValueError("flat field needs a std image to propagate uncertainty")
                fstd = fm._std.to(dev)
                kw.update(flat_std=fstd, ff_std_mean=_roi_means(flat_set, eng, fstd, (x0, x1, y0, y1), "std"))
        exposures = [s.features["exposure"] for s in sets]
        out = eng.merge(frames, exposures, ICRF, ICRF_diff if use_std else None, stds, darks=darks, dark_min=mins,
                        median_k=gs.MEDIAN_FILTER_KERNEL_SIZE, out_dtype=torch.float64 if out_dtype is None else out_dtype,
                        std_table=std_table, **kw)
        hdr = type(sets[0].measurand)(out["val"], out.get("std"))
        hdr_set = ImageSet(file_path=sets[0].get_file_path_without_exposure(), features=dict(sets[0].features) if sets[0].features else None,
                           measurand=hdr)
        hdr_set.is_HDR = True
        return hdr_set

    def process_HDR_image(self, ICRF=None, ICRF_diff=None, dark_list: Optional[List[ImageSet]] = None,
                          flat_list: Optional[List[ImageSet]] = None, use_std: Optional[bool] = None, out_dtype=None, STD_data=None):
        """exposure_series.py:399-419: merge the input images into self.merged_image_set.
        `out_dtype=torch.float32` (an addition; None = float64) stores the merged value / std images as float32: the same float64
        arithmetic, rounded once at the kernel's store - what ImageSet.save_32bit then writes.

        Defaults mirror the reference: `ICRF=None` reads settings.ICRF_CALIBRATED_FILE (:406-407; deviation E - the table is
        read as ONE (BITS, C) array and the derivative is formed with the reference's gradient convention), `dark_list=None`
        globs settings.DEFAULT_DARK_PATH (:409) and `flat_list=None` settings.DEFAULT_FLAT_PATH (image_set.py:146-155). A
        path that is not configured means "none": no dark frames / no flat field - but a missing ICRF raises.
        `STD_data` (None: the table of settings.STD_FILE_NAME, when set): the per-DN STD table behind frames without a std image; a series
        with no std image at all is merged with the table inside the fused kernel (_compute_HDR_image_set).
        A series whose images all hold float32 std images - set in memory, or loaded by load_std_image from the float32 '<name> STD.tif'
        files ImageSet.save_32bit writes - is merged from them as they are (engine.plan_merge: hm_merge_std_f32, no float64 copies), up to
        HM_MAX_FRAMES frames; the result is that of the widened stds, bit for bit."""
        if ICRF is None:
            if gs.ICRF_CALIBRATED_FILE is None:
                raise ValueError("process_HDR_image(ICRF=None) needs settings.ICRF_CALIBRATED_FILE (settings.configure(...)) "
                                 "or an explicit ICRF array")
            ICRF, default_diff = read_ICRF_file(gs.ICRF_CALIBRATED_FILE)
            if ICRF_diff is None:
                ICRF_diff = default_diff
        if not self.input_image_sets:
            raise ValueError("no input images")
        if dark_list is None and gs.DEFAULT_DARK_PATH is not None:
            dark_list = ImageSet.multiple_from_path(Path(gs.DEFAULT_DARK_PATH), use_cupy=self.use_cupy)
        if flat_list is None and gs.DEFAULT_FLAT_PATH is not None:
            flat_list = ImageSet.multiple_from_path(Path(gs.DEFAULT_FLAT_PATH), use_cupy=self.use_cupy)
        flat_set = self.input_image_sets[0].get_flat_field(flat_list) if flat_list else None
        self.merged_image_set = self._compute_HDR_image_set(dark_list, None, None, ICRF, ICRF_diff, flat_set=flat_set,
                                                            use_std=use_std, out_dtype=out_dtype, STD_data=STD_data)

    # ---- linearity statistics (exposure_series.py:421-476; "next" row f-1)
    def process_linearity(self, ICRF, linearity_limit: Optional[int] = None, use_std: Optional[bool] = False, *,
                          from_dn: bool = False, ICRF_diff=None, STD_data=None):
        """exposure_series.py:421-446 on a linearized series. from_dn=True (an addition) takes a series that still holds its 8-bit frames
        as DNs (from_dn measurands) and gives its pairs the statistics that self.linearize(ICRF, ICRF_diff) followed by
        process_linearity(ICRF, linearity_limit, use_std) would give them - with use_std the stds ICRF_diff * calculate_numerical_STD(
        STD_data) - in one hm_pairs_statistics_dn call: no float64 frame is written and the image sets stay DN frames. See
        _process_linearity_from_dn for what it asks of the series."""
        if from_dn:
            return self._process_linearity_from_dn(ICRF, linearity_limit, use_std, ICRF_diff, STD_data)
        lower, upper = map_linearity_limits(linearity_limit, linearity_limit, ICRF)
        for image_set in self.input_image_sets:
            if image_set.measurand.shape is None:
                image_set.load_value_image()
            if image_set.measurand._std is None and use_std:
                image_set.load_std_image()
        # the thresholds ride on the all-pairs launch where that applies (no separate pass over the frames); otherwise frame by frame
        if self._all_pairs_fused(lower, upper):
            return
        for image_set in self.input_image_sets:
            image_set.measurand.apply_thresholds(lower, upper)
        if self._all_pairs_fused():
            return
        for pair in self.exposure_pairs:
            v = pair.short_exposure.measurand._tv()
            if v is not None and v.dim() == 3 and v.shape[-1] <= 4 and pair.long_exposure.measurand.shape == tuple(v.shape):
                pair.compute_difference_stats()              # fused: no difference images in HBM
            else:
                pair.compute_difference()
                pair.compute_stats(axis=(0, 1), release_memory_after=True)

    def _own_pairs_stack(self):
        """(vals, stds or None, [(i, j, exposure ratio), ...]) when one all-pairs launch can serve this series: the pairs are pairs of the
        series' own images, all images share one (H, W, C <= 4) shape on one device and one backend and either all or none of them carry a
        std. None otherwise."""
        pairs = self._own_pairs()
        if pairs is None:
            return None
        sets = self.input_image_sets
        vals = [s.measurand._f64() for s in sets]
        if not all(v.device == vals[0].device for v in vals):
            return None
        stds = [s.measurand._std for s in sets] if sets[0].measurand._std is not None else None
        return vals, stds, pairs

    def _own_pairs(self):
        """[(i, j, exposure ratio), ...] under _own_pairs_stack's conditions on the pairs, shapes, stds and backends - no pixel is touched
        (the devices are the caller's to compare on the tensors it takes). None otherwise."""
        sets = self.input_image_sets
        if not self.exposure_pairs or not sets or len(sets) > nat.HM_MAX_FRAMES:      # (hm_pairs_statistics takes no more on either build)
            return None
        index = {id(s): i for i, s in enumerate(sets)}
        if any(id(p.short_exposure) not in index or id(p.long_exposure) not in index for p in self.exposure_pairs):
            return None
        shapes = {s.measurand.shape for s in sets}
        if len(shapes) != 1 or None in shapes or len(next(iter(shapes))) != 3 or next(iter(shapes))[-1] > 4:
            return None
        have_std = [s.measurand._std is not None for s in sets]
        if any(have_std) != all(have_std) or len({s.measurand.backend for s in sets}) != 1:
            return None
        return [(index[id(p.short_exposure)], index[id(p.long_exposure)], p.exposure_ratio) for p in self.exposure_pairs]

    def _process_linearity_from_dn(self, ICRF, linearity_limit, use_std, ICRF_diff, STD_data):
        """process_linearity(from_dn=True): _from_dn_inputs says what it asks of the series."""
        lower, upper = map_linearity_limits(linearity_limit, linearity_limit, ICRF)
        dns, pairs, icrf, diff, std_table = self._from_dn_inputs(ICRF, lower, upper, use_std, ICRF_diff, STD_data)
        exp = self.input_image_sets[0].measurand._export
        stats = self._eng().pairs_statistics_dn(dns, pairs, icrf, diff, std_table, thresholds=(lower, upper), to_host=True)
        for p, (ab, rel) in zip(self.exposure_pairs, stats):
            p.absolute_stats, p.relative_stats = {k: exp(v) for k, v in ab.items()}, {k: exp(v) for k, v in rel.items()}
            p.absolute_difference = p.relative_difference = None

    def _from_dn_inputs(self, ICRF, lower, upper, use_std, ICRF_diff, STD_data):
        """What from_dn=True asks of the series, for process_linearity and process_linearity_distribution alike: every image set holds a
        from_dn measurand (uint8 DNs) without a std frame, and the conditions of _own_pairs_stack hold (the pairs are pairs of the series'
        own images, one (H, W, C <= 4) shape, one device, one backend); ValueError otherwise. use_std needs ICRF_diff and a per-DN STD
        table (STD_data, or settings.STD_FILE_NAME). (BITS,) tables serve every channel, as they do in linearize and
        calculate_numerical_STD. lower / upper: one limit per channel. -> (DN frames, pairs, ICRF, ICRF_diff or None, STD table or None),
        the tables (BITS, C)."""
        sets = self.input_image_sets
        for image_set in sets:
            if image_set.measurand.shape is None:
                image_set.load_value_image()
        if not sets or any(s.measurand._dn is None for s in sets):
            raise ValueError("from_dn=True needs every image set to hold a from_dn measurand (8-bit DNs); linearize the series and call "
                             "process_linearity(ICRF, linearity_limit, use_std) instead")
        if any(s.measurand._std is not None for s in sets):
            raise ValueError("from_dn=True takes its stds from the per-DN STD table; a series whose images carry std frames goes the default "
                             "route: series.linearize(ICRF, ICRF_diff).process_linearity(ICRF, linearity_limit, use_std)")
        pairs = self._own_pairs()
        dns = [s.measurand._dn for s in sets]
        if pairs is None or not all(d.device == dns[0].device for d in dns):
            raise ValueError("from_dn=True needs the pairs to be pairs of the series' own images, all of one (H, W, C <= 4) shape on one "
                             "device and one backend")
        n_ch = dns[0].shape[-1]
        if len(lower) != n_ch or len(upper) != n_ch:
            raise ValueError("The length of 'lower' and 'upper' must match the size of the independent axis.")

        def table(t):                                          # (BITS, C), a (BITS,) column repeated for every channel
            t = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
            return np.repeat(t[:, None], n_ch, axis=1) if t.ndim == 1 else t
        diff = std_table = None
        if use_std:
            if STD_data is None:
                STD_data = read_STD_file()
            if ICRF_diff is None or STD_data is None:
                raise ValueError("use_std=True with from_dn=True needs ICRF_diff and STD_data (or settings.STD_FILE_NAME)")
            diff, std_table = table(ICRF_diff), table(STD_data)
        return dns, pairs, table(ICRF), diff, std_table

    def _all_pairs_fused(self, lower=None, upper=None) -> bool:
        """Every pair of the series in ONE launch (hm_pairs_statistics): each frame is read from HBM once instead of once per
        pair it takes part in. Applies when the pairs are pairs of this series' own images, all images share one (H, W, C <= 4)
        shape on one device and either all or none of them carry a std; otherwise the per-pair path above runs."""
        stack = self._own_pairs_stack()
        if stack is None:
            return False
        sets = self.input_image_sets
        vals, stds, pairs = stack
        thresholds = None
        if lower is not None or upper is not None:           # apply_thresholds (measurand.py:375-428) inside the launch, in place
            n_ch = vals[0].shape[-1]
            lower = [None] * n_ch if lower is None else lower
            upper = [None] * n_ch if upper is None else upper
            if len(lower) != n_ch or len(upper) != n_ch:
                raise ValueError("The length of 'lower' and 'upper' must match the size of the independent axis.")
            thresholds = ([-math.inf if l is None else l for l in lower], [math.inf if u is None else u for u in upper])
            vals = [v.contiguous() for v in vals]
            if stds is not None:
                stds = [sd.to(torch.float64).contiguous() for sd in stds]
            for s_, v in zip(sets, vals):                      # the image sets keep the tensors that are thresholded in place
                s_.measurand.val = v
            if stds is not None:
                for s_, sd in zip(sets, stds):
                    s_.measurand.std = sd
        exp = sets[0].measurand._export
        for p, (ab, rel) in zip(self.exposure_pairs, self._eng().pairs_statistics(vals, stds, pairs, to_host=True, thresholds=thresholds)):
            # (host tensors: 6C numbers per pair, fetched with ONE copy; NumPy arrays on the host backend)
            p.absolute_stats, p.relative_stats = {k: exp(v) for k, v in ab.items()}, {k: exp(v) for k, v in rel.items()}
            p.absolute_difference = p.relative_difference = None
        return True

    def process_linearity_distribution(self, bins: int, included_range=None, channels=None, use_std: Optional[bool] = False,
                                       lower: Optional[List] = None, upper: Optional[List] = None, from_dn: bool = False, ICRF=None,
                                       ICRF_diff=None, STD_data=None):
        """The distributions of every exposure pair: a list in self.exposure_pairs order of what pair.compute_difference() followed by
        pair.process_linearity_distribution(bins, included_range, channels, use_std) returns - (absolute, relative), each
        {channel: (hist, bin_edges)}. lower / upper: per-channel limits as apply_thresholds takes them, applied to the values as they are
        read: no image set is changed (process_linearity stays the call that thresholds in place).
        Under the conditions of _all_pairs_fused (and use_std only with a std on every image, bins <= HM_PAIRS_HIST_MAX_BINS) all pairs
        go through hm_pairs_histogram - no difference image is written, a frame is read once per launch; otherwise pair by pair through
        the difference images, each pair's dropped after its histograms.
        from_dn=True (an addition) takes a series that still holds its 8-bit frames as DNs (from_dn measurands; _from_dn_inputs says what
        it asks) and returns what the same call returns on a deep copy of the series that self.linearize(ICRF, ICRF_diff) made float64
        first - with use_std the stds ICRF_diff * calculate_numerical_STD(STD_data) - through hm_pairs_minmax_dn / hm_pairs_histogram_dn:
        no float64 frame is written and the image sets stay DN frames. Counts and edges are equal; weighted bins differ by the order of
        their sums only."""
        if channels is None:
            channels = list(range(gs.NUM_OF_CHS))
        if from_dn:
            if ICRF is None:
                raise ValueError("from_dn=True needs ICRF: the per-DN value table")
            sets = self.input_image_sets
            for image_set in sets:
                if image_set.measurand.shape is None:
                    image_set.load_value_image()
            n_ch = sets[0].measurand.shape[-1] if sets and sets[0].measurand.shape else 0
            lower = [None] * n_ch if lower is None else lower
            upper = [None] * n_ch if upper is None else upper
            lower, upper = [-math.inf if l is None else l for l in lower], [math.inf if u is None else u for u in upper]
            dns, pairs, icrf, diff, std_table = self._from_dn_inputs(ICRF, lower, upper, use_std, ICRF_diff, STD_data)
            return self._eng().pairs_histogram_dn(dns, pairs, icrf, diff, std_table, bins=bins, included_range=included_range, channels=channels,
                                                  thresholds=(lower, upper))
        for image_set in self.input_image_sets:
            if image_set.measurand.shape is None:
                image_set.load_value_image()
            if image_set.measurand._std is None and use_std:
                image_set.load_std_image()
        stack = self._own_pairs_stack() if int(bins) <= nat.HM_PAIRS_HIST_MAX_BINS else None
        if stack is not None and (not use_std or stack[1] is not None):
            vals, stds, pairs = stack
            n_ch = vals[0].shape[-1]
            thresholds = None
            if lower is not None or upper is not None:
                lower = [None] * n_ch if lower is None else lower
                upper = [None] * n_ch if upper is None else upper
                thresholds = ([-math.inf if l is None else l for l in lower], [math.inf if u is None else u for u in upper])
            return self._eng().pairs_histogram(vals, stds if use_std else None, pairs, bins, included_range, channels, thresholds=thresholds)
        import copy
        out = []
        for pair in self.exposure_pairs or []:
            if lower is None and upper is None:
                ab, rel = ImageSet.compute_difference(pair.short_exposure, pair.long_exposure)
            else:                                            # thresholded copies: the series' images stay as they are
                short, long_ = copy.copy(pair.short_exposure), copy.copy(pair.long_exposure)
                short.measurand, long_.measurand = copy.deepcopy(short.measurand), copy.deepcopy(long_.measurand)
                short.measurand.apply_thresholds(lower, upper)
                long_.measurand.apply_thresholds(lower, upper)
                ab, rel = ImageSet.compute_difference(short, long_)
            out.append((ab.measurand.compute_channel_histogram(bins, included_range, channels, use_std),
                        rel.measurand.compute_channel_histogram(bins, included_range, channels, use_std)))
        return out

    def collect_exposure_pair_stats(self, return_cupy: Optional[bool] = False):
        rel = {"ratios": [], "means": [], "stds": [], "errors": []}
        ab = {"ratios": [], "means": [], "stds": [], "errors": []}
        for p in self.exposure_pairs:
            for res, st in ((ab, p.absolute_stats), (rel, p.relative_stats)):
                res["ratios"].append(p.exposure_ratio)
                res["means"].append(_host(st["mean"]))
                res["stds"].append(_host(st["std"]))
                res["errors"].append(_host(st["error"]))
        return _to_2d_array(ab), _to_2d_array(rel)


def _host(x):
    return None if x is None else (x.cpu().numpy() if isinstance(x, torch.Tensor) else x)


def _to_2d_array(dictionary: Dict):
    return {k: np.array(v) for k, v in dictionary.items()}


def map_linearity_limits(lower_limit: Optional[int], upper_limit: Optional[int], ICRF):
    """modules/general_functions.py:97-131 (host; returns per-channel lists)."""
    n = gs.NUM_OF_CHS
    lower = np.array([gs.LOWER_LIN_LIM if lower_limit is None else lower_limit] * n, dtype="float64")
    upper = np.array([gs.UPPER_LIN_LIM if upper_limit is None else gs.MAX_DN - upper_limit] * n, dtype="float64")
    if ICRF is None:
        lower /= gs.MAX_DN
        upper /= gs.MAX_DN
    else:
        icrf = ICRF.cpu().numpy() if isinstance(ICRF, torch.Tensor) else np.asarray(ICRF)
        for c in range(n):
            lower[c] = icrf[int(lower[c]), c]
            upper[c] = icrf[int(upper[c]), c]
    return list(lower), list(upper)
