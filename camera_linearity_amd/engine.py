"""Functional layer over the C ABI: torch device tensors in, torch device tensors out.

Everything here is plumbing - argument checking, pointer tables, output allocation - around the
hand-written HIP kernels in csrc/. No arithmetic of the hot path happens in Python or in torch ops.
The only host-side numbers are the 256-entry Gaussian weight tables (modules/measurand.py:615-616
evaluated on the DN grid with NumPy, so that they are bit-identical to what the reference computes
for 8-bit frames; 2**bit_depth entries for uint16 frames) and per-frame scalars (1/exposure, DN thresholds).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native as nat
from .settings import BITS, MAX_DN

_F64 = torch.float64
_U8 = torch.uint8
_U16 = torch.uint16


# ---------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------
def _require_cuda(t: torch.Tensor, name: str) -> None:
    """The operand lives where the active library computes: in HBM for the HIP backend - or, inside nat.host_mode() (the explicit
    host backend, Measurand(use_cupy=False)), in host memory. The HIP backend never takes host tensors: there is no CPU fallback."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)} instead.")
    if nat.in_host_mode():
        if t.is_cuda:
            raise RuntimeError(f"{name} lives on {t.device}; the host backend computes on host tensors")
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}; the HIP backend only computes on device tensors "
                           "(there is no CPU fallback)")


class _NoDevice:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _on(device):
    """torch.cuda.device(device) for the HIP backend, nothing for host tensors."""
    return _NoDevice() if torch.device(device).type != "cuda" else torch.cuda.device(device)


def _dev_f64(x, device) -> torch.Tensor:
    """float64 contiguous tensor on `device` from a tensor / ndarray / sequence (tables, not images)."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=_F64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), device=device)


def _ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


_weight_cache: Dict[str, tuple] = {}


def _check_bit_depth(bit_depth) -> int:
    """The bit depth of uint16 DN frames (hm_merge_u16, hm_linearize_u16): an integer in 9..16."""
    if isinstance(bit_depth, bool) or not isinstance(bit_depth, (int, np.integer)) or not 9 <= int(bit_depth) <= 16:
        raise ValueError(f"bit_depth must be an integer in 9..16 for uint16 frames, got {bit_depth!r}")
    return int(bit_depth)


def weight_luts_host(bit_depth: int = 8):
    """w, dw on the DN grid v = k / (2**bit_depth - 1) (8 bits: k/255): modules/measurand.py:615-616 with NumPy (`np.e ** x`)."""
    if bit_depth == 8:
        v = np.arange(BITS, dtype=np.uint8).astype(np.float64) / MAX_DN   # modules/image_set.py:223
    else:
        bit_depth = _check_bit_depth(bit_depth)
        v = np.arange(2 ** bit_depth, dtype=np.uint32).astype(np.float64) / (2 ** bit_depth - 1)
    w = np.e ** (-30 * (v - 0.5) ** 2)
    dw = -2 * 30 * (v - 0.5) * w
    return w, dw


def weight_luts(device, bit_depth: int = 8) -> tuple:
    key = str(torch.device(device)) if bit_depth == 8 else f"{torch.device(device)}/{int(bit_depth)}"
    if key not in _weight_cache:
        w, dw = weight_luts_host(bit_depth)
        _weight_cache[key] = (torch.as_tensor(w, device=device), torch.as_tensor(dw, device=device))
    return _weight_cache[key]


def dark_min_dn(scale: float, threshold: float, bit_depth: Optional[int] = None) -> int:
    """Smallest dark DN that counts as hot: the reference tests `dark.val > threshold`
    (modules/measurand.py:545) with dark.val = (DN/255) * scale (modules/image_set.py:223,260);
    evaluated here for all 256 DNs with the same float64 operations, so the DN-domain comparison the
    kernel performs (`dark_dn >= min_dn`) is exactly equivalent. Returns 256 when no DN is hot.
    bit_depth (9..16, uint16 dark maps of hm_merge_u16_darks): the same evaluation over all 2**bit_depth DNs on DN / (2**bit_depth - 1);
    returns 2**bit_depth when no DN is hot."""
    if bit_depth is None:
        n_dn, v = BITS, np.arange(BITS, dtype=np.uint8).astype(np.float64) / MAX_DN
    else:
        n_dn = 2 ** _check_bit_depth(bit_depth)
        v = np.arange(n_dn, dtype=np.uint32).astype(np.float64) / (n_dn - 1)
    if scale != 1.0:
        v = np.array([scale], dtype=np.float64) * v                       # Measurand(scale) * dark, measurand.py:198
    hot = np.nonzero(v > threshold)[0]
    return int(hot[0]) if hot.size else n_dn


def _stream(device):
    return None if torch.device(device).type != "cuda" else nat.current_stream_ptr(device)


# ---------------------------------------------------------------------------------------------
# rows 1, 3, 4: per-frame kernels
# ---------------------------------------------------------------------------------------------
def u8_to_unit(dn: torch.Tensor) -> torch.Tensor:
    """modules/image_set.py:223."""
    _require_cuda(dn, "dn")
    dn = dn.contiguous()
    out = torch.empty(dn.shape, dtype=_F64, device=dn.device)
    with _on(dn.device):
        nat.check(nat.lib.hm_u8_to_unit_f64(dn.data_ptr(), out.data_ptr(), dn.numel(), _stream(dn.device)), "hm_u8_to_unit_f64")
    return out


def gaussian_weight(val: torch.Tensor):
    """modules/measurand.py:606-618 -> (w, dw)."""
    _require_cuda(val, "val")
    val = val.contiguous()
    w = torch.empty(val.shape, dtype=_F64, device=val.device)
    dw = torch.empty(val.shape, dtype=_F64, device=val.device)
    with _on(val.device):
        if val.dtype == _U8:
            wl, dwl = weight_luts(val.device)
            rc = nat.lib.hm_gaussian_weight_u8(val.data_ptr(), wl.data_ptr(), dwl.data_ptr(), w.data_ptr(), dw.data_ptr(),
                                               val.numel(), _stream(val.device))
        elif val.dtype == _F64:
            rc = nat.lib.hm_gaussian_weight_f64(val.data_ptr(), w.data_ptr(), dw.data_ptr(), val.numel(), _stream(val.device))
        else:
            raise TypeError(f"gaussian_weight expects uint8 or float64, got {val.dtype}")
    nat.check(rc, "hm_gaussian_weight")
    return w, dw


def linearize(val: torch.Tensor, std: Optional[torch.Tensor], icrf, icrf_diff=None, return_index: bool = False, bit_depth: Optional[int] = None):
    """modules/measurand.py:471-541. `icrf` is (256, C) or 1-D (256,). Returns (val, std|None[, idx]).
    torch.uint16 DNs need `bit_depth` in 9..16 (hm_linearize_u16): tables of 2**bit_depth rows, idx = DN & (2**bit_depth - 1) as uint16."""
    _require_cuda(val, "val")
    if val.dtype == _U16:
        bit_depth = _check_bit_depth(bit_depth)
    elif bit_depth is not None:
        raise ValueError(f"bit_depth is for torch.uint16 DNs, got {val.dtype} values")
    n_rows = BITS if bit_depth is None else 2 ** bit_depth
    dev = val.device
    val = val.contiguous()
    icrf_t = _dev_f64(icrf, dev)
    diff_t = None if icrf_diff is None else _dev_f64(icrf_diff, dev)
    C_ = val.shape[-1] if val.dim() > 0 else 1
    if icrf_t.dim() == 1:
        lut_stride = 1
    else:
        if icrf_t.shape[-1] != C_:
            raise ValueError(f"ICRF has {icrf_t.shape[-1]} channels, value has {C_}")
        lut_stride = C_
    if icrf_t.shape[0] != n_rows:
        raise ValueError(f"ICRF must have {n_rows} rows, got {icrf_t.shape[0]}")
    if bit_depth is not None and diff_t is not None and diff_t.shape != icrf_t.shape:
        raise ValueError(f"ICRF_diff must have the ICRF's shape {tuple(icrf_t.shape)}, got {tuple(diff_t.shape)}")
    use_std = std is not None and diff_t is not None                      # measurand.py:498-500
    if use_std:
        _require_cuda(std, "std")
        if std.shape != val.shape:
            raise ValueError("Value and std shapes must match.")
        std = std.to(_F64).contiguous()
    out_val = torch.empty(val.shape, dtype=_F64, device=dev)
    out_std = torch.empty(val.shape, dtype=_F64, device=dev) if use_std else None
    idx = None
    with _on(dev):
        if val.dtype == _U8:
            rc = nat.lib.hm_linearize_u8(val.data_ptr(), nat.ptr(std) if use_std else None, icrf_t.data_ptr(), nat.ptr(diff_t),
                                         out_val.data_ptr(), nat.ptr(out_std), val.numel(), C_, lut_stride, _stream(dev))
            if return_index:
                idx = val.clone()                                          # measurand.py:505
        elif val.dtype == _U16:
            if return_index:
                idx = torch.empty(val.shape, dtype=_U16, device=dev)
            rc = nat.lib.hm_linearize_u16(val.data_ptr(), nat.ptr(std) if use_std else None, icrf_t.data_ptr(), nat.ptr(diff_t),
                                          out_val.data_ptr(), nat.ptr(out_std), nat.ptr(idx), val.numel(), C_, lut_stride, bit_depth,
                                          _stream(dev))
        elif val.dtype == _F64:
            if return_index:
                idx = torch.empty(val.shape, dtype=_U8, device=dev)
            rc = nat.lib.hm_linearize_f64(val.data_ptr(), nat.ptr(std) if use_std else None, icrf_t.data_ptr(), nat.ptr(diff_t),
                                          out_val.data_ptr(), nat.ptr(out_std), nat.ptr(idx), val.numel(), C_, lut_stride,
                                          _stream(dev))
        else:
            raise TypeError(f"linearize expects uint8 or float64 values, got {val.dtype}")
    nat.check(rc, "hm_linearize")
    return (out_val, out_std, idx) if return_index else (out_val, out_std)


# ---------------------------------------------------------------------------------------------
# rows 8, 9 standalone
# ---------------------------------------------------------------------------------------------
def hot_pixel_filter(x: torch.Tensor, dark_map: torch.Tensor, threshold: float, median_k: int,
                     min_dn: Optional[int] = None) -> torch.Tensor:
    """modules/measurand.py:543-557 (intended semantics). `dark_map` is a uint8 DN map (hot iff
    DN >= min_dn; min_dn defaults to dark_min_dn(1.0, threshold)) or a float64 value map (hot iff > threshold)."""
    _require_cuda(x, "x")
    _require_cuda(dark_map, "dark_map")
    if x.dim() != 3 or dark_map.shape != x.shape:
        raise ValueError("hot_pixel_filter expects (H, W, C) arrays of equal shape")
    x = x.contiguous()
    dark_map = dark_map.contiguous()
    H, W, Cc = x.shape
    out = torch.empty_like(x)
    mu8 = dark_map.data_ptr() if dark_map.dtype == _U8 else None
    mf64 = dark_map.data_ptr() if dark_map.dtype == _F64 else None
    if mu8 is None and mf64 is None:
        raise TypeError("dark map must be uint8 or float64")
    if min_dn is None:
        min_dn = dark_min_dn(1.0, threshold)
    fn = {_U8: nat.lib.hm_hot_pixel_filter_u8, _F64: nat.lib.hm_hot_pixel_filter_f64}.get(x.dtype)
    if fn is None:
        raise TypeError("hot_pixel_filter expects uint8 or float64 data")
    with _on(x.device):
        nat.check(fn(x.data_ptr(), mu8, mf64, int(min_dn), float(threshold), int(median_k), out.data_ptr(), H, W, Cc,
                     _stream(x.device)), "hm_hot_pixel_filter")
    return out


def flat_roi_bounds(size_x: int, size_y: int, p: float):
    """modules/measurand.py:570-576 with the integer ROI index."""
    import math
    dx = math.floor(size_x * p)
    dy = math.floor(size_y * p)
    i = (math.floor(1 / p) - 1) // 2
    return i * dx, (i + 1) * dx, i * dy, (i + 1) * dy


def roi_mean(img: torch.Tensor, x0: int, x1: int, y0: int, y1: int) -> torch.Tensor:
    """modules/measurand.py:579 - per-channel mean over img[x0:x1, y0:y1, :] (uint8 images are DN/255)."""
    _require_cuda(img, "img")
    if img.dim() != 3:
        raise ValueError("roi_mean expects an (H, W, C) image")
    img = img.contiguous()
    H, W, Cc = img.shape
    out = torch.empty(Cc, dtype=_F64, device=img.device)
    ws = torch.empty(nat.lib.hm_roi_mean_workspace_bytes() // 8, dtype=_F64, device=img.device)
    fn = {_U8: nat.lib.hm_roi_mean_u8, _F64: nat.lib.hm_roi_mean_f64}.get(img.dtype)
    if fn is None:
        raise TypeError("roi_mean expects uint8 or float64")
    with _on(img.device):
        nat.check(fn(img.data_ptr(), H, W, Cc, x0, x1, y0, y1, out.data_ptr(), ws.data_ptr(), _stream(img.device)), "hm_roi_mean")
    return out


def normalize_by_map(val: torch.Tensor, std: Optional[torch.Tensor], flat: torch.Tensor, flat_std: Optional[torch.Tensor],
                     ff_mean, ff_std_mean=None):
    """modules/measurand.py:585-604. `flat` uint8 DN or float64; means are host sequences of C floats."""
    _require_cuda(val, "val")
    val = val.contiguous()
    flat = flat.contiguous()
    Cc = val.shape[-1]
    m = (C.c_double * nat.HM_MAX_CHANNELS)(*[float(x) for x in ff_mean])
    s = (C.c_double * nat.HM_MAX_CHANNELS)(*[float(x) for x in (ff_std_mean if ff_std_mean is not None else [0.0] * Cc)])
    out_val = torch.empty_like(val)
    out_std = torch.empty_like(val) if std is not None else None
    with _on(val.device):
        nat.check(nat.lib.hm_normalize_by_map(
            val.data_ptr(), nat.ptr(std.contiguous()) if std is not None else None,
            flat.data_ptr() if flat.dtype == _U8 else None, flat.data_ptr() if flat.dtype == _F64 else None,
            nat.ptr(flat_std.contiguous()) if flat_std is not None else None,
            C.cast(m, C.POINTER(C.c_double)), C.cast(s, C.POINTER(C.c_double)),
            out_val.data_ptr(), nat.ptr(out_std), val.numel(), Cc, _stream(val.device)), "hm_normalize_by_map")
    return out_val, out_std


# ---------------------------------------------------------------------------------------------
# rows 5-9 fused: the merge
# ---------------------------------------------------------------------------------------------
class MergePlan:
    """A validated hm_merge_args plus the tensors it points into (kept alive until the plan dies).
    `launch()` enqueues the fused kernel on the current stream of the plan's device; it can be called
    repeatedly (bench, hipGraph capture)."""

    def __init__(self, args: nat.MergeArgs, keep: list, device, outputs: dict, std_table: Optional[torch.Tensor] = None, stds_f32=None,
                 frames_u16=None, bit_depth: Optional[int] = None, darks_u16=None):
        self.args = args
        self._keep = keep
        self.device = torch.device(device)
        self.outputs = outputs
        self._ref = C.byref(args)
        self.host = self.device.type != "cuda"             # a plan of the host backend (built inside nat.host_mode())
        self.std_table = std_table                         # float64 per-DN std table: the plan goes through hm_merge_std_table ((256, C)), with
                                                           # uint16 frames through hm_merge_u16_std_table ((2**bit_depth, C))
        # the C entry point the plan goes through and the entry's own argument after the struct: the ctypes array of N pointers to float32
        # std frames (hm_merge_std_f32), the table, or none
        self.bit_depth = bit_depth                         # uint16 DN frames: the plan goes through hm_merge_u16 (ctypes array of N frame pointers, depth)
        self._bytes_extra = ()                             # what the entry's _algorithmic_bytes form takes after the struct
        if frames_u16 is not None and std_table is not None:         # ... with the per-DN std table, with or without uint16 dark maps
            self._entry, self._bytes_extra = "hm_merge_u16_std_table", (darks_u16,)
            self._extra = (frames_u16, darks_u16, std_table.data_ptr(), int(bit_depth))
        elif darks_u16 is not None:                        # ... with uint16 dark maps: hm_merge_u16_darks (ctypes array of N map pointers or NULLs)
            self._entry, self._extra, self._bytes_extra = "hm_merge_u16_darks", (frames_u16, darks_u16, int(bit_depth)), (darks_u16,)
        elif frames_u16 is not None:
            self._entry, self._extra = "hm_merge_u16", (frames_u16, int(bit_depth))
        elif stds_f32 is not None:
            self._entry, self._extra = "hm_merge_std_f32", (stds_f32,)
        elif std_table is not None:
            self._entry, self._extra = "hm_merge_std_table", (std_table.data_ptr(),)
        else:
            self._entry, self._extra = "hm_merge", ()
        lib = nat.host_lib() if self.host else nat.hip_lib
        self._run = getattr(lib, self._entry)
        self._describe = getattr(lib, self._entry + "_describe")
        self._bytes = getattr(nat.hip_lib, self._entry + "_algorithmic_bytes")

    def launch(self, stream: Optional[int] = None) -> None:
        if self.host:
            with nat.host_mode():
                nat.check(self._run(self._ref, *self._extra, None), self._entry)
            return
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if torch.cuda.current_device() == self.device.index:
            rc = self._run(self._ref, *self._extra, stream)
        else:
            with _on(self.device):
                rc = self._run(self._ref, *self._extra, stream)
        if rc:
            nat.check(rc, self._entry)

    @property
    def algorithmic_bytes(self) -> int:
        return int(self._bytes(self._ref, *self._bytes_extra))

    @property
    def kernels(self) -> str:
        """Names of the kernels launch() dispatches to, in launch order (the entry's _describe form: the library's own dispatch, dry)."""
        buf = C.create_string_buffer(512)
        nat.check(self._describe(self._ref, *self._extra, buf, 512), self._entry + "_describe")
        return buf.value.decode()


def plan_merge(frames: Sequence[torch.Tensor], exposures: Sequence[float], icrf, icrf_diff=None,
               stds: Optional[Sequence[torch.Tensor]] = None,
               darks: Optional[Sequence[Optional[torch.Tensor]]] = None,
               dark_min: Optional[Sequence[int]] = None, median_k: int = 3,
               flat: Optional[torch.Tensor] = None, flat_std: Optional[torch.Tensor] = None,
               ff_mean=None, ff_std_mean=None, want_sum_w: bool = False, want_val: bool = True,
               height: Optional[int] = None, row0: int = 0, rows: Optional[int] = None, buf_row0: int = 0,
               variant: int = 0, hot_queue: bool = True, out_dtype: torch.dtype = torch.float64, std_table=None,
               bit_depth: Optional[int] = None) -> MergePlan:
    """Build the launch descriptor for one fused merge (modules/exposure_series.py:317-419).

    frames : N tensors (buf_rows, W, C), all uint8 DNs or all float64 values, ascending exposure.
             They cover image rows [buf_row0, buf_row0 + buf_rows) of an image `height` rows tall;
             the call produces rows [row0, row0 + rows). Defaults: the buffers are the whole image.
    stds   : N std tensors with the frames' shape. Tensors that are ALL torch.float32 (what ImageSet.save_32bit writes and a float32
             Measurand keeps) are read by the kernels as they are (hm_merge_std_f32: made contiguous, never copied into float64) when there
             are at most HM_MAX_FRAMES frames and no forced chunking (variant > -2). Anything else - float64, mixed dtypes, float16 /
             bfloat16, float32 with more frames or forced chunking - is widened to float64 first. The outputs are the same bits either way:
             widening float32 loses nothing and each std is widened once inside the kernel.
    darks  : per frame a uint8 dark DN map covering the same rows as the frames, or None;
             dark_min[i] = smallest hot DN (see dark_min_dn()). hot_queue: give the hot-pixel pass its queue workspace
             (hm_merge_hot_workspace_bytes: 1 byte per output element) so that it stays balanced on dense maps;
             False = the workspace-free path (one hot element per wave at a time; sparse maps only).
    flat, flat_std : flat-field value (uint8 DN or float64) and float64 uncertainty covering the
             OUTPUT rows; ff_mean / ff_std_mean are the C ROI means (host floats).
    out_dtype : torch.float64 (default) or torch.float32 - the element type of the `val` / `std` outputs (hm_merge_args.out_kind).
             All arithmetic is float64 either way; float32 rounds the float64 result once, to nearest even, at the kernel's store, so
             the outputs equal the float64 outputs cast to float32 - with half the output bytes. `sum_w` stays float64. More than
             HM_MAX_FRAMES frames (and a forced chunking, variant <= -2) exist for float64 only: NotImplementedError.
    std_table : (256, C) array or tensor - the per-DN STD table of ImageSet.calculate_numerical_STD (video_processing.
             noise_profiles_to_STD_data) instead of `stds`: frame i's std is std_table[idx_i, c], formed inside the kernel from the table in LDS
             (hm_merge_std_table), so no std frame exists in device memory. The outputs equal those of `stds=[linearize(f, None,
             std_table)[0] for f in frames]`, bit for bit. Needs icrf_diff; excludes `stds` (ValueError). At most HM_MAX_FRAMES frames
             and no forced chunking: NotImplementedError.
    bit_depth : 9..16, required for (and only for) torch.uint16 DN frames of 9- to 16-bit cameras (hm_merge_u16): ValueError otherwise. A DN
             has the value DN / (2**bit_depth - 1) and the table index DN & (2**bit_depth - 1); `icrf` / `icrf_diff` must have
             2**bit_depth rows, the weight tables are weight_luts(device, bit_depth). float32 stds are widened to float64. `darks` are
             torch.uint16 maps of the frames' shape (hm_merge_u16_darks): frame i is hot where (dark DN & (2**bit_depth - 1)) >=
             dark_min[i], thresholds 1 .. 2**bit_depth (dark_min_dn(scale, threshold, bit_depth)); `median_k` and `hot_queue` as for 8-bit
             frames (False: the patch kernel tests every element itself). Not built for such frames - NotImplementedError: `std_table`
             (their (2**bit_depth, C) table goes through plan_merge_u16_std_table), dark maps of another dtype, a uint8 `flat`, more than
             HM_MAX_FRAMES frames (or forced chunking).
             variant: 0 the library's choice, -1 one element per thread, 1 / 2 / 3 the streaming kernel with its tables in LDS / in global
             memory / split between the two.
    """
    return _plan_merge(frames, exposures, icrf, icrf_diff, stds, darks, dark_min, median_k, flat, flat_std, ff_mean, ff_std_mean, want_sum_w,
                       want_val, height, row0, rows, buf_row0, variant, hot_queue, out_dtype, std_table, bit_depth, u16_table=False)


def _plan_merge(frames, exposures, icrf, icrf_diff, stds, darks, dark_min, median_k, flat, flat_std, ff_mean, ff_std_mean, want_sum_w,
                want_val, height, row0, rows, buf_row0, variant, hot_queue, out_dtype, std_table, bit_depth, u16_table) -> MergePlan:
    """plan_merge's body. u16_table: the call is plan_merge_u16_std_table's - uint16 frames with the (2**bit_depth, C) per-DN std table."""
    if out_dtype not in (_F64, torch.float32):
        raise TypeError(f"out_dtype must be torch.float64 or torch.float32, got {out_dtype}")
    n = len(frames)
    if n == 0:
        raise ValueError("merge needs at least one frame")
    for i, f in enumerate(frames):
        _require_cuda(f, f"frames[{i}]")
    dev = frames[0].device
    dt = frames[0].dtype
    u16 = dt == _U16
    if u16:
        bit_depth = _check_bit_depth(bit_depth)
        if std_table is not None and not u16_table:
            raise NotImplementedError("uint16 frames: plan_merge(std_table=...) takes the (256, C) table of 8-bit frames; the per-DN std table "
                                      "of a 9- to 16-bit camera goes through plan_merge_u16_std_table / merge_u16_std_table")
        if darks is not None and any(d is not None and d.dtype != _U16 for d in darks):
            raise NotImplementedError("uint16 frames: uint16 dark maps are expected (hm_merge_u16_darks); uint8 and other dark map dtypes "
                                      "are built for 8-bit frames only")
        if flat is not None and flat.dtype == _U8:
            raise NotImplementedError("uint16 frames: a uint8 flat field is built for 8-bit frames only (pass a float64 flat)")
        if n > nat.HM_MAX_FRAMES or variant <= -2:
            raise NotImplementedError(f"uint16 frames: at most {nat.HM_MAX_FRAMES} frames in one launch (no chunked path)")
    elif u16_table:
        raise TypeError(f"plan_merge_u16_std_table takes torch.uint16 frames, got {dt}")
    elif bit_depth is not None:
        raise ValueError(f"bit_depth is for torch.uint16 frames, got {dt} frames")
    if dt not in (_U8, _F64, _U16):
        raise TypeError(f"frames must be uint8, float64 or (with bit_depth) uint16, got {dt}")
    n_rows = 2 ** bit_depth if u16 else BITS
    shape = tuple(frames[0].shape)
    if len(shape) != 3:
        raise ValueError(f"frames must be (H, W, C), got shape {shape}")
    keep: list = []
    fr = []
    for i, f in enumerate(frames):
        if f.device != dev or f.dtype != dt or tuple(f.shape) != shape:
            raise ValueError("all frames must share device, dtype and shape")
        f = f.contiguous()
        fr.append(f)
    keep.extend(fr)
    buf_rows, W, Cc = shape
    height = buf_rows + buf_row0 if height is None else int(height)
    rows = (buf_row0 + buf_rows - row0) if rows is None else int(rows)
    if len(exposures) != n:
        raise ValueError("one exposure per frame is required")
    if std_table is not None:
        if stds is not None:
            raise ValueError("std_table and stds are mutually exclusive: the table takes the place of the std frames")
        if icrf_diff is None:
            raise ValueError("ICRF_diff is required to propagate uncertainty")
        if n > nat.HM_MAX_FRAMES or variant <= -2:
            raise NotImplementedError(f"std_table merges take at most {nat.HM_MAX_FRAMES} frames in one launch (the chunked path reads std frames)")
    with_std = stds is not None or std_table is not None
    sd, sd_f32 = [], False
    if stds is not None:
        if len(stds) != n:
            raise ValueError("one std frame per value frame is required")
        if icrf_diff is None:
            raise ValueError("ICRF_diff is required to propagate uncertainty")
        for i, s in enumerate(stds):
            _require_cuda(s, f"stds[{i}]")
            if tuple(s.shape) != shape:
                raise ValueError("Value and std shapes must match.")
        # float32 std frames as they are (hm_merge_std_f32) where one launch takes the stack; everything else widened, as ever
        sd_f32 = all(s.dtype == torch.float32 for s in stds) and n <= nat.HM_MAX_FRAMES and variant > -2 and not u16
        sd = [s.contiguous() if sd_f32 else s.to(_F64).contiguous() for s in stds]
        keep.extend(sd)
    icrf_t = _dev_f64(icrf, dev)
    if tuple(icrf_t.shape) != (n_rows, Cc):
        raise ValueError(f"ICRF must have shape ({n_rows}, {Cc}), got {tuple(icrf_t.shape)}")
    diff_t = None
    if icrf_diff is not None:
        diff_t = _dev_f64(icrf_diff, dev)
        if tuple(diff_t.shape) != (n_rows, Cc):
            raise ValueError(f"ICRF_diff must have shape ({n_rows}, {Cc})")
    w_lut, dw_lut = weight_luts(dev, bit_depth) if u16 else weight_luts(dev)
    keep += [icrf_t, diff_t, w_lut, dw_lut]
    table_t = None
    if std_table is not None:
        table_t = _dev_f64(std_table, dev)
        if tuple(table_t.shape) != (n_rows, Cc):
            raise ValueError(f"std_table must have shape ({n_rows}, {Cc}), got {tuple(table_t.shape)}")
        keep.append(table_t)

    a = nat.MergeArgs()
    a.struct_size = C.sizeof(nat.MergeArgs)
    a.n_frames, a.channels, a.variant = n, Cc, int(variant)
    a.out_kind = nat.HM_OUT_F32 if out_dtype == torch.float32 else nat.HM_OUT_F64
    a.height, a.width, a.row0, a.rows, a.buf_row0, a.buf_rows = height, W, int(row0), rows, int(buf_row0), buf_rows
    fptrs, sptrs = _ptr_array(fr), None
    if u16:
        pass                                               # hm_merge_u16 takes the frame pointers beside the struct
    elif dt == _U8:
        a.frames_u8 = C.cast(fptrs, C.POINTER(C.c_void_p))
    else:
        a.frames_f64 = C.cast(fptrs, C.POINTER(C.c_void_p))
    keep.append(fptrs)
    if stds is not None:
        sptrs = _ptr_array(sd)
        if not sd_f32:
            a.stds = C.cast(sptrs, C.POINTER(C.c_void_p))
        keep.append(sptrs)
    exp = (C.c_double * n)(*[float(t) for t in exposures])
    a.exposures = C.cast(exp, C.POINTER(C.c_double))
    keep.append(exp)
    a.icrf, a.icrf_diff = icrf_t.data_ptr(), nat.ptr(diff_t)
    a.w_lut, a.dw_lut = w_lut.data_ptr(), dw_lut.data_ptr()
    darks_u16 = None
    if darks is not None and any(d is not None for d in darks):
        if len(darks) != n or dark_min is None or len(dark_min) != n:
            raise ValueError("darks and dark_min need one entry per frame")
        dk = []
        for i, d in enumerate(darks):
            if d is None:
                dk.append(None)
                continue
            _require_cuda(d, f"darks[{i}]")
            if d.dtype != (_U16 if u16 else _U8) or tuple(d.shape) != shape:
                raise ValueError(f"dark maps must be {'uint16' if u16 else 'uint8'} with the frames' shape")
            dk.append(d.contiguous())
        dptrs = _ptr_array(dk)
        dmin = (C.c_int32 * n)(*[int(x) for x in dark_min])
        if u16:
            darks_u16 = dptrs                              # hm_merge_u16_darks takes the map pointers beside the struct
        else:
            a.darks_u8 = C.cast(dptrs, C.POINTER(C.c_void_p))
        a.dark_min_dn = C.cast(dmin, C.POINTER(C.c_int32))
        a.median_k = int(median_k)
        keep += [dk, dptrs, dmin]
        if hot_queue:
            ws_bytes = int(nat.lib.hm_merge_hot_workspace_bytes(rows * W * Cc))
            ws = torch.empty(ws_bytes, dtype=_U8, device=dev)          # torch allocations are 512-byte aligned
            a.hot_workspace, a.hot_workspace_bytes = ws.data_ptr(), ws_bytes
            keep.append(ws)
    out_shape = (rows, W, Cc)
    if flat is not None:
        _require_cuda(flat, "flat")
        if tuple(flat.shape) != out_shape:
            raise ValueError(f"flat field must cover the output rows: expected {out_shape}, got {tuple(flat.shape)}")
        flat = flat.contiguous()
        if flat.dtype == _U8:
            a.flat_u8 = flat.data_ptr()
        elif flat.dtype == _F64:
            a.flat_f64 = flat.data_ptr()
        else:
            raise TypeError("flat must be uint8 or float64")
        if ff_mean is None:
            raise ValueError("ff_mean is required with a flat field")
        for c in range(Cc):
            a.ff_mean[c] = float(ff_mean[c])
        keep.append(flat)
        if with_std:
            if flat_std is None or ff_std_mean is None:
                raise ValueError("flat_std and ff_std_mean are required to propagate uncertainty through the flat field")
            _require_cuda(flat_std, "flat_std")
            flat_std = flat_std.to(_F64).contiguous()
            if tuple(flat_std.shape) != out_shape:
                raise ValueError("flat_std must cover the output rows")
            a.flat_std = flat_std.data_ptr()
            for c in range(Cc):
                a.ff_std_mean[c] = float(ff_std_mean[c])
            keep.append(flat_std)
    outputs = {}
    if want_val:
        outputs["val"] = torch.empty(out_shape, dtype=out_dtype, device=dev)
        a.out_val = outputs["val"].data_ptr()
        if with_std:
            outputs["std"] = torch.empty(out_shape, dtype=out_dtype, device=dev)
            a.out_std = outputs["std"].data_ptr()
    if want_sum_w:
        outputs["sum_w"] = torch.empty(out_shape, dtype=_F64, device=dev)
        a.out_sum_w = outputs["sum_w"].data_ptr()
    # more than HM_MAX_FRAMES frames (or a forced chunking, variant <= -2): hm_merge runs HM_MAX_FRAMES frames per launch and keeps the
    # running sum of weights in out_sum_w, or in this workspace when the call has none
    fw = int(nat.lib.hm_merge_frames_workspace_bytes(n if variant > -2 else nat.HM_MAX_FRAMES + 1, rows * W * Cc, int(want_sum_w)))
    if fw:
        ws = torch.empty(fw, dtype=_U8, device=dev)
        a.frames_workspace, a.frames_workspace_bytes = ws.data_ptr(), fw
        keep.append(ws)
    plan = MergePlan(a, keep, dev, outputs, std_table=table_t, stds_f32=sptrs if sd_f32 else None,
                     frames_u16=fptrs if u16 else None, bit_depth=bit_depth, darks_u16=darks_u16)
    if out_dtype == torch.float32 or table_t is not None or sd_f32 or u16:
        plan.kernels                       # the library's own dispatch, dry: what it refuses for float32 outputs / table calls raises here, not at the first launch
    return plan


def plan_merge_u16_std_table(frames: Sequence[torch.Tensor], exposures: Sequence[float], icrf, icrf_diff, std_table, *, bit_depth: int,
                             darks: Optional[Sequence[Optional[torch.Tensor]]] = None, dark_min: Optional[Sequence[int]] = None,
                             median_k: int = 3, hot_queue: bool = True, flat: Optional[torch.Tensor] = None,
                             flat_std: Optional[torch.Tensor] = None, ff_mean=None, ff_std_mean=None, want_sum_w: bool = False,
                             want_val: bool = True, height: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                             buf_row0: int = 0, variant: int = 0, out_dtype: torch.dtype = torch.float64) -> MergePlan:
    """plan_merge for torch.uint16 DN frames of a 9- to 16-bit camera with the per-frame stds taken from the camera's per-DN STD table
    (hm_merge_u16_std_table): std_table is (2**bit_depth, C) - what noise_moments_to_STD_data makes - and frame i's std at an element of
    channel c is std_table[DN_i & (2**bit_depth - 1), c], formed inside the kernels, so no std frame exists in device memory. The outputs
    equal those of plan_merge(..., stds=[linearize(f, None, std_table, bit_depth=bit_depth)[0] for f in frames], bit_depth=bit_depth), bit
    for bit; with `darks` (torch.uint16 maps, as plan_merge takes them for such frames) a hot frame's std is the k x k median of the table
    mapped over its neighbourhood. Everything else - flat field, row tiles, out_dtype, variant - is plan_merge's for uint16 frames, and so
    is what it refuses (NotImplementedError: more than HM_MAX_FRAMES frames, variant <= -2, uint8 dark maps, a uint8 flat). ValueError: no
    icrf_diff, a table that is not (2**bit_depth, C). There is no `stds` argument: the table takes the place of the std frames."""
    if icrf_diff is None:
        raise ValueError("ICRF_diff is required to propagate uncertainty")
    if std_table is None:
        raise ValueError("std_table is required: the (2**bit_depth, C) per-DN STD table")
    return _plan_merge(frames, exposures, icrf, icrf_diff, None, darks, dark_min, median_k, flat, flat_std, ff_mean, ff_std_mean, want_sum_w,
                       want_val, height, row0, rows, buf_row0, variant, hot_queue, out_dtype, std_table, bit_depth, u16_table=True)


def merge_u16_std_table(frames, exposures, icrf, icrf_diff, std_table, **kw) -> dict:
    """plan_merge_u16_std_table(...).launch(); returns {'val', 'std', 'sum_w'?} device tensors."""
    plan = plan_merge_u16_std_table(frames, exposures, icrf, icrf_diff, std_table, **kw)
    plan.launch()
    return plan.outputs


def merge(frames, exposures, icrf, icrf_diff=None, stds=None, **kw) -> dict:
    """plan_merge(...).launch(); returns {'val', 'std'?, 'sum_w'?} device tensors (`std_table=`: see plan_merge)."""
    plan = plan_merge(frames, exposures, icrf, icrf_diff, stds, **kw)
    plan.launch()
    return plan.outputs


class PlanGraph:
    """A sequence of merge plans recorded ONCE into a hipGraph and replayed with one host call.

    The library makes no synchronising call, allocates nothing and copies nothing (every entry point only enqueues kernels on the stream it
    is given; workspaces are the caller's), so whatever `MergePlan.launch()` enqueues - the streaming kernel, the dark-map scan and patch,
    the launches of a chunked stack - is capturable as it is. What a graph saves is host time: ~6 us of ctypes + argument checking +
    kernel-argument packing per hm_merge call, which is the whole cost of a small stack (BASELINE config 1, 3 x 256 x 256 x 3: the kernel
    runs for ~3 us). Streams of LARGE stacks gain nothing (the device is busy for longer than the host needs to enqueue the next launch).

    The graph holds the plans (and through them every tensor the recorded kernels read or write): inputs are refreshed by copying into
    the plans' frame tensors (`frames[i].copy_(...)`), outputs are read from `plans[i].outputs` after `replay()`.
    """

    def __init__(self, plans: Sequence[MergePlan], warmup: bool = True, lanes: int = 1):
        """lanes > 1: the plans are dealt round-robin onto `lanes` parallel branches of the graph (forked from and joined to the capture
        stream), so that kernels too small to fill 256 CUs overlap; the plans must then be independent of each other (no plan reads what
        another writes)."""
        plans = list(plans)
        if not plans:
            raise ValueError("PlanGraph needs at least one plan")
        if any(p.host for p in plans):
            raise TypeError("PlanGraph records device launches; host-backend plans run synchronously in launch()")
        dev = plans[0].device
        if any(p.device != dev for p in plans):
            raise ValueError("all plans of a graph must live on one device")
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        self.plans = plans
        self.device = dev
        self.lanes = min(int(lanes), len(plans))
        with torch.cuda.device(dev):
            side = torch.cuda.Stream(dev)
            branches = [torch.cuda.Stream(dev) for _ in range(self.lanes - 1)]
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                if warmup:                      # first launches query the kernels' occupancy and load their code objects: outside the capture
                    for p in plans:
                        p.launch()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=side):
                    for b in branches:          # fork
                        b.wait_stream(side)
                    for i, p in enumerate(plans):
                        lane = i % self.lanes
                        p.launch(side.cuda_stream if lane == 0 else branches[lane - 1].cuda_stream)
                    for b in branches:          # join
                        side.wait_stream(b)
            torch.cuda.current_stream(dev).wait_stream(side)

    def replay(self) -> None:
        """Enqueue the recorded launches on the current stream of the graph's device."""
        if torch.cuda.current_device() == self.device.index:
            self.graph.replay()
        else:
            with torch.cuda.device(self.device):
                self.graph.replay()


def sum_of_weights(frames, darks=None, dark_min=None, median_k: int = 3, **kw):
    """modules/exposure_series.py:317-345 -> (S, S**2) as device tensors. uint16 frames: with `bit_depth=` (and uint16 `darks`)."""
    Cc = frames[0].shape[-1]
    n_rows = 2 ** _check_bit_depth(kw.get("bit_depth")) if frames[0].dtype == _U16 else BITS
    ident = np.zeros((n_rows, Cc))
    plan = plan_merge(frames, [1.0] * len(frames), ident, darks=darks, dark_min=dark_min, median_k=median_k,
                      want_sum_w=True, want_val=False, **kw)
    plan.launch()
    S = plan.outputs["sum_w"]
    return S, elementwise_binary(nat.HM_OP_MUL, S, None, S, None)[0]


# ---------------------------------------------------------------------------------------------
# row 10: operators
# ---------------------------------------------------------------------------------------------
def _bcast_strides(t: torch.Tensor, shape) -> List[int]:
    pad = len(shape) - t.dim()
    st = [0] * pad + list(t.stride())
    sh = [1] * pad + list(t.shape)
    return [0 if sh[d] == 1 and shape[d] != 1 else st[d] for d in range(len(shape))]


def elementwise_binary(op: int, x1: torch.Tensor, s1, x2: torch.Tensor, s2):
    """modules/measurand.py:106-241 for two float64 device operands (NumPy broadcasting)."""
    _require_cuda(x1, "x1")
    _require_cuda(x2, "x2")
    x1 = x1.to(_F64).contiguous()
    x2 = x2.to(_F64).contiguous()
    if s1 is not None:
        s1 = s1.to(_F64).contiguous()
    if s2 is not None:
        s2 = s2.to(_F64).contiguous()
    try:
        shape = torch.broadcast_shapes(x1.shape, x2.shape)
    except RuntimeError:
        raise ValueError("Measurands are not broadcastable.")
    if len(shape) > nat.HM_MAX_DIMS:
        raise NotImplementedError(f"more than {nat.HM_MAX_DIMS} dimensions")
    if len(shape) == 0:
        shape = (1,)
    nd = len(shape)
    out = torch.empty(shape, dtype=_F64, device=x1.device)
    with_std = s1 is not None or s2 is not None
    out_std = torch.empty(shape, dtype=_F64, device=x1.device) if with_std else None
    sh = (C.c_int64 * nd)(*shape)
    st1 = (C.c_int64 * nd)(*_bcast_strides(x1, shape))
    st2 = (C.c_int64 * nd)(*_bcast_strides(x2, shape))
    with _on(x1.device):
        nat.check(nat.lib.hm_binary_op(op, x1.data_ptr(), nat.ptr(s1), x2.data_ptr(), nat.ptr(s2), out.data_ptr(),
                                       nat.ptr(out_std), nd, sh, st1, st2, _stream(x1.device)), "hm_binary_op")
    return out, out_std


def pow_scalar(x: torch.Tensor, s: Optional[torch.Tensor], exponent: float):
    """modules/measurand.py:217-241 for a plain scalar exponent -> (val, std | None); hm_pow_scalar (no pow() for 2, 0.5, 1, small integers)."""
    _require_cuda(x, "val")
    x = x.contiguous()
    s = None if s is None else s.to(_F64).contiguous()
    out = torch.empty_like(x)
    out_s = None if s is None else torch.empty_like(x)
    with _on(x.device):
        nat.check(nat.lib.hm_pow_scalar(x.data_ptr(), nat.ptr(s), float(exponent), out.data_ptr(), nat.ptr(out_s), x.numel(),
                                        _stream(x.device)), "hm_pow_scalar")
    return out, out_s


def elementwise_unary(op: int, x: torch.Tensor, s):
    _require_cuda(x, "x")
    x = x.to(_F64).contiguous()
    if s is not None:
        s = s.to(_F64).contiguous()
    out = torch.empty_like(x)
    out_std = torch.empty_like(x) if s is not None else None
    with _on(x.device):
        nat.check(nat.lib.hm_unary_op(op, x.data_ptr(), nat.ptr(s), out.data_ptr(), nat.ptr(out_std), x.numel(),
                                      _stream(x.device)), "hm_unary_op")
    return out, out_std


# ---------------------------------------------------------------------------------------------
# linearity statistics
# ---------------------------------------------------------------------------------------------
HM_TAKE_MAX = 16          # include/hdrmerge.h


def take_axis(x: torch.Tensor, s: Optional[torch.Tensor], indices: Sequence[int], axis: Optional[int]):
    """modules/measurand.py:352-373 (`lib.take(val, dims, axis)`): axis=None indexes the flattened array."""
    _require_cuda(x, "val")
    x = x.contiguous()
    if s is not None:
        _require_cuda(s, "std")
        s = s.to(_F64).contiguous()
    idx = [int(i) for i in indices]
    if axis is None:
        outer, axis_len, inner, out_shape = 1, x.numel(), 1, (len(idx),)
    else:
        ax = axis % x.dim()
        outer = int(np.prod(x.shape[:ax], dtype=np.int64))
        inner = int(np.prod(x.shape[ax + 1:], dtype=np.int64))
        axis_len = x.shape[ax]
        out_shape = tuple(x.shape[:ax]) + (len(idx),) + tuple(x.shape[ax + 1:])
    if any(i < -axis_len or i >= axis_len for i in idx):
        raise IndexError(f"index out of bounds for axis of size {axis_len}")
    out = torch.empty(out_shape, dtype=_F64, device=x.device)
    out_s = None if s is None else torch.empty(out_shape, dtype=_F64, device=x.device)
    with _on(x.device):
        if len(idx) <= HM_TAKE_MAX:
            arr = (C.c_int64 * len(idx))(*idx)
            nat.check(nat.lib.hm_take_axis(x.data_ptr(), nat.ptr(s), out.data_ptr(), nat.ptr(out_s), outer, axis_len, inner,
                                           arr, len(idx), _stream(x.device)), "hm_take_axis")
        else:
            # np.take has no limit on the number of indices; hm_take_axis takes HM_TAKE_MAX per launch: one launch per chunk into its
            # slice of the dense (outer, n, inner) output (a strided device copy when outer > 1)
            ov = out.view(outer, len(idx), inner)
            osv = None if out_s is None else out_s.view(outer, len(idx), inner)
            for k0 in range(0, len(idx), HM_TAKE_MAX):
                part = idx[k0:k0 + HM_TAKE_MAX]
                arr = (C.c_int64 * len(part))(*part)
                direct = outer == 1
                tv = ov[:, k0:k0 + len(part)] if direct else torch.empty((outer, len(part), inner), dtype=_F64, device=x.device)
                ts = None if s is None else (osv[:, k0:k0 + len(part)] if direct else torch.empty_like(tv))
                nat.check(nat.lib.hm_take_axis(x.data_ptr(), nat.ptr(s), tv.data_ptr(), nat.ptr(ts), outer, axis_len, inner,
                                               arr, len(part), _stream(x.device)), "hm_take_axis")
                if not direct:
                    ov[:, k0:k0 + len(part)].copy_(tv)
                    if ts is not None:
                        osv[:, k0:k0 + len(part)].copy_(ts)
    return out, out_s


def apply_thresholds_(val: torch.Tensor, std: Optional[torch.Tensor], lower: Sequence[float], upper: Sequence[float]) -> None:
    """modules/measurand.py:375-428, in place on contiguous float64 device tensors (last axis = channels)."""
    _require_cuda(val, "val")
    Cc = val.shape[-1]
    lo = (C.c_double * Cc)(*[float(x) for x in lower])
    hi = (C.c_double * Cc)(*[float(x) for x in upper])
    with _on(val.device):
        nat.check(nat.lib.hm_apply_thresholds(val.data_ptr(), nat.ptr(std), lo, hi, val.numel(), Cc, _stream(val.device)),
                  "hm_apply_thresholds")


def _bcast_setup(a, sa, b, sb):
    """Operands of compute_difference / interpolate that do not have one shape: the broadcast result shape and the element strides
    (0 on broadcast axes) of the two contiguous operands; an operand's std must have the operand's shape (one Measurand)."""
    try:
        shape = tuple(torch.broadcast_shapes(a.shape, b.shape))
    except RuntimeError:
        raise ValueError("Measurands are not broadcastable.")
    if len(shape) > nat.HM_MAX_DIMS:
        raise NotImplementedError(f"more than {nat.HM_MAX_DIMS} dimensions")
    if len(shape) == 0:
        shape = (1,)
    for v, s_ in ((a, sa), (b, sb)):
        if s_ is not None and s_.shape != v.shape:
            raise ValueError("Value and std shapes must match.")
    nd = len(shape)
    return shape, (C.c_int64 * nd)(*shape), (C.c_int64 * nd)(*_bcast_strides(a, shape)), (C.c_int64 * nd)(*_bcast_strides(b, shape))


def compute_difference(x, sx, y, sy, multiplier: float):
    """modules/measurand.py:620-655 -> (abs, abs_std, rel, rel_std). Operands of different shapes broadcast (hm_compute_difference_bcast)."""
    _require_cuda(x, "x")
    _require_cuda(y, "y")
    x, y = x.contiguous(), y.contiguous()
    if x.shape != y.shape:
        sx = None if sx is None else sx.contiguous()
        sy = None if sy is None else sy.contiguous()
        shape, sh, st1, st2 = _bcast_setup(x, sx, y, sy)
        with_std = sx is not None or sy is not None
        mk = lambda on: torch.empty(shape, dtype=_F64, device=x.device) if on else None      # noqa: E731
        ad, rd, ads, rds = mk(True), mk(True), mk(with_std), mk(with_std)
        with _on(x.device):
            nat.check(nat.lib.hm_compute_difference_bcast(x.data_ptr(), nat.ptr(sx), y.data_ptr(), nat.ptr(sy), float(multiplier), ad.data_ptr(),
                                                          nat.ptr(ads), rd.data_ptr(), nat.ptr(rds), len(shape), sh, st1, st2, _stream(x.device)),
                      "hm_compute_difference_bcast")
        return ad, ads, rd, rds
    sx = None if sx is None else sx.contiguous()
    sy = None if sy is None else sy.contiguous()
    with_std = sx is not None or sy is not None
    ad, rd = torch.empty_like(x), torch.empty_like(x)
    ads = torch.empty_like(x) if with_std else None
    rds = torch.empty_like(x) if with_std else None
    with _on(x.device):
        nat.check(nat.lib.hm_compute_difference(x.data_ptr(), nat.ptr(sx), y.data_ptr(), nat.ptr(sy), float(multiplier),
                                                ad.data_ptr(), nat.ptr(ads), rd.data_ptr(), nat.ptr(rds), x.numel(),
                                                _stream(x.device)), "hm_compute_difference")
    return ad, ads, rd, rds


def interpolate(x0, s0, x1, s1, y0: float, y1: float, y: float):
    """modules/measurand.py:657-681. Operands of different shapes broadcast (hm_interpolate_bcast)."""
    _require_cuda(x0, "x0")
    _require_cuda(x1, "x1")
    x0, x1 = x0.contiguous(), x1.contiguous()
    s0 = None if s0 is None else s0.contiguous()
    s1 = None if s1 is None else s1.contiguous()
    if x0.shape != x1.shape:
        shape, sh, st0, st1 = _bcast_setup(x0, s0, x1, s1)
        out = torch.empty(shape, dtype=_F64, device=x0.device)
        out_std = torch.empty(shape, dtype=_F64, device=x0.device) if (s0 is not None or s1 is not None) else None
        with _on(x0.device):
            nat.check(nat.lib.hm_interpolate_bcast(x0.data_ptr(), nat.ptr(s0), x1.data_ptr(), nat.ptr(s1), float(y0), float(y1), float(y),
                                                   out.data_ptr(), nat.ptr(out_std), len(shape), sh, st0, st1, _stream(x0.device)),
                      "hm_interpolate_bcast")
        return out, out_std
    out = torch.empty_like(x0)
    out_std = torch.empty_like(x0) if (s0 is not None or s1 is not None) else None
    with _on(x0.device):
        nat.check(nat.lib.hm_interpolate(x0.data_ptr(), nat.ptr(s0), x1.data_ptr(), nat.ptr(s1), float(y0), float(y1), float(y),
                                         out.data_ptr(), nat.ptr(out_std), x0.numel(), _stream(x0.device)), "hm_interpolate")
    return out, out_std


def channel_statistics(val: torch.Tensor, std: Optional[torch.Tensor]):
    """modules/measurand.py:318-350 over every axis but the last -> dict(mean, std, error) of (C,) device tensors."""
    _require_cuda(val, "val")
    val = val.contiguous()
    std = None if std is None else std.contiguous()
    Cc = val.shape[-1]
    out = torch.empty(3 * Cc, dtype=_F64, device=val.device)
    ws = torch.empty(nat.lib.hm_channel_statistics_workspace_bytes() // 8, dtype=_F64, device=val.device)
    with _on(val.device):
        nat.check(nat.lib.hm_channel_statistics(val.data_ptr(), nat.ptr(std), val.numel(), Cc, out.data_ptr(), ws.data_ptr(),
                                                _stream(val.device)), "hm_channel_statistics")
    return {"mean": out[:Cc], "std": out[Cc:2 * Cc], "error": out[2 * Cc:] if std is not None else None}


def axis_statistics(val: torch.Tensor, std: Optional[torch.Tensor], axis):
    """modules/measurand.py:318-350 for any `axis` (int or tuple, NumPy conventions) -> dict(mean, std, error) shaped like NumPy's
    result (the reduced axes removed). Adjacent reduced axes are reduced in place on the dense (outer, A, inner) view
    (hm_axis_statistics), two separate groups of them on the (outer, A1, mid, A2, inner) view (hm_axis_statistics2); only three or more
    separate groups are first brought together (the kept axes in order, then the reduced ones: a layout copy)."""
    _require_cuda(val, "val")
    nd = val.dim()
    axes = sorted({a % nd for a in ((axis,) if isinstance(axis, int) else tuple(axis))})
    if not axes or any(not -nd <= a < nd for a in ((axis,) if isinstance(axis, int) else tuple(axis))):
        raise ValueError(f"axis {axis} is out of bounds for an array of dimension {nd}")
    if std is not None:
        _require_cuda(std, "std")
        if std.shape != val.shape:
            raise ValueError("Value and std shapes must match.")
        std = std.to(_F64)
    kept = [d for d in range(nd) if d not in axes]
    out_shape = tuple(val.shape[d] for d in kept)
    groups = [[axes[0]]]                                       # runs of adjacent reduced axes
    for a_ in axes[1:]:
        if a_ == groups[-1][-1] + 1:
            groups[-1].append(a_)
        else:
            groups.append([a_])
    if len(groups) > 2:                                        # three or more separate groups: bring them together (a layout copy)
        perm = kept + axes
        val = val.permute(perm)
        std = None if std is None else std.permute(perm)
        groups = [list(range(len(kept), nd))]
    val = val.contiguous()
    std = None if std is None else std.contiguous()
    sh = list(val.shape)
    prod = lambda lo, hi: int(np.prod(sh[lo:hi], dtype=np.int64))   # noqa: E731
    if prod(0, len(sh)) == 0:
        raise ValueError("statistics of an empty array")
    dev = val.device
    mean = torch.empty(out_shape, dtype=_F64, device=dev)
    sd = torch.empty(out_shape, dtype=_F64, device=dev)
    err = torch.empty(out_shape, dtype=_F64, device=dev) if std is not None else None
    if len(groups) == 1:
        g = groups[0]
        outer, A, inner = prod(0, g[0]), prod(g[0], g[-1] + 1), prod(g[-1] + 1, len(sh))
        ws_b = int(nat.lib.hm_axis_statistics_workspace_bytes(outer, A, inner))
        ws = torch.empty(max(1, ws_b // 8), dtype=_F64, device=dev)
        with _on(dev):
            nat.check(nat.lib.hm_axis_statistics(val.data_ptr(), nat.ptr(std), outer, A, inner, mean.data_ptr(), sd.data_ptr(), nat.ptr(err),
                                                 ws.data_ptr(), _stream(dev)), "hm_axis_statistics")
    else:                                                      # two groups with kept axes between them: reduced in place, no layout copy
        g1, g2 = groups
        dims = (prod(0, g1[0]), prod(g1[0], g1[-1] + 1), prod(g1[-1] + 1, g2[0]), prod(g2[0], g2[-1] + 1), prod(g2[-1] + 1, len(sh)))
        ws_b = int(nat.lib.hm_axis_statistics2_workspace_bytes(*dims))
        ws = torch.empty(max(1, ws_b // 8), dtype=_F64, device=dev)
        with _on(dev):
            nat.check(nat.lib.hm_axis_statistics2(val.data_ptr(), nat.ptr(std), *dims, mean.data_ptr(), sd.data_ptr(), nat.ptr(err),
                                                  ws.data_ptr(), _stream(dev)), "hm_axis_statistics2")
    return {"mean": mean, "std": sd, "error": err}


def pair_statistics(x, sx, y, sy, multiplier: float):
    """ExposurePair.compute_difference + compute_stats(axis=(0,1)) in one fused reduction (no difference images):
    -> (absolute_stats, relative_stats), each dict(mean, std, error) of (C,) device tensors."""
    _require_cuda(x, "x")
    _require_cuda(y, "y")
    if x.shape != y.shape:
        raise ValueError("pair statistics need frames of equal shape")
    x, y = x.contiguous(), y.contiguous()
    sx = None if sx is None else sx.contiguous()
    sy = None if sy is None else sy.contiguous()
    Cc = x.shape[-1]
    out = torch.empty(6 * Cc, dtype=_F64, device=x.device)
    ws = torch.empty(nat.lib.hm_pair_statistics_workspace_bytes() // 8, dtype=_F64, device=x.device)
    with _on(x.device):
        nat.check(nat.lib.hm_pair_statistics(x.data_ptr(), nat.ptr(sx), y.data_ptr(), nat.ptr(sy), float(multiplier), x.numel(), Cc,
                                             out.data_ptr(), ws.data_ptr(), _stream(x.device)), "hm_pair_statistics")
    w = sx is not None or sy is not None
    mk = lambda o: {"mean": out[o:o + Cc], "std": out[o + Cc:o + 2 * Cc], "error": out[o + 2 * Cc:o + 3 * Cc] if w else None}   # noqa: E731
    return mk(0), mk(3 * Cc)


def pairs_statistics(vals: Sequence[torch.Tensor], stds: Optional[Sequence[torch.Tensor]], pairs: Sequence[tuple], to_host: bool = False,
                     thresholds: Optional[tuple] = None):
    """Statistics of the absolute and relative difference of EVERY exposure pair of a stack in one fused launch
    (hm_pairs_statistics; modules/exposure_series.py:421-446). `pairs` = [(i, j, multiplier), ...] with i the short and j the
    long exposure. Returns one (abs_stats, rel_stats) tuple of dicts per pair, as pair_statistics() does.
    thresholds = (lower, upper), C numbers each: apply_thresholds(lower, upper) is applied to every frame (and std) IN PLACE first,
    fused into the launch's loads - the frames must then be the contiguous float64 tensors the caller keeps."""
    n = len(vals)
    for i, v in enumerate(vals):
        _require_cuda(v, f"vals[{i}]")
        if v.shape != vals[0].shape or v.dtype != _F64:
            raise ValueError("pairs_statistics needs float64 frames of one shape")
    dev = vals[0].device
    if thresholds is not None and (any(not v.is_contiguous() for v in vals) or
                                   (stds is not None and any(s is None or s.dtype != _F64 or not s.is_contiguous() for s in stds))):
        raise ValueError("in-place thresholds need contiguous float64 frames (and stds)")
    vals = [v.contiguous() for v in vals]
    if stds is not None:
        if len(stds) != n or any(s is None for s in stds):
            raise ValueError("one std frame per value frame (or none at all)")
        stds = [s.to(_F64).contiguous() for s in stds]
    Cc = vals[0].shape[-1]
    lo = hi = None
    if thresholds is not None:
        if len(thresholds[0]) != Cc or len(thresholds[1]) != Cc:
            raise ValueError("The length of 'lower' and 'upper' must match the size of the independent axis.")
        lo = (C.c_double * Cc)(*[float(x) for x in thresholds[0]])
        hi = (C.c_double * Cc)(*[float(x) for x in thresholds[1]])
    P = len(pairs)
    vp = _ptr_array(vals)
    sp = None if stds is None else _ptr_array(stds)
    pi = (C.c_int32 * P)(*[int(p[0]) for p in pairs])
    pj = (C.c_int32 * P)(*[int(p[1]) for p in pairs])
    pm = (C.c_double * P)(*[float(p[2]) for p in pairs])
    out = torch.empty(P * 6 * Cc, dtype=_F64, device=dev)
    ws = torch.empty(max(1, nat.lib.hm_pairs_statistics_workspace_bytes(P) // 8), dtype=_F64, device=dev)
    with _on(dev):
        nat.check(nat.lib.hm_pairs_statistics(C.cast(vp, C.POINTER(C.c_void_p)), None if sp is None else C.cast(sp, C.POINTER(C.c_void_p)), n,
                                              pi, pj, pm, P, vals[0].numel(), Cc, lo, hi, out.data_ptr(), ws.data_ptr(), _stream(dev)),
                  "hm_pairs_statistics")
    w = stds is not None
    if to_host:
        out = out.cpu()                                   # one device-to-host copy for all pairs (P * 6C numbers)
    res = []
    for p in range(P):
        b = p * 6 * Cc
        mk = lambda o: {"mean": out[o:o + Cc], "std": out[o + Cc:o + 2 * Cc], "error": out[o + 2 * Cc:o + 3 * Cc] if w else None}   # noqa: E731
        res.append((mk(b), mk(b + 3 * Cc)))
    return res


class _PairsDnArgs:
    """What the entries that read DN frames (pairs_statistics_dn, pairs_histogram_dn) take, checked and kept alive: the DN frames, the
    (2**bit_depth, C) tables on the frames' device, the thresholds and the pair arrays. `what` names the caller in the errors."""

    def __init__(self, what: str, frames: Sequence[torch.Tensor], pairs: Sequence[tuple], icrf, icrf_diff=None, std_table=None, thresholds=None,
                 bit_depth: Optional[int] = None, variant: int = 0):
        frames = list(frames)
        if not frames:
            raise ValueError(f"{what} needs at least one frame")
        for i, f in enumerate(frames):
            _require_cuda(f, f"frames[{i}]")
        first = frames[0]
        if first.dtype not in (_U8, _U16):
            raise ValueError(f"{what} takes torch.uint8 or torch.uint16 DN frames, got {first.dtype}")
        if any(f.dtype != first.dtype or f.shape != first.shape or f.device != first.device for f in frames):
            raise ValueError(f"{what} needs DN frames of one dtype and one shape on one device")
        self.bit_depth = 8 if _welford_bit_depth(first.dtype, bit_depth) is None else int(bit_depth)
        if std_table is not None and icrf_diff is None:
            raise ValueError("std_table needs icrf_diff: the std of a DN is ICRF_diff * STD_table")
        dev = first.device
        Cc = first.shape[-1] if first.dim() > 0 else 1
        rows = 2 ** self.bit_depth
        self.tables = []
        for name, t in (("ICRF", icrf), ("ICRF_diff", icrf_diff), ("std_table", std_table)):
            t = None if t is None else _dev_f64(t, dev)
            if t is not None and tuple(t.shape) != (rows, Cc):
                raise ValueError(f"{name} must be shaped ({rows}, {Cc}), got {tuple(t.shape)}")
            self.tables.append(t)
        self.lo = self.hi = None
        if thresholds is not None:
            if len(thresholds[0]) != Cc or len(thresholds[1]) != Cc:
                raise ValueError("The length of 'lower' and 'upper' must match the size of the independent axis.")
            self.lo = (C.c_double * Cc)(*[float(x) for x in thresholds[0]])
            self.hi = (C.c_double * Cc)(*[float(x) for x in thresholds[1]])
        self.frames = [f.contiguous() for f in frames]
        self.n_pairs = P = len(pairs)
        self.channels = Cc
        self.weighted = std_table is not None
        self.variant = int(variant)
        self.device = dev
        self.host = dev.type != "cuda"
        self._fp = _ptr_array(self.frames)
        self._pi = (C.c_int32 * P)(*[int(p[0]) for p in pairs])
        self._pj = (C.c_int32 * P)(*[int(p[1]) for p in pairs])
        self._pm = (C.c_double * P)(*[float(p[2]) for p in pairs])


class PairsDnPlan(_PairsDnArgs):
    """One hm_pairs_statistics_dn call with everything it reads and writes: the DN frames, the tables, the pair arrays, the output and the
    workspace. launch() only enqueues (the table kernel, the statistics kernels, the final fold), so a PlanGraph can record it; the
    statistics are in `outputs["stats"]` (n_pairs * 6C float64) after the stream has run."""

    def __init__(self, frames: Sequence[torch.Tensor], pairs: Sequence[tuple], icrf, icrf_diff=None, std_table=None, thresholds=None,
                 bit_depth: Optional[int] = None, variant: int = 0):
        super().__init__("pairs_statistics_dn", frames, pairs, icrf, icrf_diff, std_table, thresholds, bit_depth, variant)
        P, Cc, dev = self.n_pairs, self.channels, self.device
        self.outputs = {"stats": torch.empty(P * 6 * Cc, dtype=_F64, device=dev)}
        self._ws = torch.empty(max(1, (nat.lib.hm_pairs_statistics_dn_workspace_bytes(P, Cc, self.bit_depth) + 7) // 8), dtype=_F64, device=dev)

    def launch(self, stream: Optional[int] = None) -> None:
        icrf, diff, table = self.tables
        with _on(self.device):
            nat.check(nat.lib.hm_pairs_statistics_dn(C.cast(self._fp, C.POINTER(C.c_void_p)), len(self.frames), self.bit_depth, icrf.data_ptr(),
                                                     nat.ptr(diff), nat.ptr(table), self._pi, self._pj, self._pm, self.n_pairs,
                                                     self.frames[0].numel(), self.channels, self.lo, self.hi, self.variant,
                                                     self.outputs["stats"].data_ptr(), self._ws.data_ptr(),
                                                     _stream(self.device) if stream is None else stream), "hm_pairs_statistics_dn")

    def kernels(self) -> str:
        aligned = all(f.data_ptr() % (2 if self.bit_depth == 8 else 4) == 0 for f in self.frames)
        return pairs_statistics_dn_kernel(self.frames[0].numel(), len(self.frames), self.n_pairs, self.channels, self.weighted, self.bit_depth,
                                          self.variant, aligned)


def pairs_statistics_dn(frames: Sequence[torch.Tensor], pairs: Sequence[tuple], icrf, icrf_diff=None, std_table=None, thresholds=None,
                        bit_depth: Optional[int] = None, to_host: bool = False, variant: int = 0):
    """pairs_statistics() straight from DN frames (hm_pairs_statistics_dn): torch.uint8 frames, or torch.uint16 frames with `bit_depth` in
    9..16. Element e of a frame, channel c, idx = DN & (2**bit_depth - 1) stands for the value icrf[idx, c] and - with `std_table`, the
    weighted statistics - the std icrf_diff[idx, c] * std_table[idx, c]; thresholds = (lower, upper) exclude a value outside its channel's
    limits together with its std (apply_thresholds). The tables are (2**bit_depth, C). The frames are not modified and no float64 frame
    is written. `variant`: 0 the library's choice, 1 the table in LDS, 2 gathered from global memory, -1 the per-wave kernel; the result
    does not depend on it. Returns what pairs_statistics returns."""
    plan = PairsDnPlan(frames, pairs, icrf, icrf_diff, std_table, thresholds, bit_depth, variant)
    plan.launch()
    out = plan.outputs["stats"]
    Cc, w = plan.channels, plan.weighted
    if to_host:
        out = out.cpu()                                   # one device-to-host copy for all pairs (P * 6C numbers)
    res = []
    for p in range(plan.n_pairs):
        b = p * 6 * Cc
        mk = lambda o: {"mean": out[o:o + Cc], "std": out[o + Cc:o + 2 * Cc], "error": out[o + 2 * Cc:o + 3 * Cc] if w else None}   # noqa: E731
        res.append((mk(b), mk(b + 3 * Cc)))
    return res


def pairs_statistics_dn_kernel(n_elems: int, n_frames: int, n_pairs: int, channels: int, with_std: bool, bit_depth: int, variant: int = 0,
                               frames_aligned: bool = True) -> str:
    """The statistics kernel of each launch of such a pairs_statistics_dn call, as hm_pairs_statistics_dn_describe names them (e.g.
    "pairs_stats_dn_lds<dn=u16,bits=12,tab=global,std=1,ni=1>"); nothing is launched. frames_aligned: every frame 2-byte (uint8) or
    4-byte (uint16) aligned. For tests and benchmarks."""
    buf = C.create_string_buffer(512)
    nat.check(nat.lib.hm_pairs_statistics_dn_describe(int(n_elems), int(n_frames), int(n_pairs), int(channels), int(bool(with_std)),
                                                      int(bit_depth), int(variant), int(bool(frames_aligned)), buf, len(buf)),
              "hm_pairs_statistics_dn_describe")
    return buf.value.decode()


def channel_minmax(val: torch.Tensor) -> np.ndarray:
    """(C, 2) host array: min and max of the finite values of each channel of a (..., C) float64 tensor (hm_channel_minmax; a channel
    without finite values gives (+inf, -inf)). One read-back of 2C doubles."""
    _require_cuda(val, "val")
    val = val.contiguous()
    Cc = val.shape[-1]
    ws = torch.empty(max(1, nat.lib.hm_histogram_workspace_bytes(1, Cc) // 8), dtype=_F64, device=val.device)
    mm = torch.empty(2 * Cc, dtype=_F64, device=val.device)
    with _on(val.device):
        nat.check(nat.lib.hm_channel_minmax(val.data_ptr(), None, val.numel(), Cc, mm.data_ptr(), ws.data_ptr(), _stream(val.device)),
                  "hm_channel_minmax")
        return mm.cpu().numpy().reshape(Cc, 2)


def channel_histogram(val: torch.Tensor, std: Optional[torch.Tensor], bins: int, included_range, channels: Sequence[int]):
    """modules/measurand.py:430-469 -> {c: (hist ndarray, bin_edges ndarray)} like np.histogram. A range of None is
    evaluated per channel from the counted values (np.histogram's default), with one extra reduction."""
    _require_cuda(val, "val")
    val = val.contiguous()
    std = None if std is None else std.contiguous()
    Cc = val.shape[-1]
    ws = torch.empty(max(1, nat.lib.hm_histogram_workspace_bytes(int(bins), Cc) // 8), dtype=_F64, device=val.device)
    out = {}
    with _on(val.device):
        if included_range is None:
            mm = torch.empty(2 * Cc, dtype=_F64, device=val.device)
            nat.check(nat.lib.hm_channel_minmax(val.data_ptr(), nat.ptr(std), val.numel(), Cc, mm.data_ptr(), ws.data_ptr(),
                                                _stream(val.device)), "hm_channel_minmax")
            mmh = mm.cpu().numpy().reshape(Cc, 2)
        groups = {}
        for c in channels:
            lo, hi = (float(mmh[c, 0]), float(mmh[c, 1])) if included_range is None else (float(included_range[0]), float(included_range[1]))
            if included_range is None and lo > hi:         # (+inf, -inf): nothing counted - np.histogram of an empty selection uses (0, 1)
                lo, hi = 0.0, 1.0
            if lo == hi:                                   # np.histogram widens an empty range by +-0.5
                lo, hi = lo - 0.5, hi + 0.5
            groups.setdefault((lo, hi), []).append(c)
        for (lo, hi), cs in groups.items():
            edges = np.linspace(lo, hi, int(bins) + 1)
            edges_d = torch.as_tensor(edges, device=val.device)
            res = torch.empty(Cc * int(bins), dtype=_F64, device=val.device)
            mask = sum(1 << c for c in cs)
            nat.check(nat.lib.hm_channel_histogram(val.data_ptr(), nat.ptr(std), val.numel(), Cc, mask, edges_d.data_ptr(), int(bins), lo, hi,
                                                   res.data_ptr(), ws.data_ptr(), _stream(val.device)), "hm_channel_histogram")
            r = res.cpu().numpy().reshape(Cc, int(bins))
            for c in cs:
                out[c] = (r[c] if std is not None else r[c].astype(np.int64), edges)
    return out


def _pairs_histogram_edges(minmax, included_range, P: int, Cc: int, bins: int, channels: Sequence[int], what: str) -> np.ndarray:
    """The (P, 2, C, bins + 1) bin edges of an all-pairs histogram call: np.linspace over `included_range`, or over np.histogram's default
    range per (pair, kind, channel) from minmax() - a device tensor of P * 2 * C * 2 min / max values, fetched with one host copy - with
    channel_histogram's two NumPy rules. Channels outside `channels` keep zero edges (they count nothing)."""
    if included_range is None:
        ranges = minmax().cpu().numpy().reshape(P, 2, Cc, 2).copy()        # one device-to-host copy for all pairs
        empty = ranges[..., 0] > ranges[..., 1]                            # (+inf, -inf): nothing counted - np.histogram of an empty selection uses (0, 1)
        ranges[empty] = (0.0, 1.0)
    else:
        ranges = np.empty((P, 2, Cc, 2))
        ranges[..., 0], ranges[..., 1] = float(included_range[0]), float(included_range[1])
    same = ranges[..., 0] == ranges[..., 1]                                # np.histogram widens an empty range by +-0.5
    ranges[same] += (-0.5, 0.5)
    if not np.all(ranges[:, :, channels, 1] > ranges[:, :, channels, 0]):
        raise ValueError(f"{what}: the upper end of the range must be above the lower end")
    edges = np.zeros((P, 2, Cc, bins + 1))
    for idx in np.ndindex(P, 2, Cc):
        if idx[2] in channels:
            edges[idx] = np.linspace(ranges[idx][0], ranges[idx][1], bins + 1)
    return edges


def pairs_histogram(vals: Sequence[torch.Tensor], stds: Optional[Sequence[torch.Tensor]], pairs: Sequence[tuple], bins: int, included_range,
                    channels: Sequence[int], thresholds: Optional[tuple] = None):
    """ExposurePair.compute_difference + process_linearity_distribution of EVERY exposure pair of a stack without the difference images
    (hm_pairs_histogram; `pairs` as in pairs_statistics). Returns one (abs_dict, rel_dict) per pair, each {c: (hist, bin_edges)} as
    channel_histogram() builds them: int64 counts without stds, float64 sums of 1 / std with them, edges np.linspace(lo, hi, bins + 1).
    included_range None: np.histogram's default range per (pair, kind, channel) from hm_pairs_minmax (one host copy), with channel_histogram's
    two NumPy rules. thresholds = (lower, upper): apply_thresholds on the values as read; the frames are NOT modified."""
    n, bins = len(vals), int(bins)
    for i, v in enumerate(vals):
        _require_cuda(v, f"vals[{i}]")
        if v.shape != vals[0].shape or v.dtype != _F64:
            raise ValueError("pairs_histogram needs float64 frames of one shape")
    if not 1 <= bins <= nat.HM_PAIRS_HIST_MAX_BINS:
        raise ValueError(f"pairs_histogram takes 1..{nat.HM_PAIRS_HIST_MAX_BINS} bins")
    dev = vals[0].device
    vals = [v.contiguous() for v in vals]
    if stds is not None:
        if len(stds) != n or any(s is None for s in stds):
            raise ValueError("one std frame per value frame (or none at all)")
        stds = [s.to(_F64).contiguous() for s in stds]
    Cc = vals[0].shape[-1]
    channels = [int(c) for c in channels]
    if any(c < 0 or c >= Cc for c in channels):
        raise ValueError("channel outside the frames' channels")
    lo = hi = None
    if thresholds is not None:
        if len(thresholds[0]) != Cc or len(thresholds[1]) != Cc:
            raise ValueError("The length of 'lower' and 'upper' must match the size of the independent axis.")
        lo = (C.c_double * Cc)(*[float(x) for x in thresholds[0]])
        hi = (C.c_double * Cc)(*[float(x) for x in thresholds[1]])
    P = len(pairs)
    vp = C.cast(_ptr_array(vals), C.POINTER(C.c_void_p))
    sp = None if stds is None else C.cast(_ptr_array(stds), C.POINTER(C.c_void_p))
    pi = (C.c_int32 * P)(*[int(p[0]) for p in pairs])
    pj = (C.c_int32 * P)(*[int(p[1]) for p in pairs])
    pm = (C.c_double * P)(*[float(p[2]) for p in pairs])
    ws = torch.empty(max(1, nat.lib.hm_pairs_histogram_workspace_bytes(P, bins, Cc) // 8), dtype=_F64, device=dev)
    with _on(dev):
        def minmax():
            mm = torch.empty(P * 2 * Cc * 2, dtype=_F64, device=dev)
            nat.check(nat.lib.hm_pairs_minmax(vp, sp, n, pi, pj, pm, P, vals[0].numel(), Cc, lo, hi, mm.data_ptr(), ws.data_ptr(), _stream(dev)),
                      "hm_pairs_minmax")
            return mm
        edges = _pairs_histogram_edges(minmax, included_range, P, Cc, bins, channels, "pairs_histogram")
        edges_d = torch.as_tensor(edges, device=dev)
        res = torch.empty(P * 2 * Cc * bins, dtype=_F64, device=dev)
        nat.check(nat.lib.hm_pairs_histogram(vp, sp, n, pi, pj, pm, P, vals[0].numel(), Cc, sum(1 << c for c in set(channels)), lo, hi,
                                             edges_d.data_ptr(), bins, res.data_ptr(), ws.data_ptr(), _stream(dev)), "hm_pairs_histogram")
        r = res.cpu().numpy().reshape(P, 2, Cc, bins)
    if stds is None:
        r = r.astype(np.int64)
    return [tuple({c: (r[p, k, c], edges[p, k, c]) for c in channels} for k in range(2)) for p in range(P)]


def pairs_histogram_dn(frames: Sequence[torch.Tensor], pairs: Sequence[tuple], icrf, icrf_diff=None, std_table=None, bins: int = 128,
                       included_range=None, channels: Optional[Sequence[int]] = None, thresholds: Optional[tuple] = None,
                       bit_depth: Optional[int] = None, variant: int = 0):
    """pairs_histogram() straight from DN frames (hm_pairs_minmax_dn, hm_pairs_histogram_dn): torch.uint8 frames, or torch.uint16 frames with
    `bit_depth` in 9..16, and (2**bit_depth, C) tables - the dtype and depth rules and the per-element semantics of pairs_statistics_dn
    (value icrf[idx, c], with `std_table` the std icrf_diff[idx, c] * std_table[idx, c] and weighted histograms, thresholds on the values
    as read). The frames are not modified and no float64 frame is written. channels None: every channel. Edges and result as
    pairs_histogram: included_range None takes every (pair, kind, channel)'s default range from one hm_pairs_minmax_dn pass first.
    `variant`: 0 the library's choice, 1 the table in LDS beside the histograms, 2 gathered from global memory; the counts do not depend
    on it."""
    plan = _PairsDnArgs("pairs_histogram_dn", frames, pairs, icrf, icrf_diff, std_table, thresholds, bit_depth, variant)
    bins = int(bins)
    if not 1 <= bins <= nat.HM_PAIRS_HIST_MAX_BINS:
        raise ValueError(f"pairs_histogram_dn takes 1..{nat.HM_PAIRS_HIST_MAX_BINS} bins")
    Cc, P, dev = plan.channels, plan.n_pairs, plan.device
    channels = list(range(Cc)) if channels is None else [int(c) for c in channels]
    if any(c < 0 or c >= Cc for c in channels):
        raise ValueError("channel outside the frames' channels")
    icrf_t, diff_t, table_t = plan.tables
    fp = C.cast(plan._fp, C.POINTER(C.c_void_p))
    n_frames, n = len(plan.frames), plan.frames[0].numel()
    ws = torch.empty(max(1, (nat.lib.hm_pairs_histogram_dn_workspace_bytes(P, bins, Cc, plan.bit_depth) + 7) // 8), dtype=_F64, device=dev)
    with _on(dev):
        def minmax():
            mm = torch.empty(P * 2 * Cc * 2, dtype=_F64, device=dev)
            nat.check(nat.lib.hm_pairs_minmax_dn(fp, n_frames, plan.bit_depth, icrf_t.data_ptr(), nat.ptr(diff_t), nat.ptr(table_t), plan._pi,
                                                 plan._pj, plan._pm, P, n, Cc, plan.lo, plan.hi, plan.variant, mm.data_ptr(), ws.data_ptr(),
                                                 _stream(dev)), "hm_pairs_minmax_dn")
            return mm
        edges = _pairs_histogram_edges(minmax, included_range, P, Cc, bins, channels, "pairs_histogram_dn")
        edges_d = torch.as_tensor(edges, device=dev)
        res = torch.empty(P * 2 * Cc * bins, dtype=_F64, device=dev)
        nat.check(nat.lib.hm_pairs_histogram_dn(fp, n_frames, plan.bit_depth, icrf_t.data_ptr(), nat.ptr(diff_t), nat.ptr(table_t), plan._pi,
                                                plan._pj, plan._pm, P, n, Cc, sum(1 << c for c in set(channels)), plan.lo, plan.hi,
                                                edges_d.data_ptr(), bins, plan.variant, res.data_ptr(), ws.data_ptr(), _stream(dev)),
                  "hm_pairs_histogram_dn")
        r = res.cpu().numpy().reshape(P, 2, Cc, bins)
    if not plan.weighted:
        r = r.astype(np.int64)
    return [tuple({c: (r[p, k, c], edges[p, k, c]) for c in channels} for k in range(2)) for p in range(P)]


def pairs_histogram_dn_kernel(n_elems: int, n_frames: int, n_pairs: int, channels: int, with_std: bool, bit_depth: int, bins: int,
                              variant: int = 0) -> str:
    """The histogram kernel of each launch of such a pairs_histogram_dn call, as hm_pairs_histogram_dn_describe names them (e.g.
    "pairs_hist_dn<dn=u16,bits=12,tab=global,std=1,np=8,wpp=2>"); nothing is launched. For tests and benchmarks."""
    buf = C.create_string_buffer(1024)
    nat.check(nat.lib.hm_pairs_histogram_dn_describe(int(n_elems), int(n_frames), int(n_pairs), int(channels), int(bool(with_std)),
                                                     int(bit_depth), int(bins), int(variant), buf, len(buf)),
              "hm_pairs_histogram_dn_describe")
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------
# weighted Gaussian kernel density estimates (modules/measurand.py:716-761)
# ------------------------------------------------------------------------------------------------
def kde_bandwidth(mom: np.ndarray):
    """(h, scale) of hm_kde_evaluate from one channel's hm_kde_moments, with the errors scipy.stats.gaussian_kde(values, 'silverman',
    weights) raises there (scipy 1.15): p = w / sum w, neff = 1 / sum p^2, factor = (0.75 neff)^(-1/5), var = np.cov(bias=False,
    aweights=p) = sum p (x - x_bar)^2 / (sum p - sum p^2 / sum p), h = sqrt(var) factor; scale = (2 pi)^(-1/2) / h / sum w.
    Constant data always raise LinAlgError (deviation M: scipy's weighted covariance sometimes rounds to a tiny positive value)."""
    count, sw, sw2, _, lo, hi, nonfinite, npos, nneg, _, m2 = (float(v) for v in mom[:nat.HM_KDE_MOMENTS])
    if count <= 1:
        raise ValueError("`dataset` input should have multiple elements.")
    if nonfinite:
        raise ValueError("array must not contain infs or NaNs")
    if npos and nneg:
        raise ValueError("weights of mixed sign")
    if sw == 0.0:
        raise ValueError("array must not contain infs or NaNs")
    if lo == hi:
        raise np.linalg.LinAlgError("1-th leading minor of the array is not positive definite")
    neff = 1.0 / (sw2 / (sw * sw))
    factor = np.power(neff * 3.0 / 4.0, -1.0 / 5)
    var = (m2 / sw) / (1.0 - sw2 / (sw * sw))
    if not (var > 0.0 and np.isfinite(var)):
        raise np.linalg.LinAlgError("1-th leading minor of the array is not positive definite")
    h = float(np.sqrt(var) * factor)
    return h, float(np.power(2 * np.pi, -0.5) / h / sw), (lo, hi)


def kernel_density_estimate(val: torch.Tensor, std: Optional[torch.Tensor], data_points: int, included_range, channels: Sequence[int]):
    """modules/measurand.py:716-761 -> {c: (estimate ndarray (data_points,), x_range ndarray)}: hm_kde_moments per channel, one read-back,
    the bandwidth and np.linspace grid on the host, hm_kde_evaluate per channel, one read-back."""
    _require_cuda(val, "val")
    val = val.contiguous()
    if val.dtype != _F64:
        raise TypeError("val must be float64")
    if std is not None:
        _require_cuda(std, "std")
        std = std.to(_F64).contiguous()
        if std.shape != val.shape:
            raise ValueError("Value and std shapes must match.")
    Cc = val.shape[-1] if val.dim() else 1
    n = val.numel()
    m = int(data_points)
    if m < 0:
        raise ValueError(f"Number of samples, {m}, must be non-negative.")
    channels = list(channels)
    for c in channels:
        if not -Cc <= c < Cc:
            raise IndexError(f"index {c} is out of bounds for axis with size {Cc}")
    dev = val.device
    wsb = nat.lib.hm_kde_workspace_bytes(n, Cc, m)
    ws = torch.empty(wsb, dtype=_U8, device=dev) if wsb else None
    wsp, wsn = nat.ptr(ws), int(wsb)
    mom = torch.empty((len(channels), nat.HM_KDE_MOMENTS), dtype=_F64, device=dev)
    with _on(dev):
        for k, c in enumerate(channels):
            nat.check(nat.lib.hm_kde_moments(val.data_ptr(), nat.ptr(std), n, Cc, c % Cc, mom[k].data_ptr(), wsp, wsn, _stream(dev)),
                      "hm_kde_moments")
        momh = mom.cpu().numpy()
        grids, params = [], []
        for k, c in enumerate(channels):
            h, scale, (lo, hi) = kde_bandwidth(momh[k])
            if included_range is not None:
                lo, hi = included_range[0], included_range[1]
            grids.append(np.linspace(lo, hi, num=m))
            params.append((h, scale))
        res = torch.zeros((len(channels), m), dtype=_F64, device=dev)
        if m:
            grid_d = torch.as_tensor(np.stack(grids), device=dev)
            for k, c in enumerate(channels):
                nat.check(nat.lib.hm_kde_evaluate(val.data_ptr(), nat.ptr(std), n, Cc, c % Cc, params[k][0], params[k][1], grid_d[k].data_ptr(),
                                                  m, res[k].data_ptr(), wsp, wsn, _stream(dev)), "hm_kde_evaluate")
        r = res.cpu().numpy()
    return {c: (r[k].copy(), grids[k]) for k, c in enumerate(channels)}


# ------------------------------------------------------------------------------------------------
# upstream producer: Welford mean / M2 over video frames (modules/video_processing.py:161-219)
# ------------------------------------------------------------------------------------------------
def _welford_bit_depth(dtype, bit_depth):
    """None for uint8 frames; the checked depth for torch.uint16 ones (which need one). A depth with any other dtype is refused."""
    if dtype == _U16:
        if bit_depth is None:
            raise ValueError("torch.uint16 frames need bit_depth (9..16): the camera's DN range")
        return _check_bit_depth(bit_depth)
    if bit_depth is not None:
        raise ValueError(f"bit_depth is for torch.uint16 frames, got {dtype}")
    return None


def welford_update(frames: Sequence[torch.Tensor], count_before: int, mean: torch.Tensor, m2: Optional[torch.Tensor],
                   icrf=None, bit_depth: Optional[int] = None, variant: int = 0) -> int:
    """Fold `frames` (uint8 (H, W, C) device tensors, in order) into the running float64 mean / m2 in place
    (video_processing.py:199-208). Returns the new frame count. Frames are folded HM_MAX_FRAMES per launch.
    torch.uint16 frames need `bit_depth` in 9..16 (hm_welford_update_u16): an ICRF of 2**bit_depth rows, a DN's index
    DN & (2**bit_depth - 1), DN / (2**bit_depth - 1) without an ICRF. `variant` says where the device kernel takes a frame value from
    (0: the library's choice, 1: a table in LDS, 2: computed, without an ICRF only, 3: the ICRF in global memory); the result does not
    depend on it."""
    _require_cuda(mean, "mean")
    if mean.dtype != _F64 or not mean.is_contiguous():
        raise TypeError("mean must be a contiguous float64 tensor")
    if m2 is not None and (m2.dtype != _F64 or not m2.is_contiguous() or m2.shape != mean.shape):
        raise TypeError("m2 must be a contiguous float64 tensor shaped like mean")
    dev = mean.device
    Cc = mean.shape[-1]
    frames = list(frames)
    first = frames[0].dtype if frames and isinstance(frames[0], torch.Tensor) else _U16 if bit_depth is not None else _U8
    bit_depth = _welford_bit_depth(first, bit_depth)
    rows, dn_dtype = (BITS, _U8) if bit_depth is None else (2 ** bit_depth, _U16)
    lut = None if icrf is None else _dev_f64(icrf, dev)
    if lut is not None and tuple(lut.shape) != (rows, Cc):
        raise ValueError(f"ICRF must be shaped ({rows}, {Cc})")
    count = int(count_before)
    for f in frames:
        _require_cuda(f, "frame")
        if f.dtype != dn_dtype or f.shape != mean.shape:
            raise ValueError(f"every frame must be a {str(dn_dtype).replace('torch.', '')} tensor shaped like mean")
    with _on(dev):
        for k0 in range(0, len(frames), nat.HM_MAX_FRAMES):
            batch = [f.contiguous() for f in frames[k0:k0 + nat.HM_MAX_FRAMES]]
            head = (_ptr_array(batch), len(batch), count, nat.ptr(lut), mean.data_ptr(), nat.ptr(m2), mean.numel(), Cc)
            if bit_depth is None:
                nat.check(nat.lib.hm_welford_update(*head, _stream(dev)), "hm_welford_update")
            else:
                nat.check(nat.lib.hm_welford_update_u16(*head, bit_depth, int(variant), _stream(dev)), "hm_welford_update_u16")
            count += len(batch)
    return count


def welford_finalize(mean: torch.Tensor, m2: Optional[torch.Tensor], count: int, bit_depth: Optional[int] = None):
    """-> (mean frame uint8, std frame uint8 or None), video_processing.py:210-215. With `bit_depth` (9..16) the frames are torch.uint16
    and the mean is scaled by 2**bit_depth - 1 (hm_welford_finalize_u16)."""
    _require_cuda(mean, "mean")
    if bit_depth is not None:
        bit_depth = _check_bit_depth(bit_depth)
    dtype = _U8 if bit_depth is None else _U16
    out_mean = torch.empty(mean.shape, dtype=dtype, device=mean.device)
    out_std = None if m2 is None else torch.empty(mean.shape, dtype=dtype, device=mean.device)
    with _on(mean.device):
        if bit_depth is None:
            nat.check(nat.lib.hm_welford_finalize(mean.data_ptr(), nat.ptr(m2), int(count), out_mean.data_ptr(), nat.ptr(out_std),
                                                  mean.numel(), _stream(mean.device)), "hm_welford_finalize")
        else:
            nat.check(nat.lib.hm_welford_finalize_u16(mean.data_ptr(), nat.ptr(m2), int(count), bit_depth, out_mean.data_ptr(), nat.ptr(out_std),
                                                      mean.numel(), _stream(mean.device)), "hm_welford_finalize_u16")
    return out_mean, out_std


def welford_kernel(n_elems: int, n_frames: int, channels: int, with_icrf: bool, with_m2: bool, bit_depth: int, variant: int = 0) -> str:
    """The kernel welford_update(..., bit_depth=bit_depth, variant=variant) starts on such a call, as hm_welford_update_u16_describe names
    it (e.g. "k_welford_u16<m2=1,tab=lds,bits=12>"); nothing is launched. For tests and benchmarks."""
    buf = C.create_string_buffer(128)
    nat.check(nat.lib.hm_welford_update_u16_describe(int(n_elems), int(n_frames), int(channels), int(bool(with_icrf)), int(bool(with_m2)),
                                                     int(bit_depth), int(variant), buf, len(buf)), "hm_welford_update_u16_describe")
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------
# camera noise profiles and the per-DN STD table (modules/video_processing.py:12-133)
# ------------------------------------------------------------------------------------------------
_I64 = torch.int64


def _check_profiles(profiles: torch.Tensor) -> int:
    _require_cuda(profiles, "profiles")
    if profiles.dtype != _I64 or not profiles.is_contiguous():
        raise TypeError("profiles must be a contiguous int64 tensor")
    if profiles.dim() != 3 or tuple(profiles.shape[:2]) != (BITS, BITS):
        raise ValueError(f"profiles must be shaped ({BITS}, {BITS}, C)")
    return profiles.shape[2]


def noise_profile_update(frames: Sequence[torch.Tensor], mean_u8: torch.Tensor, profiles: torch.Tensor) -> None:
    """Add every element of `frames` (uint8 (H, W, C) tensors) to profiles[mean DN, frame DN, c] in place (video_processing.py:
    93-104). `profiles` ((256, 256, C) int64) is zeroed by the caller before the first update. HM_MAX_FRAMES frames per launch."""
    Cc = _check_profiles(profiles)
    _require_cuda(mean_u8, "mean_frame")
    if mean_u8.dtype != _U8 or not mean_u8.is_contiguous():
        raise TypeError("mean_frame must be a contiguous uint8 tensor")
    if mean_u8.shape[-1] != Cc:
        raise ValueError(f"mean_frame has {mean_u8.shape[-1]} channels, profiles {Cc}")
    frames = list(frames)
    for f in frames:
        _require_cuda(f, "frame")
        if f.dtype != _U8 or f.shape != mean_u8.shape:
            raise ValueError("every frame must be a uint8 tensor shaped like mean_frame")
    dev = profiles.device
    n = mean_u8.numel()
    wsb = nat.lib.hm_noise_profile_workspace_bytes(n, Cc)
    ws = torch.empty(max(1, wsb), dtype=_U8, device=dev) if wsb else None
    with _on(dev):
        for k0 in range(0, len(frames), nat.HM_MAX_FRAMES):
            batch = [f.contiguous() for f in frames[k0:k0 + nat.HM_MAX_FRAMES]]
            nat.check(nat.lib.hm_noise_profile_update(_ptr_array(batch), len(batch), mean_u8.data_ptr(), n, Cc, profiles.data_ptr(),
                                                      nat.ptr(ws), wsb, _stream(dev)), "hm_noise_profile_update")


def noise_profile_std(profiles: torch.Tensor) -> torch.Tensor:
    """-> (256, C) float64: _calculate_STD (video_processing.py:109-133) of every channel; NaN for a level without counts."""
    Cc = _check_profiles(profiles)
    dev = profiles.device
    edges = torch.as_tensor(np.linspace(0, 1, num=BITS, dtype=float), device=dev)          # :120, bit-identical by construction
    out = torch.empty((BITS, Cc), dtype=_F64, device=dev)
    with _on(dev):
        nat.check(nat.lib.hm_noise_profile_std(profiles.data_ptr(), Cc, edges.data_ptr(), out.data_ptr(), _stream(dev)),
                  "hm_noise_profile_std")
    return out


def noise_profile_clean_edges(profiles: torch.Tensor) -> torch.Tensor:
    """clean_data_edges (video_processing.py:12-74) of every channel's (256, 256) distributions, in place; returns `profiles`."""
    Cc = _check_profiles(profiles)
    dev = profiles.device
    with _on(dev):
        nat.check(nat.lib.hm_noise_profile_clean_edges(profiles.data_ptr(), Cc, _stream(dev)), "hm_noise_profile_clean_edges")
    return profiles


def _check_moments(moments: torch.Tensor, bit_depth) -> tuple:
    """-> (bit_depth, C) of a (2**bit_depth, C, 3) int64 noise-moments tensor"""
    bit_depth = _check_bit_depth(bit_depth)
    _require_cuda(moments, "moments")
    if moments.dtype != _I64 or not moments.is_contiguous():
        raise TypeError("moments must be a contiguous int64 tensor")
    if moments.dim() != 3 or moments.shape[0] != 2 ** bit_depth or moments.shape[2] != 3:
        raise ValueError(f"moments must be shaped ({2 ** bit_depth}, C, 3) at bit_depth {bit_depth}, got {tuple(moments.shape)}")
    return bit_depth, moments.shape[1]


def noise_moments_update(frames: Sequence[torch.Tensor], mean_u16: torch.Tensor, moments: torch.Tensor, bit_depth: int,
                         variant: Optional[int] = None) -> None:
    """Add every element of `frames` (torch.uint16 (H, W, C) tensors of a `bit_depth`-bit camera, 9..16) to the noise moments of its mean
    level in place (hm_noise_moments_update_u16): with m = mean DN & M, f = frame DN & M and d = f - m, moments[m, c] += (1, d, d * d).
    `moments` ((2**bit_depth, C, 3) int64) is zeroed by the caller before the first update. HM_MAX_FRAMES frames per launch. `variant` says
    where the device kernel keeps a launch's sums (None or 0: the library's choice, 1: the whole table in LDS, 2: global atomics, 3: a
    hashed window in LDS); the result does not depend on it."""
    bit_depth, Cc = _check_moments(moments, bit_depth)
    _require_cuda(mean_u16, "mean_frame")
    if mean_u16.dtype != _U16:
        raise ValueError(f"bit_depth is for a torch.uint16 mean_frame, got {mean_u16.dtype}")
    if not mean_u16.is_contiguous():
        raise TypeError("mean_frame must be a contiguous uint16 tensor")
    if mean_u16.dim() < 1 or mean_u16.shape[-1] != Cc:
        raise ValueError(f"mean_frame has {mean_u16.shape[-1] if mean_u16.dim() else 0} channels, moments {Cc}")
    frames = list(frames)
    for f in frames:
        _require_cuda(f, "frame")
        if f.dtype != _U16:
            raise ValueError(f"bit_depth is for torch.uint16 frames, got {f.dtype}")
        if f.shape != mean_u16.shape:
            raise ValueError("every frame must be a uint16 tensor shaped like mean_frame")
    dev = moments.device
    n = mean_u16.numel()
    variant = 0 if variant is None else int(variant)
    with _on(dev):
        for k0 in range(0, len(frames), nat.HM_MAX_FRAMES):
            batch = [f.contiguous() for f in frames[k0:k0 + nat.HM_MAX_FRAMES]]
            nat.check(nat.lib.hm_noise_moments_update_u16(_ptr_array(batch), len(batch), mean_u16.data_ptr(), n, Cc, bit_depth,
                                                          moments.data_ptr(), variant, _stream(dev)), "hm_noise_moments_update_u16")


def noise_moments_std(moments: torch.Tensor, bit_depth: int) -> torch.Tensor:
    """-> (2**bit_depth, C) float64 per-DN STD table on the DN grid k / (2**bit_depth - 1): sqrt(n S2 - S1^2) / n / M per level and channel
    (hm_noise_moments_std), _calculate_STD's quantity; NaN for a level without counts."""
    bit_depth, Cc = _check_moments(moments, bit_depth)
    dev = moments.device
    out = torch.empty((2 ** bit_depth, Cc), dtype=_F64, device=dev)
    with _on(dev):
        nat.check(nat.lib.hm_noise_moments_std(moments.data_ptr(), Cc, bit_depth, out.data_ptr(), _stream(dev)), "hm_noise_moments_std")
    return out


def noise_moments_kernel(n_elems: int, n_frames: int, channels: int, bit_depth: int, variant: int = 0) -> str:
    """The kernel noise_moments_update starts on such a call, as hm_noise_moments_update_u16_describe names it
    (e.g. "k_noise_moments_u16<C=3,tab=lds,bits=11>"); nothing is launched. For tests and benchmarks."""
    buf = C.create_string_buffer(128)
    nat.check(nat.lib.hm_noise_moments_update_u16_describe(int(n_elems), int(n_frames), int(channels), int(bit_depth), int(variant), buf, len(buf)),
              "hm_noise_moments_update_u16_describe")
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------
# ICRF-calibration energy function (modules/ICRF_calibration_exposure.py:66-201), batched over candidates
# ------------------------------------------------------------------------------------------------
def _check_stacks(dn_stacks: Sequence[torch.Tensor], std_stacks: Optional[Sequence[Optional[torch.Tensor]]], exposures, batch: bool = False,
                  dn_dtype=_U8):
    """The uint8 (X, Y, N) stacks of a calibration - one, or those of a batch: one shape, one device -, their float64 std stacks (None,
    or a sequence whose entries are all None: no stds) and the N exposures, checked in this order
    -> (contiguous stacks, contiguous std stacks | None, exposures as a float64 array). `batch` words the std messages for a batch, whose
    std stacks must also live on the stacks' device. `dn_dtype`: torch.uint16 for a stack with a bit depth (linearity_energy(..., bit_depth=)
    DEPlanU16 and DEBatchPlanU16; DEPlan and DEBatchPlan take uint8 stacks only)."""
    first = dn_stacks[0]
    for s in dn_stacks:
        _require_cuda(s, "image_value_stack")
        if s.dtype != dn_dtype:
            raise TypeError("image_value_stack must be uint8 digital numbers")
        if s.dim() != 3:
            raise ValueError("image_stack must be a 3D array with shape (X, Y, N).")             # ICRF_calibration_exposure.py:82-83
        if s.shape != first.shape:
            raise ValueError(f"the stacks of a batch must have one shape: {tuple(s.shape)} != {tuple(first.shape)}")
        if s.device != first.device:
            raise ValueError(f"the stacks of a batch must live on one device: {s.device} != {first.device}")
    t = np.asarray(exposures, dtype=np.float64)
    if t.ndim != 1 or t.size != first.shape[2]:
        raise ValueError("exposure_values must be a 1D array matching the third dimension of image_stack.")   # :85-86
    if std_stacks is None or all(s is None for s in std_stacks):
        return [s.contiguous() for s in dn_stacks], None, t
    std_stacks = list(std_stacks)
    if len(std_stacks) != len(dn_stacks) or any(s is None for s in std_stacks):
        raise ValueError("image_std_stacks must be given for every stack of a batch or for none")
    for s in std_stacks:
        _require_cuda(s, "image_std_stack")
        if s.shape != first.shape or s.dtype != _F64 or (batch and s.device != first.device):
            raise ValueError("image_std_stack must be float64, shaped like image_value_stack and on its device" if batch else
                             "image_std_stack must be float64 and shaped like image_value_stack")
    return [s.contiguous() for s in dn_stacks], [s.contiguous() for s in std_stacks], t


def _energy_bit_depth(dn_stack, bit_depth) -> Optional[int]:
    """The depth of an energy call's stack: None for uint8 DNs, `bit_depth` in 9..16 for torch.uint16 ones. Any other dtype is left to
    _check_stacks' TypeError unless it comes with a bit_depth, which only uint16 stacks take."""
    if isinstance(dn_stack, torch.Tensor) and dn_stack.dtype == _U16:
        if bit_depth is None:
            raise ValueError("a torch.uint16 image_value_stack needs bit_depth (9..16): the number of rows of its candidate ICRFs")
        return _check_bit_depth(bit_depth)
    if bit_depth is not None:
        raise ValueError(f"bit_depth is for torch.uint16 DN stacks, got {getattr(dn_stack, 'dtype', type(dn_stack))}")
    return None


def linearity_energy(dn_stack: torch.Tensor, std_stack: Optional[torch.Tensor], exposures: Sequence[float], icrf_batch,
                     lower: int, upper: int, valid=None, use_relative: bool = True, return_pairs: bool = False,
                     bit_depth: Optional[int] = None, variant: int = 0):
    """Energy of every candidate ICRF row of `icrf_batch` ((B, 256) float64) on one channel's (X, Y, N) uint8 stack.
    -> energies (B,) float64 device tensor [, pair results (B, N(N-1)/2)].
    torch.uint16 stacks need `bit_depth` in 9..16 (hm_linearity_energy_u16): candidates of 2**bit_depth entries, a DN's index
    DN & (2**bit_depth - 1), `lower` / `upper` DNs of that depth. `variant` places the candidate's row on the device (0: the library's
    choice, 1: LDS, up to 14 bits, 2: global memory); the result does not depend on it."""
    bit_depth = _energy_bit_depth(dn_stack, bit_depth)
    (dn_stack,), sd, t = _check_stacks([dn_stack], [std_stack], exposures, dn_dtype=_U8 if bit_depth is None else _U16)
    std_stack = None if sd is None else sd[0]
    dev = dn_stack.device
    N = dn_stack.shape[2]
    n_rows = BITS if bit_depth is None else 2 ** bit_depth
    lut = _dev_f64(icrf_batch, dev)
    if lut.dim() == 1:
        lut = lut[None]
    if lut.shape[1] != n_rows:
        raise ValueError(f"candidate ICRFs must have {n_rows} entries")
    if bit_depth is not None and not (0 <= int(lower) < n_rows and 0 <= int(upper) < n_rows):
        raise ValueError(f"lower and upper must be DNs in 0..{n_rows - 1} at bit_depth {bit_depth}, got {lower}, {upper}")
    lut = lut.contiguous()
    B = lut.shape[0]
    vd = None if valid is None else torch.as_tensor(np.asarray(valid, dtype=np.uint8), device=dev)
    P = dn_stack.shape[0] * dn_stack.shape[1]
    pairs = N * (N - 1) // 2
    energy = torch.empty(B, dtype=_F64, device=dev)
    out_pairs = torch.empty((B, pairs), dtype=_F64, device=dev) if return_pairs else None
    ws = torch.empty(max(1, nat.lib.hm_linearity_energy_workspace_bytes(P, N, B) // 8), dtype=_F64, device=dev)
    head = (dn_stack.data_ptr(), nat.ptr(std_stack), (C.c_double * N)(*t.tolist()), lut.data_ptr(), nat.ptr(vd), B, int(lower), int(upper),
            int(bool(use_relative)), P, N)
    tail = (nat.ptr(out_pairs), energy.data_ptr(), ws.data_ptr(), _stream(dev))
    with _on(dev):
        if bit_depth is None:
            nat.check(nat.lib.hm_linearity_energy(*head, *tail), "hm_linearity_energy")
        else:
            nat.check(nat.lib.hm_linearity_energy_u16(*head, bit_depth, int(variant), *tail), "hm_linearity_energy_u16")
    return (energy, out_pairs) if return_pairs else energy


def energy_kernel(n_pixels: int, n_frames: int, n_candidates: int, with_std: bool, bit_depth: int, variant: int = 0) -> str:
    """The kernel linearity_energy(..., bit_depth=bit_depth, variant=variant) starts on such a problem, as hm_linearity_energy_u16_describe
    names it (e.g. "k_energy_pixel_u16<N=7,std=1,lut=lds,bits=12>"); nothing is launched. For tests and benchmarks."""
    buf = C.create_string_buffer(128)
    nat.check(nat.lib.hm_linearity_energy_u16_describe(int(n_pixels), int(n_frames), int(n_candidates), int(bool(with_std)), int(bit_depth),
                                                       int(variant), buf, len(buf)), "hm_linearity_energy_u16_describe")
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------
# ICRF-calibration differential evolution (modules/ICRF_calibration_exposure.py:288-369), one generation per hm_de_generation call
# ------------------------------------------------------------------------------------------------
def _status_dict(w: np.ndarray) -> dict:
    f = w.view(np.float64)
    return dict(generation=int(w[nat.HM_DE_GENERATION]) - 1, best_index=int(w[nat.HM_DE_BEST_INDEX]), stop=int(w[nat.HM_DE_STOP]),
                evaluations=int(w[nat.HM_DE_EVALUATIONS]), best_energy=float(f[nat.HM_DE_BEST_ENERGY]),
                mean=float(f[nat.HM_DE_MEAN]), std=float(f[nat.HM_DE_STD]))


class _DEPlanBase:
    """What DEPlan, DEPlanU16, DEBatchPlan and DEBatchPlanU16 share: one native call per generation, `check_every` of them recorded as one
    linear chain and replayed until the plan has stopped. A subclass sets `device` and `host` (through `_init_one` or `_init_batch`),
    names its entry point (`_entry`) and supplies `_call(stream)` (the native call -> status code), `read_status()` and
    `_stopped(status)`."""
    _entry = ""
    _graph = None
    _graph_len = 0

    def launch(self, stream: Optional[int] = None) -> None:
        """Enqueue one generation - of every problem, for a batch - on `stream` (default: the current stream of the plan's device)."""
        if self.host:
            with nat.host_mode():
                nat.check(self._call(None), self._entry)
            return
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        with _on(self.device):
            rc = self._call(stream)
        if rc:
            nat.check(rc, self._entry)

    def _record(self, n: int) -> None:
        """Record n generations as one linear chain (warm-up launch outside the capture: it is a real generation, the first of the run)."""
        dev = self.device
        with torch.cuda.device(dev):
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                self.launch(side.cuda_stream)           # first launches load the kernels' code objects: outside the capture
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph, stream=side):
                    for _ in range(n):
                        self.launch(side.cuda_stream)
            torch.cuda.current_stream(dev).wait_stream(side)
        self._graph_len = n

    def run(self, check_every: int = 8, graph: bool = True):
        """Advance until the stop flag is set - EVERY problem's, for a batch: `check_every` generations per status read.
        -> the final read_status()."""
        check_every = int(check_every)
        if check_every < 1:
            raise ValueError("check_every must be >= 1")
        use_graph = graph and not self.host
        if use_graph and self._graph_len != check_every:
            self._record(check_every)                   # (runs generation 0 as its warm-up launch)
        while True:
            if use_graph:
                with _on(self.device):
                    self._graph.replay()
            else:
                for _ in range(check_every):
                    self.launch()
            st = self.read_status()
            if self._stopped(st):
                return st

    def _init_one(self, dn_stack, std_stack, exposures, mean_icrf, pca, lower_limits, upper_limits, population, lower, upper, seed,
                  max_generations, mutation, recombination, tol, energy_limit, n_rows, dn_dtype):
        """The state of ONE problem on a stack of `dn_dtype` DNs with candidate rows of `n_rows` entries (DEPlan: uint8, 256; DEPlanU16:
        uint16, 2**bit_depth)."""
        (self.dn,), sd, t = _check_stacks([dn_stack], [std_stack], exposures, dn_dtype=dn_dtype)
        self.std = None if sd is None else sd[0]
        dev = dn_stack.device
        self.device = dev
        self.host = dev.type != "cuda"
        N = dn_stack.shape[2]
        pop = np.ascontiguousarray(np.asarray(population, dtype=np.float64))
        if pop.ndim != 2:
            raise ValueError("population must be (S, P) in scaled coordinates [0, 1]")
        S, P = pop.shape
        self.S, self.P, self.N = S, P, N
        self.n_pixels = dn_stack.shape[0] * dn_stack.shape[1]
        self.mean_icrf = _dev_f64(np.asarray(mean_icrf, dtype=np.float64).reshape(-1), dev)
        self.pca = _dev_f64(np.asarray(pca, dtype=np.float64), dev)
        if self.mean_icrf.numel() != n_rows or tuple(self.pca.shape) != (n_rows, P):
            raise ValueError(f"mean ICRF must have {n_rows} entries and the PCA basis must be ({n_rows}, {P})")
        self.lo = _dev_f64(np.broadcast_to(np.asarray(lower_limits, dtype=np.float64), (P,)).copy(), dev)
        self.hi = _dev_f64(np.broadcast_to(np.asarray(upper_limits, dtype=np.float64), (P,)).copy(), dev)
        self.population = torch.as_tensor(pop, device=dev).clone()
        self.energies = torch.full((S,), float("inf"), dtype=_F64, device=dev)
        self.trial = torch.zeros((S, P), dtype=_F64, device=dev)
        self.trial_energies = torch.full((S,), float("inf"), dtype=_F64, device=dev)
        self.icrf = torch.zeros((S, n_rows), dtype=_F64, device=dev)
        self.valid = torch.zeros(S, dtype=_U8, device=dev)
        self.status = torch.zeros(nat.HM_DE_STATUS_WORDS, dtype=torch.int64, device=dev)
        self._t = (C.c_double * N)(*t.tolist())
        self._scalars = (int(lower), int(upper), int(S), int(P), C.c_int64(int(seed) & 0xFFFFFFFFFFFFFFFF).value,
                         int(max_generations), float(mutation[0]), float(mutation[1]), float(recombination), float(tol),
                         float(energy_limit))
        with nat.host_mode() if self.host else _NoDevice():
            ws_bytes = nat.lib.hm_de_workspace_bytes(self.n_pixels, N, S)
        self.workspace = torch.empty(max(1, ws_bytes // 8), dtype=_F64, device=dev)

    def _init_batch(self, dn_stacks, std_stacks, exposures, mean_icrfs, pcas, lower_limits, upper_limits, populations, lower, upper, seeds,
                    max_generations, mutation, recombination, tol, energy_limit, stack_of, n_rows, dn_dtype):
        """The state of K problems of one shape on stacks of `dn_dtype` DNs with candidate rows of `n_rows` entries (DEBatchPlan: uint8,
        256; DEBatchPlanU16: uint16, 2**bit_depth), the problem outermost in every state tensor."""
        dn_stacks = list(dn_stacks)
        if not dn_stacks:
            raise ValueError("dn_stacks must hold at least one stack")
        self.dn, self.std, t = _check_stacks(dn_stacks, std_stacks, exposures, batch=True, dn_dtype=dn_dtype)
        dev = dn_stacks[0].device
        self.device = dev
        self.host = dev.type != "cuda"
        N = dn_stacks[0].shape[2]
        pop = np.ascontiguousarray(np.asarray(populations, dtype=np.float64))
        if pop.ndim != 3:
            raise ValueError("populations must be (K, S, P) in scaled coordinates [0, 1]")
        K, S, P = pop.shape
        if K < 1 or K > nat.HM_DE_MAX_PROBLEMS:
            raise ValueError(f"a batch holds 1 to {nat.HM_DE_MAX_PROBLEMS} problems, got {K}")
        if stack_of is None:
            if len(dn_stacks) != K:
                raise ValueError(f"{len(dn_stacks)} stacks for {K} problems: give stack_of, the stack index of every problem")
            stack_of = range(K)
        stack_of = [int(i) for i in stack_of]
        if len(stack_of) != K or any(i < 0 or i >= len(dn_stacks) for i in stack_of):
            raise ValueError(f"stack_of must hold {K} indices into the {len(dn_stacks)} stacks, got {stack_of}")
        seeds = [int(s) for s in seeds]
        if len(seeds) != K or len(mean_icrfs) != K or len(pcas) != K:
            raise ValueError(f"seeds, mean_icrfs and pcas must hold one entry per problem ({K})")
        self.K, self.S, self.P, self.N = K, S, P, N
        self.stack_of = stack_of
        self.n_pixels = dn_stacks[0].shape[0] * dn_stacks[0].shape[1]
        means = [np.asarray(m, dtype=np.float64).reshape(-1) for m in mean_icrfs]
        bases = [np.asarray(b, dtype=np.float64) for b in pcas]
        if any(m.size != n_rows for m in means) or any(b.shape != (n_rows, P) for b in bases):
            raise ValueError(f"every mean ICRF must have {n_rows} entries and every PCA basis must be ({n_rows}, {P})")
        self.mean_icrf = _dev_f64(np.stack(means), dev)
        self.pca = _dev_f64(np.stack(bases), dev)
        self.lo = _dev_f64(np.broadcast_to(np.asarray(lower_limits, dtype=np.float64), (P,)).copy(), dev)
        self.hi = _dev_f64(np.broadcast_to(np.asarray(upper_limits, dtype=np.float64), (P,)).copy(), dev)
        self.population = torch.as_tensor(pop, device=dev).clone()
        self.energies = torch.full((K, S), float("inf"), dtype=_F64, device=dev)
        self.trial = torch.zeros((K, S, P), dtype=_F64, device=dev)
        self.trial_energies = torch.full((K, S), float("inf"), dtype=_F64, device=dev)
        self.icrf = torch.zeros((K, S, n_rows), dtype=_F64, device=dev)
        self.valid = torch.zeros((K, S), dtype=_U8, device=dev)
        self.status = torch.zeros((K, nat.HM_DE_STATUS_WORDS), dtype=torch.int64, device=dev)
        self._t = (C.c_double * N)(*t.tolist())
        self._dn = _ptr_array([self.dn[i] for i in stack_of])
        self._sd = None if self.std is None else _ptr_array([self.std[i] for i in stack_of])
        self._seeds = (C.c_int64 * K)(*[C.c_int64(s & 0xFFFFFFFFFFFFFFFF).value for s in seeds])
        self._scalars = (int(lower), int(upper), int(S), int(P), int(max_generations), float(mutation[0]), float(mutation[1]),
                         float(recombination), float(tol), float(energy_limit))
        with nat.host_mode() if self.host else _NoDevice():
            ws_bytes = nat.lib.hm_de_batch_workspace_bytes(self.n_pixels, N, S, K)
        self.workspace = torch.empty(max(1, ws_bytes // 8), dtype=_F64, device=dev)

    def _batch_head(self):
        """The leading arguments that hm_de_generation_batch and hm_de_generation_u16_batch share, up to energy_limit."""
        lower, upper, S, P, max_gen, m_lo, m_hi, cr, tol, e_lim = self._scalars
        return (self.K, self.population.data_ptr(), self.energies.data_ptr(), self.trial.data_ptr(), self.trial_energies.data_ptr(),
                self.icrf.data_ptr(), self.valid.data_ptr(), self.status.data_ptr(), self.mean_icrf.data_ptr(), self.pca.data_ptr(),
                self.lo.data_ptr(), self.hi.data_ptr(), self._dn, self._sd, self._seeds, self._t, self.n_pixels, self.N, lower, upper, S, P,
                max_gen, m_lo, m_hi, cr, tol, e_lim)


class DEPlan(_DEPlanBase):
    """The state of one channel's differential-evolution solve (population, energies, trial rows, candidate ICRFs, verdicts, status block,
    workspace - all on the stack's device) and the launches that advance it. `launch()` enqueues ONE generation (hm_de_generation: trial
    kernel, the energy kernels, select kernel); the generation counter and the stop flag live in the status block on the device, so
    `run()` records `check_every` generations once into a hipGraph - a linear chain, no parallel branches - and replays it, reading
    the status block back once per replay. `graph=False` issues the same calls eagerly. After the stop flag is set a generation is a
    no-op, so the result does not depend on `check_every`. Built inside nat.host_mode() on a host stack, it calls the host build in a
    loop (no graph)."""
    _entry = "hm_de_generation"

    def __init__(self, dn_stack: torch.Tensor, std_stack: Optional[torch.Tensor], exposures: Sequence[float], mean_icrf, pca,
                 lower_limits, upper_limits, population, lower: int, upper: int, seed: int, max_generations: int,
                 mutation=(0.0, 1.95), recombination: float = 0.4, tol: float = 0.01, energy_limit: float = 0.0):
        self._init_one(dn_stack, std_stack, exposures, mean_icrf, pca, lower_limits, upper_limits, population, lower, upper, seed,
                       max_generations, mutation, recombination, tol, energy_limit, BITS, _U8)

    def _call(self, stream):
        lower, upper, S, P, seed, max_gen, m_lo, m_hi, cr, tol, e_lim = self._scalars
        return nat.lib.hm_de_generation(self.population.data_ptr(), self.energies.data_ptr(), self.trial.data_ptr(),
                                        self.trial_energies.data_ptr(), self.icrf.data_ptr(), self.valid.data_ptr(),
                                        self.status.data_ptr(), self.mean_icrf.data_ptr(), self.pca.data_ptr(), self.lo.data_ptr(),
                                        self.hi.data_ptr(), self.dn.data_ptr(), nat.ptr(self.std), self._t, self.n_pixels, self.N,
                                        lower, upper, S, P, seed, max_gen, m_lo, m_hi, cr, tol, e_lim, self.workspace.data_ptr(), stream)

    def read_status(self) -> dict:
        """The status block, copied to the host (this synchronises): generation = the number of generations after the initial
        evaluation that have run."""
        return _status_dict(self.status.cpu().numpy())

    def _stopped(self, status: dict) -> bool:
        return bool(status["stop"])


class DEPlanU16(_DEPlanBase):
    """DEPlan for one channel of a 9- to 16-bit camera: a torch.uint16 (X, Y, N) stack with its `bit_depth`, a mean ICRF of 2**bit_depth
    entries and a PCA basis of (2**bit_depth, P); `lower` / `upper` are DNs of that depth. The state tensors are DEPlan's, `icrf` of shape
    (S, 2**bit_depth). `launch()` enqueues ONE generation (hm_de_generation_u16: the trial kernel on rows of 2**bit_depth entries,
    hm_linearity_energy_u16 with `variant` - the placement of a candidate's row, see linearity_energy; the result does not depend on
    it -, the select kernel); `run()` records and replays a linear chain as DEPlan does. The warm-up launch that precedes the recording
    is also where the energy entry raises its kernels' dynamic-LDS limit, which is host-side work that stays outside the capture.
    One problem per plan; DEBatchPlanU16 advances several such problems per launch."""
    _entry = "hm_de_generation_u16"

    def __init__(self, dn_stack: torch.Tensor, std_stack: Optional[torch.Tensor], exposures: Sequence[float], mean_icrf, pca,
                 lower_limits, upper_limits, population, lower: int, upper: int, seed: int, max_generations: int,
                 mutation=(0.0, 1.95), recombination: float = 0.4, tol: float = 0.01, energy_limit: float = 0.0,
                 bit_depth: Optional[int] = None, variant: int = 0):
        if isinstance(dn_stack, torch.Tensor) and dn_stack.dtype != _U16:
            raise TypeError(f"DEPlanU16 takes torch.uint16 digital numbers, got {dn_stack.dtype}: uint8 stacks go to DEPlan")
        self.bit_depth = _energy_bit_depth(dn_stack, bit_depth)
        if self.bit_depth is None:                                                   # (not a tensor: _check_stacks raises the TypeError)
            raise ValueError("DEPlanU16 needs bit_depth (9..16): the number of rows of its candidate ICRFs")
        n_rows = 2 ** self.bit_depth
        if not (0 <= int(lower) < n_rows and 0 <= int(upper) < n_rows):
            raise ValueError(f"lower and upper must be DNs in 0..{n_rows - 1} at bit_depth {self.bit_depth}, got {lower}, {upper}")
        if int(variant) not in (0, 1, 2):
            raise ValueError(f"variant must be 0 (the library's choice), 1 (LDS) or 2 (global memory), got {variant}")
        self.variant = int(variant)
        self._init_one(dn_stack, std_stack, exposures, mean_icrf, pca, lower_limits, upper_limits, population, lower, upper, seed,
                       max_generations, mutation, recombination, tol, energy_limit, n_rows, _U16)

    def _call(self, stream):
        lower, upper, S, P, seed, max_gen, m_lo, m_hi, cr, tol, e_lim = self._scalars
        return nat.lib.hm_de_generation_u16(self.population.data_ptr(), self.energies.data_ptr(), self.trial.data_ptr(),
                                            self.trial_energies.data_ptr(), self.icrf.data_ptr(), self.valid.data_ptr(),
                                            self.status.data_ptr(), self.mean_icrf.data_ptr(), self.pca.data_ptr(), self.lo.data_ptr(),
                                            self.hi.data_ptr(), self.dn.data_ptr(), nat.ptr(self.std), self._t, self.n_pixels, self.N,
                                            lower, upper, S, P, seed, max_gen, m_lo, m_hi, cr, tol, e_lim, self.bit_depth, self.variant,
                                            self.workspace.data_ptr(), stream)

    read_status = DEPlan.read_status
    _stopped = DEPlan._stopped


class DEBatchPlan(_DEPlanBase):
    """K independent differential-evolution problems of one shape - the channels of a calibration, restarts of a channel with other seeds,
    or both - advanced by ONE set of launches per generation (hm_de_generation_batch: trial kernel on (S, K) workgroups, the energy
    kernels on K x S candidates, select kernel on K workgroups). Problem k reads stack `stack_of[k]` of `dn_stacks` (default: its own),
    its own mean ICRF, PCA basis and seed, and owns slice k of every state tensor: `population[k]`, `energies[k]`, `trial[k]`,
    `trial_energies[k]`, `icrf[k]`, `valid[k]`, `status[k]`. Every problem evolves bit for bit as a DEPlan with the same inputs would;
    a problem whose stop flag is set costs no further work while the others run. `run()` records `check_every` generations as one
    linear chain (hipGraph), replays it until ALL stop flags are set and reads the K status blocks back with one copy per replay.
    Built inside nat.host_mode() on host stacks, it calls the host build in a loop (no graph)."""
    _entry = "hm_de_generation_batch"

    def __init__(self, dn_stacks: Sequence[torch.Tensor], std_stacks: Optional[Sequence[Optional[torch.Tensor]]], exposures: Sequence[float],
                 mean_icrfs, pcas, lower_limits, upper_limits, populations, lower: int, upper: int, seeds: Sequence[int],
                 max_generations: int, mutation=(0.0, 1.95), recombination: float = 0.4, tol: float = 0.01, energy_limit: float = 0.0,
                 stack_of: Optional[Sequence[int]] = None):
        self._init_batch(dn_stacks, std_stacks, exposures, mean_icrfs, pcas, lower_limits, upper_limits, populations, lower, upper, seeds,
                         max_generations, mutation, recombination, tol, energy_limit, stack_of, BITS, _U8)

    def _call(self, stream):
        return nat.lib.hm_de_generation_batch(*self._batch_head(), self.workspace.data_ptr(), stream)

    def read_status(self) -> list:
        """The K status blocks from ONE copy to the host (this synchronises): a list of DEPlan.read_status() dicts."""
        w = self.status.cpu().numpy()
        return [_status_dict(w[k]) for k in range(self.K)]

    def _stopped(self, status: list) -> bool:
        return all(s["stop"] for s in status)


class DEBatchPlanU16(_DEPlanBase):
    """DEBatchPlan for a 9- to 16-bit camera: K problems on torch.uint16 (X, Y, N) stacks of one shape and ONE `bit_depth` (an int, or one
    per stack - all equal), mean ICRFs of 2**bit_depth entries, PCA bases of (2**bit_depth, P), `lower` / `upper` DNs of that depth. The
    state tensors are DEBatchPlan's with `icrf` of shape (K, S, 2**bit_depth). `launch()` enqueues ONE generation of every problem
    (hm_de_generation_u16_batch: the row walk on (S, 1 | slabs, K) workgroups, the energy kernels on K x S candidates with `variant` -
    the placement of a candidate's row, see linearity_energy; the result does not depend on it -, the select kernel on K workgroups).
    Every problem evolves bit for bit as a DEPlanU16 with the same inputs would; a problem whose stop flag is set costs no further
    work. `run()`, the graph recorded after the warm-up launch (which is also where the dynamic-LDS limit of the `variant` 1 kernels is
    raised, outside the capture), `read_status()` (one copy) and the stop test (all flags) are DEBatchPlan's."""
    _entry = "hm_de_generation_u16_batch"

    def __init__(self, dn_stacks: Sequence[torch.Tensor], std_stacks: Optional[Sequence[Optional[torch.Tensor]]], exposures: Sequence[float],
                 mean_icrfs, pcas, lower_limits, upper_limits, populations, lower: int, upper: int, seeds: Sequence[int],
                 max_generations: int, mutation=(0.0, 1.95), recombination: float = 0.4, tol: float = 0.01, energy_limit: float = 0.0,
                 stack_of: Optional[Sequence[int]] = None, bit_depth=None, variant: int = 0):
        dn_stacks = list(dn_stacks)
        if not dn_stacks:
            raise ValueError("dn_stacks must hold at least one stack")
        for s in dn_stacks:
            if isinstance(s, torch.Tensor) and s.dtype != _U16:
                raise TypeError(f"DEBatchPlanU16 takes torch.uint16 digital numbers, got {s.dtype}: uint8 stacks go to DEBatchPlan")
        depths = list(bit_depth) if isinstance(bit_depth, (list, tuple)) else [bit_depth]
        if len(depths) not in (1, len(dn_stacks)) or any(d != depths[0] for d in depths):
            raise ValueError(f"the stacks of a batch must have one bit depth, got {depths} for {len(dn_stacks)} stacks")
        self.bit_depth = _energy_bit_depth(dn_stacks[0], depths[0])
        if self.bit_depth is None:                                                   # (not a tensor: _check_stacks raises the TypeError)
            raise ValueError("DEBatchPlanU16 needs bit_depth (9..16): the number of rows of its candidate ICRFs")
        n_rows = 2 ** self.bit_depth
        if not (0 <= int(lower) < n_rows and 0 <= int(upper) < n_rows):
            raise ValueError(f"lower and upper must be DNs in 0..{n_rows - 1} at bit_depth {self.bit_depth}, got {lower}, {upper}")
        if int(variant) not in (0, 1, 2):
            raise ValueError(f"variant must be 0 (the library's choice), 1 (LDS) or 2 (global memory), got {variant}")
        self.variant = int(variant)
        self._init_batch(dn_stacks, std_stacks, exposures, mean_icrfs, pcas, lower_limits, upper_limits, populations, lower, upper, seeds,
                         max_generations, mutation, recombination, tol, energy_limit, stack_of, n_rows, _U16)

    def _call(self, stream):
        return nat.lib.hm_de_generation_u16_batch(*self._batch_head(), self.bit_depth, self.variant, self.workspace.data_ptr(), stream)

    read_status = DEBatchPlan.read_status
    _stopped = DEBatchPlan._stopped
