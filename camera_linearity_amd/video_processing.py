"""Mean / STD frames of a video - mirror of modules/video_processing.py:161-262 on the HIP backend - and the camera
noise profiles with the per-DN STD table computed from them (:12-133). The mean / STD frames are also available for the uint16 frames
of 9- to 16-bit cameras (`bit_depth=`); the noise profiles stay 8-bit: their (2^b, 2^b, C) joint histogram does not scale to 16 bits.
The per-DN STD table of such a camera comes from `compute_noise_moments` / `noise_moments_to_STD_data` instead: three integers per
(mean level, channel) - count, sum of d, sum of d^2 with d = frame DN - mean DN - are all `_calculate_STD` uses of a profile row.

The reference streams frames out of `cv.VideoCapture` one at a time and updates three whole-image NumPy
arrays per frame (video_processing.py:199-208). Here the decoded frames are uploaded in batches and folded
into the device-resident float64 state by `hm_welford_update`, which reads and writes the state once per
batch (not once per frame); the frame order and the per-frame arithmetic are the reference's.

Video decoding stays with the caller: OpenCV is not a dependency of this package, so `welford_algorithm`
takes any iterable of uint8 (H, W, C) frames - e.g. `frames_from_capture(cv.VideoCapture(path))` - or a list
of such iterables (the reference's "all videos of a directory" mode, :193-195).

Deviation K (SURVEY.md 3.4 style): `if ICRF:` at :200 raises for an ndarray; the intended `ICRF is not None` is used.

Noise profiles (`compute_noise_profiles`, :77-106) count, per channel, every (mean-frame DN, frame DN) pair of every frame
into a (256, 256, C) int64 array (`hm_noise_profile_update`, a banded joint histogram in LDS); `_calculate_STD` (:109-133)
and `noise_profiles_to_STD_data` turn it into the (256, C) float64 table of `ImageSet.calculate_numerical_STD`, and
`clean_data_edges` (:12-74) runs the reference's integer cleaning passes. Sources are decoded frames as for
`welford_algorithm`; as the reference reads every video twice (once for the mean), a source must be iterable twice (a
list, or a zero-argument callable returning a fresh iterable) unless the caller passes `mean_frame=`.

Deviation L (SURVEY.md 3.4 style): `_calculate_STD` calls `math.sqrt` at :130 without importing `math` and raises NameError;
the intended `math.sqrt` is used, so a level without counts gives NaN (0 / 0 and sqrt(NaN)).
"""
from __future__ import annotations

from typing import Iterable, Iterator, Optional, Sequence, Union

import numpy as np
import torch

from . import engine
from .settings import BITS


def _engine_for(device: torch.device):
    """The HIP library for a GPU device; the host build of the same ABI for device="cpu" - an explicit choice (the reference's NumPy
    slot), never a fallback: the default device is the current GPU and the calls below raise without one."""
    if device.type == "cuda":
        return engine
    from .measurand import _HOST_ENGINE
    return _HOST_ENGINE


FRAMES_PER_LAUNCH = 32      # = HM_MAX_FRAMES: state traffic per element-frame = 32 / 32 = 1 byte with std (measured best)


def frames_from_capture(capture) -> Iterator[np.ndarray]:
    """general_functions.video_frame_generator (modules/general_functions.py:226-251) for an already opened
    cv.VideoCapture-like object (`isOpened()`, `read() -> (ok, frame)`, `release()`)."""
    if not capture.isOpened():
        raise ValueError("Unable to open video file")
    try:
        while True:
            ok, frame = capture.read()
            if not ok:
                break
            yield frame
    finally:
        capture.release()


def _as_device_frame(frame, device, bit_depth=None) -> torch.Tensor:
    """A decoded frame as a device tensor: uint8, or - with `bit_depth` (9..16) - the uint16 frame of such a camera."""
    if isinstance(frame, torch.Tensor):
        t = frame
    else:
        t = torch.from_numpy(np.ascontiguousarray(frame))
    if bit_depth is None:
        if t.dtype != torch.uint8:
            raise TypeError(f"video frames must be uint8, got {t.dtype}" + (
                " (welford_algorithm takes uint16 frames with bit_depth=9..16)" if t.dtype == torch.uint16 else ""))
    elif t.dtype != torch.uint16:
        raise ValueError(f"bit_depth is for uint16 video frames, got {t.dtype}")
    if t.dim() == 2:
        t = t[..., None]
    if torch.device(device).type == "cpu":
        return t.clone()                      # (a capture may hand out the same buffer again; a batch of frames is pending at a time)
    return t.to(device, non_blocking=True)


def welford_algorithm(frame_sources: Union[Iterable, Sequence[Iterable]], ICRF: Optional[np.ndarray] = None,
                      use_std: Optional[bool] = False, device=None, frames_per_launch: int = FRAMES_PER_LAUNCH,
                      as_numpy: bool = True, bit_depth: Optional[int] = None):
    """Mean frame and standard-deviation-of-the-mean frame over all frames (video_processing.py:161-219).

    Args:
        frame_sources: an iterable of uint8 (H, W, C) frames, or a list of such iterables (several videos folded
            into one result). A frame of None ends a source (the reference's generator protocol, :192-193).
        ICRF: (BITS, NUM_OF_CHS) float64 inverse camera response; frames are linearized on load when given.
        use_std: whether to compute the standard deviation frame.
        device: the GPU to compute on (default: the current one), or "cpu" for the host build (libhdrmerge_host.so).
        bit_depth: 9..16 for the uint16 frames (NumPy or tensors) of such a camera: MAX_DN becomes 2**bit_depth - 1, the ICRF has
            2**bit_depth rows, and the result frames are uint16 (hm_welford_update_u16 / hm_welford_finalize_u16).
    Returns:
        {'mean': uint8 (H, W, C), 'std': uint8 (H, W, C) or None} - NumPy arrays (or device tensors with as_numpy=False).
    """
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    eng = _engine_for(device)
    if frames_per_launch < 1:
        raise ValueError("frames_per_launch must be positive")
    if bit_depth is not None:
        bit_depth = engine._check_bit_depth(bit_depth)
    if isinstance(frame_sources, (list, tuple)) and frame_sources and not _looks_like_frame(frame_sources[0]):
        sources = list(frame_sources)
    else:
        sources = [frame_sources]

    mean = m2 = None
    count = 0
    pending = []

    def flush():
        nonlocal count
        if pending:
            count = eng.welford_update(pending, count, mean, m2, ICRF, bit_depth=bit_depth)
            pending.clear()

    for source in sources:
        for frame in source:
            if frame is None:
                break
            t = _as_device_frame(frame, device, bit_depth)
            if mean is None:
                mean = torch.zeros(t.shape, dtype=torch.float64, device=device)              # :181
                m2 = torch.zeros(t.shape, dtype=torch.float64, device=device) if use_std else None   # :184
            elif t.shape != mean.shape:
                raise ValueError(f"frame shape {tuple(t.shape)} differs from the first frame's {tuple(mean.shape)}")
            pending.append(t)
            if len(pending) == frames_per_launch:
                flush()
    flush()
    if mean is None:
        raise ValueError("no frames to process")
    if use_std and count < 2:
        raise ValueError("the standard deviation frame needs at least two frames")
    out_mean, out_std = eng.welford_finalize(mean, m2, count, bit_depth=bit_depth)
    if as_numpy:
        return {"mean": out_mean.cpu().numpy(), "std": None if out_std is None else out_std.cpu().numpy()}
    return {"mean": out_mean, "std": out_std}


def _looks_like_frame(x) -> bool:
    return x is None or (isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim in (2, 3))


def save_result(ret: dict, video_path) -> None:
    """The file naming of process_video (video_processing.py:222-236): '<video>.mean.tif' / '<video>.std.tif'
    next to the video, written with cv.imwrite's conventions."""
    from pathlib import Path
    from . import tiff_io
    video_path = Path(video_path)
    for key in ret:
        if ret[key] is not None:
            img = ret[key].cpu().numpy() if isinstance(ret[key], torch.Tensor) else ret[key]
            tiff_io.imwrite(video_path.parent.joinpath(video_path.name.replace(".avi", f".{key}.tif")), img)


def process_video(frame_source, video_path, ICRF: Optional[np.ndarray] = None, use_std: Optional[bool] = True,
                  bit_depth: Optional[int] = None):
    """video_processing.py:222-236 for an already opened frame source (`bit_depth`: welford_algorithm's; the TIFFs are then uint16)."""
    ret = welford_algorithm(frame_source, ICRF, use_std, bit_depth=bit_depth)
    save_result(ret, video_path)
    return ret


# ------------------------------------------------------------------------------------------------
# noise profiles and the per-DN STD table (video_processing.py:12-133)
# ------------------------------------------------------------------------------------------------
def _source_list(frame_sources) -> list:
    if callable(frame_sources):
        return [frame_sources]
    if isinstance(frame_sources, (list, tuple)) and frame_sources and not _looks_like_frame(frame_sources[0]):
        return list(frame_sources)
    return [frame_sources]


def _fresh(source):
    return source() if callable(source) else source


def compute_noise_profiles(frame_sources, mean_frame=None, device=None, frames_per_launch: int = FRAMES_PER_LAUNCH,
                           as_numpy: bool = True):
    """Noise profiles of a camera from frames of a static scene (video_processing.py:77-106).

    Args:
        frame_sources: an iterable of uint8 (H, W, C) (or (H, W)) frames, a list of such iterables (several videos folded into
            one result), or a zero-argument callable returning a fresh iterable (also as list items). A frame of None ends a source.
            Without `mean_frame` every source is read twice, so a one-shot iterator is rejected.
        mean_frame: uint8 (H, W, C) mean frame to count against; default: welford_algorithm's mean over all frames (:89).
        device: the GPU to compute on (default: the current one), or "cpu" for the host build (libhdrmerge_host.so).
    Returns:
        (profiles int64 (256, 256, C), mean_frame uint8 (H, W, C)) - NumPy arrays (device tensors with as_numpy=False);
        profiles[m, f, c] counts the elements of channel c with mean DN m and frame DN f.
    """
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    eng = _engine_for(device)
    if frames_per_launch < 1:
        raise ValueError("frames_per_launch must be positive")
    sources = _source_list(frame_sources)
    if mean_frame is None:
        for src in sources:
            if not callable(src) and iter(src) is src:
                raise ValueError("compute_noise_profiles reads every source twice (mean frame, then profiles): pass lists, "
                                 "zero-argument callables returning fresh iterables, or mean_frame=")
        mean = welford_algorithm([_fresh(s) for s in sources], None, False, device=device, frames_per_launch=frames_per_launch,
                                 as_numpy=False)["mean"]                                     # :89
    else:
        mean = _as_device_frame(mean_frame, device).contiguous()
    C = mean.shape[-1]
    profiles = torch.zeros((BITS, BITS, C), dtype=torch.int64, device=device)              # :87
    pending = []

    def flush():
        if pending:
            eng.noise_profile_update(pending, mean, profiles)
            pending.clear()

    for src in sources:
        for frame in _fresh(src):
            if frame is None:
                break
            t = _as_device_frame(frame, device)
            if t.shape != mean.shape:
                raise ValueError(f"frame shape {tuple(t.shape)} differs from the mean frame's {tuple(mean.shape)}")
            pending.append(t)
            if len(pending) == frames_per_launch:
                flush()
    flush()
    if as_numpy:
        return profiles.cpu().numpy(), mean.cpu().numpy()
    return profiles, mean


def compute_noise_moments(frame_sources, mean_frame=None, device=None, bit_depth: Optional[int] = None,
                          frames_per_launch: int = FRAMES_PER_LAUNCH, as_numpy: bool = True):
    """Per-level noise moments of a 9- to 16-bit camera from uint16 frames of a static scene: what `_calculate_STD` needs of the noise
    profile - a count, the sum of d and the sum of d^2 per (mean level, channel), d = frame DN - mean DN - without the (2^b, 2^b, C)
    histogram. `noise_moments_to_STD_data` turns them into the per-DN STD table.

    Args:
        frame_sources: as `compute_noise_profiles`, with uint16 (H, W, C) (or (H, W)) frames. Without `mean_frame` every source is read
            twice, so a one-shot iterator is rejected.
        mean_frame: uint16 (H, W, C) mean frame to count against; default: welford_algorithm(..., bit_depth=bit_depth)'s mean.
        device: the GPU to compute on (default: the current one), or "cpu" for the host build (libhdrmerge_host.so).
        bit_depth: 9..16, the camera's DN range; DNs are masked to it.
    Returns:
        (moments int64 (2**bit_depth, C, 3), mean_frame uint16 (H, W, C)) - NumPy arrays (device tensors with as_numpy=False);
        moments[m, c] = (count, sum d, sum d^2) over the elements of channel c whose mean DN is m.
    """
    bit_depth = engine._check_bit_depth(bit_depth)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    eng = _engine_for(device)
    if frames_per_launch < 1:
        raise ValueError("frames_per_launch must be positive")
    sources = _source_list(frame_sources)
    if mean_frame is None:
        for src in sources:
            if not callable(src) and iter(src) is src:
                raise ValueError("compute_noise_moments reads every source twice (mean frame, then moments): pass lists, "
                                 "zero-argument callables returning fresh iterables, or mean_frame=")
        mean = welford_algorithm([_fresh(s) for s in sources], None, False, device=device, frames_per_launch=frames_per_launch,
                                 as_numpy=False, bit_depth=bit_depth)["mean"]
    else:
        mean = _as_device_frame(mean_frame, device, bit_depth).contiguous()
    C = mean.shape[-1]
    moments = torch.zeros((2 ** bit_depth, C, 3), dtype=torch.int64, device=device)
    pending = []

    def flush():
        if pending:
            eng.noise_moments_update(pending, mean, moments, bit_depth)
            pending.clear()

    for src in sources:
        for frame in _fresh(src):
            if frame is None:
                break
            t = _as_device_frame(frame, device, bit_depth)
            if t.shape != mean.shape:
                raise ValueError(f"frame shape {tuple(t.shape)} differs from the mean frame's {tuple(mean.shape)}")
            pending.append(t)
            if len(pending) == frames_per_launch:
                flush()
    flush()
    if as_numpy:
        return moments.cpu().numpy(), mean.cpu().numpy()
    return moments, mean


def noise_moments_to_STD_data(moments, bit_depth, device=None):
    """(2**bit_depth, C) float64 STD table of a 9- to 16-bit camera from `compute_noise_moments`' moments: row k is the standard deviation
    of the frames at mean level k on the DN grid k / (2**bit_depth - 1), NaN for a level without counts. The std table of
    `engine.linearize(frame_u16, None, table, bit_depth=bit_depth)`. NumPy in, NumPy out; a tensor stays a tensor on its device."""
    bit_depth = engine._check_bit_depth(bit_depth)
    is_np = not isinstance(moments, torch.Tensor)
    if is_np:
        a = np.asarray(moments)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"moments must be an integer array, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    else:
        if moments.dtype.is_floating_point or moments.dtype == torch.bool:
            raise TypeError(f"moments must be an integer tensor, got {moments.dtype}")
        t = moments
        dev = moments.device if device is None else torch.device(device)
    if t.dim() != 3 or t.shape[0] != 2 ** bit_depth or t.shape[2] != 3:
        raise ValueError(f"moments must be shaped ({2 ** bit_depth}, C, 3) at bit_depth {bit_depth}, got {tuple(t.shape)}")
    out = _engine_for(dev).noise_moments_std(t.to(device=dev, dtype=torch.int64).contiguous(), bit_depth)
    return out.cpu().numpy() if is_np else out


def _profiles_tensor(arr, device, what: str):
    """-> (device tensor (256, 256, C) int64, was a NumPy array, channel axis added). Device tensors keep their device."""
    is_np = not isinstance(arr, torch.Tensor)
    if is_np:
        a = np.asarray(arr)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{what} must be an integer array, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    else:
        if arr.dtype.is_floating_point or arr.dtype == torch.bool:
            raise TypeError(f"{what} must be an integer tensor, got {arr.dtype}")
        t = arr
        dev = arr.device if device is None else torch.device(device)
    squeeze = t.dim() == 2
    if squeeze:
        t = t[..., None]
    if t.dim() != 3 or tuple(t.shape[:2]) != (BITS, BITS):
        raise ValueError(f"{what} must be shaped ({BITS}, {BITS}) or ({BITS}, {BITS}, C), got {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.int64).contiguous(), is_np, squeeze


def noise_profiles_to_STD_data(profiles, device=None):
    """(256, C) float64 STD table (`process_STD_data`'s STD_data, video_processing.py:136-158, without its text files): column c
    is _calculate_STD(profiles[:, :, c]). The input of ImageSet.calculate_numerical_STD / load_std_image(STD_data)."""
    t, is_np, squeeze = _profiles_tensor(profiles, device, "profiles")
    out = _engine_for(t.device).noise_profile_std(t)
    if squeeze:
        out = out[:, 0]
    return out.cpu().numpy() if is_np else out


def _calculate_STD(mean_data_array, device=None):
    """video_processing.py:109-133: the standard deviation of every signal level of ONE channel's (256, 256) profile,
    shape (256,) float64 (deviation L: NaN for a level without counts)."""
    if tuple(np.shape(mean_data_array) if not isinstance(mean_data_array, torch.Tensor) else mean_data_array.shape) != (BITS, BITS):
        raise ValueError(f"_calculate_STD takes one channel's ({BITS}, {BITS}) array")
    return noise_profiles_to_STD_data(mean_data_array, device)


def clean_data_edges(base_data_arr, device=None):
    """video_processing.py:12-74 on a (256, 256) or (256, 256, C) integer array (every channel), IN PLACE; returns it."""
    t, is_np, _ = _profiles_tensor(base_data_arr, device, "base_data_arr")
    _engine_for(t.device).noise_profile_clean_edges(t)
    if is_np:
        base_data_arr[...] = t.cpu().numpy().reshape(base_data_arr.shape)
    elif t.data_ptr() != base_data_arr.data_ptr():
        base_data_arr.copy_(t.reshape(base_data_arr.shape))
    return base_data_arr
