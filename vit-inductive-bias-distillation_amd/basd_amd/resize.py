"""The geometry of the reference's data path -- ``RandomResizedCrop(image_size)`` of the training view and
``Resize(round(image_size / crop_ratio)) -> CenterCrop(image_size)`` of the clean view and of validation
(``src/data/datasets.py:80-94,137-149``) -- on ragged batches of decoded uint8 images as ONE launch of
``basd_resize_crop`` (``csrc/resize.hip``).  With it the loader only decodes: ``collate_ragged`` packs the images of a
batch (``np.asarray(img.convert("RGB"))``, different sizes) into one uint8 buffer, that buffer is uploaded once, and both
views of every image come out of one launch as the dense uint8 NCHW batches ``TrivialAugment`` and ``BatchMixer`` take.

``draw_crop_params`` makes the random crops on the host (CPU generator); ``ResizeCrop`` turns them and the images'
sizes into a table of fixed-size records (``BasdResizeRecord`` of ``include/basd_hip.h``, which also holds the
specification of the resize), sends it with one non-blocking copy and launches once.

The resize is Pillow's 8-bit ``ImagingResample`` of the cropped window, byte for byte, with the filter ``interpolation``
names -- ``"bilinear"`` (the default, the reference's), ``"bicubic"`` or ``"box"``, one for all or one per view: the
specification is held to Pillow and the kernel to the specification in ``tests/test_resize_crop.py`` and
``tests/test_resize_filters.py``.  This is what torchvision's PIL backend does (``Resize(interpolation=BICUBIC)`` on a
PIL image is ``img.resize(size, Image.BICUBIC)`` by its documentation), which is the backend the reference's loader
uses ahead of ``ToImage()``; torchvision's tensor backend resamples in floating point and is not matched.  ``torchvision`` is not installed
where this was written: the draw order and RNG consumption of ``RandomResizedCrop.get_params``, the ``int(...)`` of
``Resize``'s long side and the ``round`` of ``CenterCrop`` are restated from the package's documentation and are NOT
verified against it.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._launch import RecordTable, batch_columns, lives_on, raw_stream, require_gpu

__all__ = ["RaggedBatch", "pack_images", "collate_ragged", "eval_window", "CropParams", "draw_crop_params",
           "make_records", "RECORD_DTYPE", "ResizeCrop", "resize_reference", "VIEWS", "MAX_RATIO", "MAX_SIDE",
           "INTERPOLATIONS", "max_reduction"]

VIEWS = ("clean", "augmented")
MAX_RATIO = 32                      # BASD_RESIZE_MAX_RATIO
MAX_SIDE = 1 << 20                  # BASD_RESIZE_MAX_SIDE
BAD_GEOMETRY, BAD_RATIO, BAD_FILTER = 1, 2, 4      # BASD_RESIZE_BAD_*
INTERPOLATIONS = ("bilinear", "bicubic", "box")    # BASD_RESIZE_FILTER_*: a name's index is its value in a record
_SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "box": 0.5}
_EXCLUDED = {
    "hamming": "its weights need cos, whose last bit differs between math libraries, so the coefficients cannot be "
               "promised to be Pillow's byte for byte",
    "lanczos": "its weights need sin, whose last bit differs between math libraries, so the coefficients cannot be "
               "promised to be Pillow's byte for byte",
    "nearest": "Pillow does not resample it with ImagingResample but with a different code path (an affine transform), "
               "which is not restated here",
}

# BasdResizeRecord: 64 bytes
RECORD_DTYPE = np.dtype([("src_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("win_x", "<i4"), ("win_y", "<i4"),
                         ("win_w", "<i4"), ("win_h", "<i4"), ("res_w", "<i4"), ("res_h", "<i4"), ("out_x", "<i4"),
                         ("out_y", "<i4"), ("filter", "<i4"), ("pad", "<i4", (3,))])
assert RECORD_DTYPE.itemsize == 64 and RECORD_DTYPE.fields["filter"][1] == 48


def _filter_name(name) -> str:
    if isinstance(name, str) and name.lower() in INTERPOLATIONS:
        return name.lower()
    if isinstance(name, str) and name.lower() in _EXCLUDED:
        raise ValueError(f"interpolation {name!r} is not offered: {_EXCLUDED[name.lower()]}; choose one of "
                         f"{INTERPOLATIONS}")
    raise ValueError(f"interpolation must be one of {INTERPOLATIONS} (got {name!r})")


def _check_interpolation(interpolation) -> dict:
    """``{view: filter name}`` for both views of a name or of a dict per view (a view it leaves out is bilinear)."""
    if isinstance(interpolation, dict):
        unknown = [v for v in interpolation if v not in VIEWS]
        if unknown:
            raise ValueError(f"interpolation names the views {unknown}; the views are {VIEWS}")
        return {view: _filter_name(interpolation.get(view, "bilinear")) for view in VIEWS}
    name = _filter_name(interpolation)
    return dict.fromkeys(VIEWS, name)


def max_reduction(filter: str = "bilinear") -> int:
    """The largest ``window / resized`` per axis the launch takes with ``filter``: ``ceil(support * ratio) <= 32`` and
    never above ``MAX_RATIO``, so 32 for bilinear and box, 16 for bicubic."""
    return min(MAX_RATIO, int(MAX_RATIO / _SUPPORT[_filter_name(filter)]))


# ----------------------------------------------------------------------------------------------------------------
# ragged batches
# ----------------------------------------------------------------------------------------------------------------
class RaggedBatch:
    """``B`` decoded images of different sizes in one buffer: ``data`` a 1-D uint8 tensor holding the images back to
    back, each interleaved HWC with ``channels`` bytes per pixel; ``sizes`` a ``(B, 2)`` int32 CPU tensor of
    ``(height, width)``.  The byte offsets are derived (``offsets``).  ``sizes`` stays on the host (the record table is
    built there); ``pin_memory()`` and ``to()`` act on ``data``, so a ``DataLoader(pin_memory=True)`` pins it and one
    ``.to(device, non_blocking=True)`` uploads the batch."""

    def __init__(self, data: torch.Tensor, sizes: torch.Tensor, channels: int = 3) -> None:
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError("data must be a 1-D uint8 tensor")
        if not data.is_contiguous():
            raise ValueError("data must be contiguous")
        sizes = torch.as_tensor(sizes)
        if sizes.dtype not in (torch.int32, torch.int64) or sizes.dim() != 2 or sizes.shape[1] != 2:
            raise ValueError(f"sizes must be a (B, 2) integer tensor of (height, width) (shape {tuple(sizes.shape)})")
        if int(channels) not in (1, 3):
            raise ValueError(f"images must have 1 or 3 channels (got {channels})")
        self.data = data
        self.sizes = sizes.to(device="cpu", dtype=torch.int32).contiguous()
        self.channels = int(channels)
        if len(self) and int(self.sizes.min()) < 1:
            raise ValueError("every image needs a positive height and width")
        if self.nbytes != data.numel():
            raise ValueError(f"sizes describe {self.nbytes} bytes, data holds {data.numel()}")

    def __len__(self) -> int:
        return int(self.sizes.shape[0])

    @property
    def nbytes(self) -> int:
        s = self.sizes.to(torch.int64)
        return int((s[:, 0] * s[:, 1]).sum()) * self.channels

    @property
    def offsets(self) -> np.ndarray:
        """(B,) int64: the byte offset of every image in ``data``."""
        s = self.sizes.numpy().astype(np.int64)
        out = np.zeros(len(self), dtype=np.int64)
        if len(self) > 1:
            np.cumsum(s[:-1, 0] * s[:-1, 1] * self.channels, out=out[1:])
        return out

    @property
    def device(self) -> torch.device:
        return self.data.device

    def image(self, i: int) -> torch.Tensor:
        """Image ``i`` as an (H, W, C) view of ``data``."""
        h, w = (int(v) for v in self.sizes[i])
        start = int(self.offsets[i])
        return self.data[start:start + h * w * self.channels].view(h, w, self.channels)

    def pin_memory(self) -> "RaggedBatch":
        return RaggedBatch(self.data.pin_memory(), self.sizes, self.channels)

    def to(self, *args, **kwargs) -> "RaggedBatch":
        data = self.data.to(*args, **kwargs)
        if data.dtype != torch.uint8:
            raise TypeError("a RaggedBatch stays uint8")
        return self if data is self.data else RaggedBatch(data, self.sizes, self.channels)


def _as_hwc(image) -> np.ndarray:
    if isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8:
            raise TypeError(f"images must be uint8 (got {image.dtype}, shape {tuple(image.shape)})")
        arr = image.detach().cpu().numpy()
    else:
        arr = np.asarray(image)                  # arrays, and PIL images through their array interface
        if arr.dtype != np.uint8:
            raise TypeError(f"images must be uint8 (got {arr.dtype}, shape {arr.shape})")
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if arr.ndim != 3 or arr.shape[2] not in (1, 3):
        raise ValueError(f"images must be (H, W), (H, W, 1) or (H, W, 3) (shape {arr.shape})")
    if arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"images must not be empty (shape {arr.shape})")
    return arr


def pack_images(images: Sequence, channels: Optional[int] = None) -> RaggedBatch:
    """A ``RaggedBatch`` of a list of decoded images: (H, W, C) or (H, W) uint8 arrays or tensors, or PIL images of
    mode ``RGB`` / ``L``.  All of one channel count (``channels``: what an empty list has; default 3)."""
    arrays = [_as_hwc(im) for im in images]
    counts = {a.shape[2] for a in arrays}
    if len(counts) > 1:
        raise ValueError(f"the images of a batch must have one channel count (got {sorted(counts)})")
    C = counts.pop() if counts else (3 if channels is None else int(channels))
    if channels is not None and int(channels) != C:
        raise ValueError(f"images have {C} channels, channels={channels}")
    sizes = torch.tensor([a.shape[:2] for a in arrays], dtype=torch.int32).reshape(-1, 2)
    data = torch.empty(sum(a.size for a in arrays), dtype=torch.uint8)
    flat, at = data.numpy(), 0
    for a in arrays:
        flat[at:at + a.size] = a.reshape(-1)
        at += a.size
    return RaggedBatch(data, sizes, C)


def collate_ragged(samples: Sequence) -> dict:
    """``collate_fn`` of a decode-only loader.  A sample is a dict with an ``"image"`` entry (anything ``pack_images``
    takes) or an ``(image, label)`` pair; the batch is ``{"images": RaggedBatch, ...}`` with every other entry collated
    as ``torch.utils.data.default_collate`` does."""
    from torch.utils.data import default_collate
    samples = list(samples)
    if samples and not isinstance(samples[0], dict):
        samples = [{"image": s[0], "label": s[1]} for s in samples]
    for s in samples:
        if "image" not in s:
            raise KeyError(f"a sample needs an 'image' entry (got {sorted(s)})")
    batch = {"images": pack_images([s["image"] for s in samples])}
    if samples:
        rest = [{k: v for k, v in s.items() if k != "image"} for s in samples]
        if rest[0]:
            batch.update(default_collate(rest))
    return batch


# ----------------------------------------------------------------------------------------------------------------
# the two transforms, restated
# ----------------------------------------------------------------------------------------------------------------
def eval_window(height: int, width: int, image_size: int, crop_ratio: float) -> tuple:
    """``Resize(round(image_size / crop_ratio)) -> CenterCrop(image_size)`` (reference ``build_eval_transform``,
    ``src/data/datasets.py:80-94``) for a ``height`` x ``width`` image: ``(res_h, res_w, top, left)``.  The short side
    goes to ``resize_size``, the long one to ``int(resize_size * long / short)``; the crop's corner is
    ``int(round((res - image_size) / 2.0))`` with Python's ``round`` (halves to even).  A resized image smaller than
    the crop (a ``crop_ratio`` above 1) would be padded by ``CenterCrop``: that is refused."""
    height, width, S = int(height), int(width), int(image_size)
    if height < 1 or width < 1 or S < 1:
        raise ValueError(f"sizes must be positive (got {height} x {width}, image_size {image_size})")
    if not float(crop_ratio) > 0.0:
        raise ValueError(f"crop_ratio must be positive (got {crop_ratio})")
    resize_size = round(S / crop_ratio)
    if width <= height:
        res_w, res_h = resize_size, int(resize_size * height / width)
    else:
        res_h, res_w = resize_size, int(resize_size * width / height)
    if res_h < S or res_w < S:
        raise ValueError(f"a {height} x {width} image resized to {res_h} x {res_w} is smaller than the crop of {S}: "
                         "CenterCrop would pad, which is not supported")
    top = int(round((res_h - S) / 2.0))
    left = int(round((res_w - S) / 2.0))
    return res_h, res_w, top, left


class CropParams(NamedTuple):
    """Per-image crop windows, (B,) each: ``top``, ``left``, ``height``, ``width`` (int64 CPU tensors, or anything
    ``torch.as_tensor`` takes)."""
    top: torch.Tensor
    left: torch.Tensor
    height: torch.Tensor
    width: torch.Tensor


def _sizes_of(sizes) -> torch.Tensor:
    sizes = torch.as_tensor(sizes.sizes if isinstance(sizes, RaggedBatch) else sizes).to(torch.int64)
    if sizes.dim() != 2 or sizes.shape[1] != 2:
        raise ValueError(f"sizes must be (B, 2) of (height, width) (shape {tuple(sizes.shape)})")
    if sizes.numel() and int(sizes.min()) < 1:
        raise ValueError("every image needs a positive height and width")
    return sizes


def draw_crop_params(sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None) -> CropParams:
    """``RandomResizedCrop.get_params`` for images of ``sizes`` ((B, 2) of (height, width), or a ``RaggedBatch``) as a
    pure host function on the CPU generator (``generator=None``: the global one).  Per image up to ten tries: an area
    fraction uniform in ``scale``, an aspect ratio log-uniform in ``ratio``, ``w = int(round(sqrt(area * aspect)))``,
    ``h = int(round(sqrt(area / aspect)))``; the first try that fits the image is placed at a uniform integer offset.
    If none fits: the whole image, clipped to the ratio bounds, centred.  Vectorised over the batch: three calls of the
    generator, each for all images and all ten tries (the reference draws per image inside worker processes, so no
    seed reproduces its sequence anyway); an offset is ``floor(u * count)`` of a uniform ``u``."""
    sizes = _sizes_of(sizes)
    if not (0.0 < scale[0] <= scale[1]) or not (0.0 < ratio[0] <= ratio[1]):
        raise ValueError(f"scale and ratio must be increasing pairs of positive numbers (got {scale}, {ratio})")
    B = sizes.shape[0]
    H, W = sizes[:, 0].tolist(), sizes[:, 1].tolist()
    frac = torch.empty(B, 10, dtype=torch.float64).uniform_(scale[0], scale[1], generator=generator).tolist()
    logr = torch.empty(B, 10, dtype=torch.float64).uniform_(math.log(ratio[0]), math.log(ratio[1]),
                                                            generator=generator).tolist()
    place = torch.rand(B, 10, 2, dtype=torch.float64, generator=generator).tolist()
    top, left, hh, ww = [0] * B, [0] * B, [0] * B, [0] * B
    for b in range(B):
        height, width = H[b], W[b]
        area = height * width
        for t in range(10):
            target = area * frac[b][t]
            aspect = math.exp(logr[b][t])
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                top[b] = min(int(place[b][t][0] * (height - h + 1)), height - h)
                left[b] = min(int(place[b][t][1] * (width - w + 1)), width - w)
                hh[b], ww[b] = h, w
                break
        else:
            in_ratio = float(width) / float(height)
            if in_ratio < ratio[0]:
                w = width
                h = int(round(w / ratio[0]))
            elif in_ratio > ratio[1]:
                h = height
                w = int(round(h * ratio[1]))
            else:
                w, h = width, height
            h, w = max(1, min(h, height)), max(1, min(w, width))
            top[b], left[b], hh[b], ww[b] = (height - h) // 2, (width - w) // 2, h, w
    as_t = lambda v: torch.tensor(v, dtype=torch.int64)                 # noqa: E731
    return CropParams(as_t(top), as_t(left), as_t(hh), as_t(ww))


def _check_views(views) -> tuple:
    views = (views,) if isinstance(views, str) else tuple(views)
    if not views or len(set(views)) != len(views) or any(v not in VIEWS for v in views):
        raise ValueError(f"views must be a non-empty selection of {VIEWS} without repeats (got {views})")
    return views


def make_records(sizes, image_size: int, crop_ratio: float, crop_params: Optional[CropParams] = None, *,
                 views=VIEWS, offsets=None, channels: int = 3, out: Optional[np.ndarray] = None,
                 interpolation: Union[str, dict] = "bilinear") -> np.ndarray:
    """The record table of a ragged batch: ``len(views) * B`` entries of ``RECORD_DTYPE``, view-major (the records of
    ``views[0]`` for all images, then those of ``views[1]``).  ``"clean"``: the whole image as the window, resized as
    ``eval_window`` says, the centre crop as the output rectangle.  ``"augmented"``: the window of ``crop_params``
    resized to ``image_size`` x ``image_size``.  ``offsets``: the images' byte offsets (default: back to back with
    ``channels`` bytes per pixel).  ``interpolation``: one of ``INTERPOLATIONS`` for every record, or a dict per view such
    as ``{"clean": "bicubic", "augmented": "bilinear"}``; it fills the records' ``filter``.  Every limit of
    ``include/basd_hip.h`` is checked here, the reduction against the limit of the view's filter (``max_reduction``);
    a violation raises ``ValueError``."""
    views = _check_views(views)
    filters = _check_interpolation(interpolation)
    sizes = _sizes_of(sizes)
    S, B = int(image_size), sizes.shape[0]
    if S < 1:
        raise ValueError(f"image_size must be positive (got {image_size})")
    H, W = sizes[:, 0].tolist(), sizes[:, 1].tolist()
    if B and max(max(H), max(W)) > MAX_SIDE:
        raise ValueError(f"image sides must not exceed {MAX_SIDE}")
    if offsets is None:
        offsets = np.zeros(B, dtype=np.int64)
        if B > 1:
            np.cumsum(np.asarray(H[:-1], dtype=np.int64) * np.asarray(W[:-1], dtype=np.int64) * int(channels),
                      out=offsets[1:])
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.shape != (B,):
        raise ValueError(f"offsets must hold {B} entries")
    rec = np.zeros(len(views) * B, dtype=RECORD_DTYPE) if out is None else out
    if rec.shape != (len(views) * B,) or rec.dtype != RECORD_DTYPE:
        raise ValueError(f"out must hold {len(views) * B} records")
    if out is not None:
        rec[...] = np.zeros((), dtype=RECORD_DTYPE)
    for v, view in enumerate(views):
        part = rec[v * B:(v + 1) * B]
        part["src_offset"], part["src_h"], part["src_w"] = offsets, H, W
        name = filters[view]
        part["filter"] = INTERPOLATIONS.index(name)
        most = max_reduction(name)
        if view == "clean":
            geo = [eval_window(H[b], W[b], S, crop_ratio) for b in range(B)]
            for b, (res_h, res_w, _, _) in enumerate(geo):
                if H[b] > most * res_h or W[b] > most * res_w or max(res_h, res_w) > MAX_SIDE:
                    raise ValueError(f"image {b} ({H[b]} x {W[b]}) resized to {res_h} x {res_w} is outside the limits "
                                     f"(a {name} reduction of at most {most} per axis, sides up to {MAX_SIDE})")
            if B:
                part["win_w"], part["win_h"] = W, H
                part["res_h"], part["res_w"] = [g[0] for g in geo], [g[1] for g in geo]
                part["out_y"], part["out_x"] = [g[2] for g in geo], [g[3] for g in geo]
        else:
            if crop_params is None:
                raise ValueError("the augmented view needs crop_params")
            top, left, hh, ww = batch_columns(crop_params, B, dict.fromkeys(CropParams._fields, torch.int64)).values()
            for b in range(B):
                if not (0 <= top[b] and 0 <= left[b] and 1 <= hh[b] and 1 <= ww[b] and top[b] + hh[b] <= H[b]
                        and left[b] + ww[b] <= W[b]):
                    raise ValueError(f"the crop window of image {b} (top {top[b]}, left {left[b]}, {hh[b]} x {ww[b]}) "
                                     f"does not lie inside its {H[b]} x {W[b]} image")
                if hh[b] > most * S or ww[b] > most * S:
                    raise ValueError(f"the crop window of image {b} ({hh[b]} x {ww[b]}) is more than {most} times "
                                     f"the image size {S} (the limit of a {name} reduction)")
            if B:
                part["win_x"], part["win_y"], part["win_w"], part["win_h"] = left, top, ww, hh
                part["res_w"], part["res_h"] = S, S
    return rec


# ----------------------------------------------------------------------------------------------------------------
# the launch
# ----------------------------------------------------------------------------------------------------------------
class ResizeCrop:
    """``ResizeCrop(image_size, crop_ratio, device=..., interpolation="bilinear")``.

    ``interpolation``: one of ``INTERPOLATIONS``, or a dict per view (``{"clean": "bicubic", "augmented": "bilinear"}``:
    the clean view the way a timm teacher was trained, the augmented one as the reference makes it); ``.interpolation``
    is the dict of both views.  Records of different filters share the table and the launch.

    ``rc(ragged, crop_params=None, *, views=("clean", "augmented")) -> {view: uint8 (B, C, S, S)}``: ``ragged`` a
    ``RaggedBatch`` whose data lives on ``device``; ``crop_params=None`` draws with ``draw_crop_params`` (global CPU
    generator) when the augmented view is asked for.  The views are slices of one allocation.  The record table is
    built in a pinned host buffer and sent with one non-blocking copy into a persistent device table (both grow to the
    largest batch seen); then exactly one launch on the current stream, no wait for the device.  ``status()`` reads
    the kernel's status word back (0: clean; it waits for the device)."""

    def __init__(self, image_size: int, crop_ratio: float, *, device,
                 interpolation: Union[str, dict] = "bilinear") -> None:
        self.image_size = int(image_size)
        self.crop_ratio = float(crop_ratio)
        if self.image_size < 1 or self.image_size > MAX_SIDE:
            raise ValueError(f"image_size must lie in [1, {MAX_SIDE}] (got {image_size})")
        if not self.crop_ratio > 0.0:
            raise ValueError(f"crop_ratio must be positive (got {crop_ratio})")
        self.interpolation = _check_interpolation(interpolation)
        self.device = torch.device(device)
        self._records = RecordTable(RECORD_DTYPE)

    def status(self) -> int:
        return self._records.status()

    def __call__(self, ragged: RaggedBatch, crop_params: Optional[CropParams] = None, *, views=VIEWS) -> dict:
        # every argument is checked before the device is: a CPU batch with a wrong argument reports the argument
        if not isinstance(ragged, RaggedBatch):
            raise TypeError(f"ragged must be a RaggedBatch (got {type(ragged).__name__}); pack_images makes one")
        views = _check_views(views)
        if not lives_on(self.device, ragged.device):
            raise ValueError(f"the images live on {ragged.device}, the resizer on {self.device}")
        B, C, S = len(ragged), ragged.channels, self.image_size
        if C * S * S >= 1 << 30:
            raise ValueError(f"an output image of {C} x {S} x {S} bytes is too large")
        if crop_params is None and "augmented" in views:
            crop_params = draw_crop_params(ragged.sizes)
        offsets = ragged.offsets
        checked = make_records(ragged.sizes, S, self.crop_ratio, crop_params, views=views, offsets=offsets,
                               interpolation=self.interpolation)
        require_gpu(ragged.data, f"the {B} images")
        n = len(views) * B
        out = torch.empty((n, C, S, S), dtype=torch.uint8, device=ragged.device)
        result = {view: out[v * B:(v + 1) * B] for v, view in enumerate(views)}
        if n == 0:
            return result
        self._records.stage(n, ragged.device)[...] = checked
        _lib.call("basd_resize_crop", ragged.data.data_ptr(), ragged.data.numel(), out.data_ptr(), n, C, S, S,
                  self._records.upload(), self._records.status_ptr, 0, raw_stream(ragged.device.index))
        return result


# ----------------------------------------------------------------------------------------------------------------
# the specification in numpy (tests and the goldens script; the product path does not use it)
# ----------------------------------------------------------------------------------------------------------------
def _reference_weight(filter: str, t: float) -> float:
    if filter == "box":
        return 1.0 if -0.5 < t <= 0.5 else 0.0                   # of t itself: the asymmetry is Pillow's
    t = abs(t)
    if filter == "bilinear":
        return 1.0 - t if t < 1.0 else 0.0
    a = -0.5
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def _reference_taps(size_in: int, size_out: int, xx: int, filter: str = "bilinear"):
    """(first source index, int coefficients) of output index ``xx``: Python floats are fp64, every operation rounded
    on its own."""
    scale = float(size_in) / size_out
    fs = max(scale, 1.0)
    support, inv = _SUPPORT[filter] * fs, 1.0 / fs
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), size_in)
    w, ww = [], 0.0
    for x in range(xmax - xmin):
        w.append(_reference_weight(filter, (x + xmin - center + 0.5) * inv))
        ww += w[-1]
    if ww != 0.0:
        w = [v / ww for v in w]
    return xmin, np.array([int(-0.5 + v * 4194304.0) if v < 0.0 else int(0.5 + v * 4194304.0) for v in w],
                          dtype=np.int64)


def _reference_pass(img: np.ndarray, size_out: int, first: int, count: int, filter: str = "bilinear",
                    extremes: Optional[list] = None) -> np.ndarray:
    """Output indices ``first .. first + count`` of the pass along axis 0 of ``img`` (n, ...) resized to ``size_out``.
    ``extremes``: a list ``[lowest, highest]`` of the unclamped accumulators seen so far, updated in place."""
    out = np.empty((count,) + img.shape[1:], dtype=np.uint8)
    shape = (-1,) + (1,) * (img.ndim - 1)
    for i in range(count):
        xmin, k = _reference_taps(img.shape[0], size_out, first + i, filter)
        acc = (1 << 21) + (k.reshape(shape) * img[xmin:xmin + len(k)].astype(np.int64)).sum(axis=0)
        if extremes is not None and acc.size:
            extremes[0], extremes[1] = min(extremes[0], int(acc.min())), max(extremes[1], int(acc.max()))
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def resize_reference(image: np.ndarray, window, resized, rect=None, filter: str = "bilinear",
                     extremes: Optional[list] = None) -> np.ndarray:
    """The specification of ``include/basd_hip.h`` in numpy: ``image`` (H, W, C) uint8, ``window`` ``(win_x, win_y,
    win_w, win_h)``, ``resized`` ``(res_w, res_h)``, ``rect`` ``(out_x, out_y, OW, OH)`` (default: the whole resized
    image), ``filter`` one of ``INTERPOLATIONS``.  Returns the rectangle as (OH, OW, C): the horizontal pass first,
    rounded to uint8, then the vertical one.  ``extremes``: a list ``[lowest, highest]`` that is updated with the
    unclamped accumulators of both passes (what the tests use to show that a case reaches the clamp)."""
    filter = _filter_name(filter)
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    win_x, win_y, win_w, win_h = (int(v) for v in window)
    res_w, res_h = (int(v) for v in resized)
    out_x, out_y, OW, OH = (0, 0, res_w, res_h) if rect is None else (int(v) for v in rect)
    win = image[win_y:win_y + win_h, win_x:win_x + win_w]
    assert win.shape[:2] == (win_h, win_w) and out_x + OW <= res_w and out_y + OH <= res_h
    horizontal = _reference_pass(win.transpose(1, 0, 2), res_w, out_x, OW, filter, extremes).transpose(1, 0, 2)
    return _reference_pass(horizontal, res_h, out_y, OH, filter, extremes)                        # from (win_h, OW, C)
