"""The decode of the reference's loader for the datasets that ship PNG files (``uoft-cs/cifar100`` of
``configs/experiment/basd_cifar100.yaml``) on the device, beside ``basd_amd.jpeg`` and in its shape: the loader ships
file bytes, ``collate_png`` packs the ``IDAT`` payloads of a batch into one uint8 buffer, that buffer is uploaded once,
and the two launches of ``basd_png_decode`` (``csrc/png.hip``: inflate, then Adler-32 / unfilter / colour) write the
decoded images as the ``RaggedBatch`` of three channels ``ResizeCrop`` takes.

``parse_png`` walks a file's chunks on the host and says whether the device decodes it (8 bits, colour types 0, 2, 3,
4, 6, no interlace: the scope is spelled out in ``include/basd_hip.h``, which also holds the specification); every
other file goes through ``pack_pngs``'s ``fallback`` (default: Pillow, where it is importable -- so a JPEG in a PNG
batch still works) and travels as a "raw" record of decoded pixels in the same buffer.

PNG is lossless, so "Pillow's bytes" are the source pixels: ``inflate_reference`` and ``decode_reference`` restate the
specification in plain Python and are held to zlib and to Pillow, the kernels are held to them, in
``tests/test_png_decode.py``.  There is no CPU fallback of the kernels.
"""
from __future__ import annotations

import struct
from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._launch import RecordTable, lives_on, raw_stream, require_gpu, retire
from .jpeg import _default_fallback
from .resize import RaggedBatch

__all__ = ["PngHeader", "parse_png", "UnsupportedPng", "PngBatch", "pack_pngs", "collate_png", "PngDecoder",
           "decode_reference", "inflate_reference", "RECORD_DTYPE", "MAX_SIDE", "MAX_BATCH", "STATUS_NAMES"]

MAX_SIDE = 16384                    # BASD_PNG_MAX_SIDE
MAX_BATCH = 65535                   # BASD_PNG_MAX_BATCH
KIND_STREAM, KIND_RAW = 0, 1        # BASD_PNG_KIND_*
STATUS_NAMES = {0: "decoded", 1: "bad record", 2: "bad block type", 3: "stored LEN is not ~NLEN", 4: "bad code lengths",
                5: "invalid code", 6: "distance past the bytes produced", 7: "truncated", 8: "wrong length",
                9: "bad filter type", 10: "Adler-32 mismatch"}
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIGNATURE = b"\x89PNG\r\n\x1a\n"

# BasdPngRecord: 64 bytes
RECORD_DTYPE = np.dtype([("src_offset", "<i8"), ("out_offset", "<i8"), ("ws_offset", "<i8"), ("plte_offset", "<i8"),
                         ("src_len", "<i4"), ("kind", "<i4"), ("width", "<i4"), ("height", "<i4"), ("color_type", "<i4"),
                         ("pad", "<i4", (3,))])
assert RECORD_DTYPE.itemsize == 64


class UnsupportedPng(ValueError):
    """A file the device does not decode and no fallback took: ``index`` in its batch, ``reason``."""

    def __init__(self, index: int, reason: str) -> None:
        super().__init__(f"image {index} is not decoded on the device ({reason}) and there is no fallback for it")
        self.index = index
        self.reason = reason


# ----------------------------------------------------------------------------------------------------------------
# the header
# ----------------------------------------------------------------------------------------------------------------
class PngHeader(NamedTuple):
    """What ``parse_png`` found.  ``reason``: ``None`` where the device decodes the file, else why not (the other fields
    then hold what was read up to that point).  ``idat``: the ``(offset, length)`` of every ``IDAT`` payload, in the
    file's order; ``plte``: the ``(offset, length)`` of the ``PLTE`` payload, or ``None``."""
    reason: Optional[str]
    width: int = 0
    height: int = 0
    color_type: int = 0
    bit_depth: int = 0
    idat: tuple = ()
    plte: Optional[tuple] = None

    @property
    def filtered_bytes(self) -> int:
        return self.height * (self.width * BPP.get(self.color_type, 0) + 1)


def parse_png(data) -> PngHeader:
    """The chunks of a file's bytes.  Never raises on malformed input: what the device does not decode has ``reason``
    set (a JPEG: "not a PNG file ..."; 16-bit, Adam7, a palette below 8 bits, ...: named).  Chunk CRCs are NOT checked:
    Pillow decodes a file whose ``IDAT`` CRC is wrong too, and the Adler-32 of the inflated bytes is checked on the
    device.  ``tRNS``, ``gAMA``, ``iCCP``, ``bKGD``, ``acTL`` and every other ancillary chunk are skipped, as
    ``convert("RGB")`` ignores them."""
    buf = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    n = len(buf)
    if buf[:8] != SIGNATURE:
        return PngHeader(f"not a PNG file (it starts with {bytes(buf[:8]).hex() or 'nothing'}, not {SIGNATURE.hex()})")
    if n < 8 + 25:
        return PngHeader("a truncated header")
    length, kind = struct.unpack_from(">I4s", buf, 8)
    if kind != b"IHDR" or length != 13:
        return PngHeader("a broken chunk structure (the first chunk is not IHDR)")
    width, height, depth, ctype, comp, filt, lace = struct.unpack_from(">IIBBBBB", buf, 16)
    base = dict(width=width, height=height, color_type=ctype, bit_depth=depth)
    if ctype not in BPP:
        return PngHeader(f"colour type {ctype}", **base)
    if depth != 8:
        return PngHeader(f"{depth}-bit samples" + (" (a palette of at most 16 colours)" if ctype == 3 else ""), **base)
    if comp != 0 or filt != 0:
        return PngHeader(f"compression method {comp}, filter method {filt}", **base)
    if lace != 0:
        return PngHeader("interlaced (Adam7)" if lace == 1 else f"interlace method {lace}", **base)
    if width == 0 or height == 0:
        return PngHeader(f"{width} x {height} pixels", **base)
    if width > MAX_SIDE or height > MAX_SIDE:
        return PngHeader(f"{width} x {height} pixels (the device decodes sides up to {MAX_SIDE})", **base)
    at, idat, plte, closed, ended = 8 + 25, [], None, False, False
    while at < n:
        if at + 12 > n:
            return PngHeader("a broken chunk structure (the file ends inside a chunk)", **base)
        length, kind = struct.unpack_from(">I4s", buf, at)
        if length > n - at - 12:
            return PngHeader(f"a broken chunk structure (the file ends inside {kind!r})", **base)
        if kind == b"IDAT":
            if closed:
                return PngHeader("IDAT chunks that do not follow one another", **base)
            idat.append((at + 8, length))
        else:
            closed = bool(idat)
            if kind == b"PLTE":
                if length % 3 or length > 768 or length == 0 or idat or plte is not None:
                    return PngHeader("a bad PLTE chunk", **base)
                plte = (at + 8, length)
            elif kind == b"IEND":
                ended = True
                break
        at += 12 + length
    if not idat:
        return PngHeader("no IDAT chunk", **base)
    if not ended:
        return PngHeader("a broken chunk structure (no IEND chunk)", **base)
    if ctype == 3 and plte is None:
        return PngHeader("a palette image without PLTE", **base)
    total = sum(length for _, length in idat)
    if total > (1 << 31) - 17:
        return PngHeader(f"a stream of {total} bytes (the limit is {(1 << 31) - 17})", **base)
    head = b""
    for o, l in idat:                                  # the two header bytes may lie in different chunks
        head += buf[o:o + min(l, 2 - len(head))]
        if len(head) == 2:
            break
    if len(head) < 2:
        return PngHeader("a zlib header that is cut short", **base)
    cmf, flg = head
    if (cmf & 15) != 8 or (cmf >> 4) > 7:
        return PngHeader(f"a zlib header that is not deflate with a window of at most 32 KiB (CMF {cmf:#04x})", **base)
    if flg & 0x20:
        return PngHeader("a zlib header with a preset dictionary", **base)
    if (cmf * 256 + flg) % 31:
        return PngHeader("a zlib header that fails its check", **base)
    return PngHeader(None, idat=tuple(idat), plte=plte, **base)


# ----------------------------------------------------------------------------------------------------------------
# batches of files
# ----------------------------------------------------------------------------------------------------------------
def status_bytes(batch: int) -> int:
    """``basd_png_status_bytes``: per image a status word and the offset of the Adler-32 bytes, at the workspace's
    start."""
    return (8 * batch + 127) & ~127


def _filtered_of(rec: np.ndarray) -> np.ndarray:
    """Per record the bytes of its filtered scanlines (int64; a raw record has none)."""
    bpp = np.zeros(rec.shape[0], dtype=np.int64)
    for ctype, b in BPP.items():
        bpp[rec["color_type"] == ctype] = b
    n = rec["height"].astype(np.int64) * (rec["width"].astype(np.int64) * bpp + 1)
    return np.where(rec["kind"] == KIND_STREAM, n, 0)


class PngBatch:
    """``B`` files in one buffer: ``data`` a 1-D uint8 tensor (a multiple of 16 bytes) that holds per file the
    concatenated ``IDAT`` payloads, the 768 palette bytes of the palette images and the decoded pixels of the files the
    fallback took; ``records`` the ``B`` rows of ``RECORD_DTYPE`` (host); ``sizes`` a ``(B, 2)`` int32 CPU tensor of
    ``(height, width)``.  ``pin_memory()`` and ``to()`` act on ``data``.  ``workspace_bytes``: the workspace the batch
    uses (the status area, then every stream's filtered scanlines at a multiple of 16); ``max_filtered`` /
    ``max_pixels``: the largest image's."""

    def __init__(self, data: torch.Tensor, records: np.ndarray, sizes: torch.Tensor) -> None:
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError("data must be a 1-D uint8 tensor")
        if not data.is_contiguous() or data.numel() % 16:
            raise ValueError(f"data must be contiguous and a multiple of 16 bytes long (got {data.numel()})")
        if records.dtype != RECORD_DTYPE or records.ndim != 1:
            raise TypeError("records must be a 1-D array of RECORD_DTYPE")
        sizes = torch.as_tensor(sizes).to(device="cpu", dtype=torch.int32).reshape(-1, 2).contiguous()
        if sizes.shape[0] != records.shape[0]:
            raise ValueError(f"{records.shape[0]} records for {sizes.shape[0]} sizes")
        if records.shape[0] > MAX_BATCH:
            raise ValueError(f"a batch holds at most {MAX_BATCH} images (got {records.shape[0]})")
        self.data, self.records, self.sizes = data, records, sizes
        filtered = _filtered_of(records)
        self.max_filtered = int(filtered.max(initial=0))
        self.max_pixels = int((records["width"].astype(np.int64) * records["height"]).max(initial=0))
        self.workspace_bytes = int(max(status_bytes(len(self)),
                                       (records["ws_offset"] + filtered)[filtered > 0].max(initial=0)))

    def __len__(self) -> int:
        return int(self.records.shape[0])

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def out_bytes(self) -> int:
        s = self.sizes.to(torch.int64)
        return int((s[:, 0] * s[:, 1]).sum()) * 3

    @property
    def fallbacks(self) -> int:
        return int((self.records["kind"] == KIND_RAW).sum())

    def pin_memory(self) -> "PngBatch":
        return PngBatch(self.data.pin_memory(), self.records, self.sizes)

    def to(self, *args, **kwargs) -> "PngBatch":
        data = self.data.to(*args, **kwargs)
        if data.dtype != torch.uint8:
            raise TypeError("a PngBatch stays uint8")
        return self if data is self.data else PngBatch(data, self.records, self.sizes)


def _pack(entries: Sequence) -> PngBatch:
    """``entries``: per image ``(stream, header, palette)`` -- the concatenated ``IDAT`` payloads, a ``PngHeader`` for
    the geometry (used with these bytes whatever they hold: the device checks them) and the ``PLTE`` bytes or ``None``
    -- or ``(pixels, None, None)`` with ``pixels`` an (H, W, 3) uint8 array."""
    B = len(entries)
    if B > MAX_BATCH:
        raise ValueError(f"a batch holds at most {MAX_BATCH} images (got {B})")
    rec = np.zeros(B, dtype=RECORD_DTYPE)
    chunks, at = [], 0

    def put(arr: np.ndarray, align: int) -> int:
        nonlocal at
        gap = -at % align
        if gap:
            chunks.append(np.zeros(gap, dtype=np.uint8))
        start = at + gap
        chunks.append(arr)
        at = start + arr.size
        return start

    sizes = np.zeros((B, 2), dtype=np.int32)
    out_at, ws_at = 0, status_bytes(B)
    for i, (payload, header, palette) in enumerate(entries):
        r = rec[i]
        if header is None:
            pixels = np.ascontiguousarray(payload)
            if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 3 or pixels.size == 0:
                raise ValueError(f"the fallback of image {i} must return an (H, W, 3) uint8 array (got "
                                 f"{pixels.dtype} {pixels.shape})")
            if max(pixels.shape[:2]) > MAX_SIDE:
                raise ValueError(f"image {i} is {pixels.shape[1]} x {pixels.shape[0]}: sides up to {MAX_SIDE} are taken")
            r["kind"], r["height"], r["width"], r["color_type"] = KIND_RAW, pixels.shape[0], pixels.shape[1], 2
            r["src_offset"], r["src_len"] = put(pixels.reshape(-1), 1), pixels.size
        else:
            stream = np.frombuffer(payload, dtype=np.uint8)
            r["kind"], r["height"], r["width"], r["color_type"] = KIND_STREAM, header.height, header.width, header.color_type
            r["src_offset"], r["src_len"] = put(stream, 1), stream.size
            if header.color_type == 3:
                table = np.zeros(768, dtype=np.uint8)
                if palette:
                    table[:min(len(palette), 768)] = np.frombuffer(palette, dtype=np.uint8)[:768]
                r["plte_offset"] = put(table, 1)
            ws_at += -ws_at % 16
            r["ws_offset"] = ws_at
            ws_at += header.filtered_bytes
        sizes[i] = r["height"], r["width"]
        r["out_offset"] = out_at
        out_at += 3 * int(r["height"]) * int(r["width"])
    put(np.zeros(-at % 16, dtype=np.uint8), 1)
    data = torch.from_numpy(np.concatenate(chunks)) if at else torch.empty(0, dtype=torch.uint8)
    return PngBatch(data, rec, torch.from_numpy(sizes))


def _idat(data: bytes, header: PngHeader) -> bytes:
    """The concatenated ``IDAT`` payloads: the one pass over the file's bytes the host makes."""
    return data[header.idat[0][0]:sum(header.idat[0])] if len(header.idat) == 1 else \
        b"".join(data[o:o + l] for o, l in header.idat)


def pack_pngs(files: Sequence, fallback: Optional[Callable] = None) -> PngBatch:
    """A ``PngBatch`` of a list of files' bytes.  A file the device does not decode (``parse_png`` gives the reason)
    goes through ``fallback``, a function from bytes to an (H, W, 3) RGB uint8 array (default:
    ``basd_amd.jpeg.pillow_fallback`` where Pillow is importable); its pixels travel in the same buffer.  Without a
    fallback such a file raises ``UnsupportedPng``."""
    if fallback is None:
        fallback = _default_fallback()
    entries = []
    for i, data in enumerate(files):
        if not isinstance(data, (bytes, bytearray, memoryview)):
            raise TypeError(f"image {i} must be the bytes of a file (got {type(data).__name__})")
        data = bytes(data)
        header = parse_png(data)
        if header.reason is None:
            entries.append((_idat(data, header), header, None if header.plte is None else
                            data[header.plte[0]:sum(header.plte)]))
        elif fallback is None:
            raise UnsupportedPng(i, header.reason)
        else:
            entries.append((fallback(data), None, None))
    return _pack(entries)


def collate_png(samples: Sequence, fallback: Optional[Callable] = None) -> dict:
    """``collate_fn`` of a loader that does not decode (``datasets.Image(decode=False)``: a sample's ``"image"`` is the
    file's bytes, or a dict with them under ``"bytes"``): ``{"images": PngBatch, ...}`` with every other entry collated
    as ``torch.utils.data.default_collate`` does."""
    from torch.utils.data import default_collate
    samples = list(samples)
    files = []
    for s in samples:
        if "image" not in s:
            raise KeyError(f"a sample needs an 'image' entry (got {sorted(s)})")
        image = s["image"]
        if isinstance(image, dict):
            if image.get("bytes") is None:
                raise KeyError(f"an 'image' dict needs its 'bytes' (got {sorted(image)})")
            image = image["bytes"]
        files.append(image)
    batch = {"images": pack_pngs(files, fallback)}
    if samples:
        rest = [{k: v for k, v in s.items() if k != "image"} for s in samples]
        if rest[0]:
            batch.update(default_collate(rest))
    return batch


# ----------------------------------------------------------------------------------------------------------------
# the launches
# ----------------------------------------------------------------------------------------------------------------
class PngDecoder:
    """``PngDecoder(device)(png_batch) -> RaggedBatch`` of three channels on the device.  ``png_batch.data`` lives on
    the device (one upload); the record table goes up with one non-blocking copy (``_launch.RecordTable``); then two
    launches on the current stream, no wait for the device.  ``workspace`` (the status area, then the filtered scanlines
    of every stream) grows to the largest batch seen, is never cleared, and is handed back through ``_launch.retire``
    when it is replaced, so the decoder may run under a ``DevicePrefetcher`` as ``JpegDecoder`` does.  ``status()`` reads
    the batch status word back (0: every image decoded; bit ``code - 1`` of ``STATUS_NAMES`` otherwise),
    ``image_status()`` the last batch's per-image words; both wait for the device."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        self._records = RecordTable(RECORD_DTYPE)
        self.workspace: Optional[torch.Tensor] = None
        self.used_bytes = 0
        self._last = 0

    def status(self) -> int:
        return self._records.status()

    def image_status(self) -> torch.Tensor:
        if self.workspace is None or not self._last:
            return torch.zeros(0, dtype=torch.int32)
        return self.workspace[:4 * self._last].view(torch.int32).cpu()

    def __call__(self, batch: PngBatch) -> RaggedBatch:
        if not isinstance(batch, PngBatch):
            raise TypeError(f"batch must be a PngBatch (got {type(batch).__name__}); pack_pngs makes one")
        if not lives_on(self.device, batch.device):
            raise ValueError(f"the streams live on {batch.device}, the decoder on {self.device}")
        B = len(batch)
        rec = batch.records
        for name, limit in (("width", MAX_SIDE), ("height", MAX_SIDE)):
            if B and (int(rec[name].min()) < 1 or int(rec[name].max()) > limit):
                i = int(np.flatnonzero((rec[name] < 1) | (rec[name] > limit))[0])
                raise ValueError(f"image {i} has {name} {int(rec[name][i])} (1 .. {limit} are decoded)")
        require_gpu(batch.data, f"the {B} streams")
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=batch.device)
        ragged = RaggedBatch(out, batch.sizes, 3)
        self._last = B
        if B == 0:
            return ragged
        need = batch.workspace_bytes
        if self.workspace is None or self.workspace.numel() < need:
            retire(self.workspace)
            self.workspace = torch.empty(need, dtype=torch.uint8, device=batch.device)
        self.used_bytes = need
        self._records.stage(B, batch.device)[...] = rec
        _lib.call("basd_png_decode", batch.data.data_ptr(), batch.data.numel(), out.data_ptr(), out.numel(), B,
                  self._records.upload(), self.workspace.data_ptr(), self.workspace.numel(), self._records.status_ptr,
                  batch.max_filtered, batch.max_pixels, raw_stream(batch.device.index))
        return ragged


# ----------------------------------------------------------------------------------------------------------------
# the specification in plain Python (tests and the goldens script; the product path does not use it)
# ----------------------------------------------------------------------------------------------------------------
_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class _Bits:
    """LSB-first bits of ``data[2:]``; past the end zeros, and ``over`` once one of them was taken."""

    def __init__(self, data: bytes) -> None:
        self.data, self.end, self.over = data, 8 * len(data), False
        self.pos = min(16, self.end)

    def peek(self, n: int) -> int:                     # n <= 16; the slice past the end is short: zeros
        at = self.pos >> 3
        return (int.from_bytes(self.data[at:at + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n)
        if self.pos + n > self.end:
            self.over, self.pos = True, self.end
        else:
            self.pos += n
        return v


def _code(lengths, codes: bool):
    """``{(length, code): symbol}`` of a list of code lengths, or ``None`` where they are no code."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    left, longest = 1, 0
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            return None
        if count[l]:
            longest = l
    if left > 0 and (codes or longest > 1):
        return None
    table, code, count[0] = {}, 0, 0
    nxt = [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits: _Bits, table: dict) -> int:
    ahead, code = bits.peek(15), 0
    for l in range(1, 16):
        code = (code << 1) | ((ahead >> (l - 1)) & 1)
        s = table.get((l, code))
        if s is not None:
            bits.take(l)
            return s
    bits.take(15)
    return -1


_FIXED = None


def inflate_reference(stream, expected_len: int):
    """``(bytes, status)`` of the concatenated ``IDAT`` payloads (zlib header first) by the text of
    ``include/basd_hip.h``: the ``expected_len`` inflated bytes and 0, or ``b""`` and the ``BASD_PNG_*`` code (2 .. 8,
    10) of the first thing wrong, checks in the header's order."""
    global _FIXED
    data = bytes(stream)
    bits, out, n = _Bits(data), bytearray(), expected_len
    final = 0
    while not final:
        final, kind = bits.take(1), bits.take(2)
        if bits.over:
            return b"", 7
        if kind == 3:
            return b"", 2
        if kind == 0:
            bits.take(-bits.pos % 8)
            length, inverse = bits.take(16), bits.take(16)
            if bits.over:
                return b"", 7
            if length ^ 0xFFFF != inverse:
                return b"", 3
            at = bits.pos >> 3
            if length > n - len(out):
                return b"", 8
            if length > len(data) - at:
                return b"", 7
            out += data[at:at + length]
            bits.pos += 8 * length
            continue
        if kind == 1:
            if _FIXED is None:
                _FIXED = (_code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _code([5] * 32, False))
            lit, dist = _FIXED
        else:
            nlit, ndist, ncode = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            if bits.over:
                return b"", 7
            if nlit > 286 or ndist > 30:
                return b"", 4
            clens = [0] * 19
            for i in range(ncode):
                clens[_ORDER[i]] = bits.take(3)
            if bits.over:
                return b"", 7
            clen = _code(clens, True)
            if clen is None:
                return b"", 4
            lengths, total = [], nlit + ndist
            while len(lengths) < total:
                s = _symbol(bits, clen)
                if bits.over:
                    return b"", 7
                if s < 0:
                    return b"", 5
                if s < 16:
                    lengths.append(s)
                    continue
                if s == 16:
                    if not lengths:
                        return b"", 4
                    value, repeat = lengths[-1], 3 + bits.take(2)
                elif s == 17:
                    value, repeat = 0, 3 + bits.take(3)
                else:
                    value, repeat = 0, 11 + bits.take(7)
                if bits.over:
                    return b"", 7
                if repeat > total - len(lengths):
                    return b"", 4
                lengths += [value] * repeat
            if lengths[256] == 0:
                return b"", 4
            lit, dist = _code(lengths[:nlit], False), _code(lengths[nlit:], False)
            if lit is None or dist is None:
                return b"", 4
        while True:
            s = _symbol(bits, lit)
            if bits.over:
                return b"", 7
            if s < 0:
                return b"", 5
            if s < 256:
                if len(out) >= n:
                    return b"", 8
                out.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                return b"", 5
            i = s - 257
            if i < 8:
                length = 3 + i
            elif i == 28:
                length = 258
            else:
                e = i // 4 - 1
                length = 3 + ((4 + i % 4) << e) + bits.take(e)
            d = _symbol(bits, dist)
            if bits.over:
                return b"", 7
            if d < 0 or d > 29:
                return b"", 5
            if d < 4:
                distance = 1 + d
            else:
                e = d // 2 - 1
                distance = 1 + ((2 + d % 2) << e) + bits.take(e)
            if bits.over:
                return b"", 7
            if distance > len(out):
                return b"", 6
            if length > n - len(out):
                return b"", 8
            start = len(out) - distance
            for j in range(length):
                out.append(out[start + j % distance])
    if len(out) != n:
        return b"", 8
    at = (bits.pos + 7) >> 3
    if 4 > len(data) - at:
        return b"", 7
    a = (1 + sum(out)) % 65521
    b = (n + sum((n - i) * v for i, v in enumerate(out))) % 65521
    if int.from_bytes(data[at:at + 4], "big") != (b << 16 | a):
        return b"", 10
    return bytes(out), 0


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def decode_stream(stream, width: int, height: int, color_type: int, palette=None):
    """``(rgb, status)`` of a file's concatenated ``IDAT`` payloads and geometry: the (H, W, 3) uint8 image and 0, or
    zeros and the ``BASD_PNG_*`` code, as the two launches report it."""
    bpp = BPP[color_type]
    stride = width * bpp + 1
    zeros = np.zeros((height, width, 3), dtype=np.uint8)
    raw, status = inflate_reference(stream, height * stride)
    if status:
        return zeros, status
    if any(raw[y * stride] > 4 for y in range(height)):
        return zeros, 9
    rows, prev = [], bytearray(width * bpp)
    for y in range(height):
        ft, line = raw[y * stride], bytearray(raw[y * stride + 1:(y + 1) * stride])
        for i in range(len(line)):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = 0 if ft == 0 else a if ft == 1 else b if ft == 2 else (a + b) >> 1 if ft == 3 else _paeth(a, b, c)
            line[i] = (line[i] + pred) & 255
        rows.append(line)
        prev = line
    px = np.frombuffer(b"".join(bytes(r) for r in rows), dtype=np.uint8).reshape(height, width, bpp)
    if color_type == 3:
        table = np.zeros(768, dtype=np.uint8)
        if palette:
            table[:min(len(palette), 768)] = np.frombuffer(bytes(palette), dtype=np.uint8)[:768]
        return table.reshape(256, 3)[px[:, :, 0]], 0
    if color_type in (0, 4):
        return np.repeat(px[:, :, :1], 3, axis=2), 0
    return np.ascontiguousarray(px[:, :, :3]), 0


def decode_reference(data) -> np.ndarray:
    """The specification of ``include/basd_hip.h`` in plain Python, by way of ``inflate_reference``: the (H, W, 3)
    uint8 RGB image of a file in the device's scope; ``ValueError`` for a file outside it or a bad one."""
    data = bytes(data)
    h = parse_png(data)
    if h.reason is not None:
        raise ValueError(f"not in the device's scope: {h.reason}")
    rgb, status = decode_stream(_idat(data, h), h.width, h.height, h.color_type,
                                None if h.plte is None else data[h.plte[0]:sum(h.plte)])
    if status:
        raise ValueError(f"a bad stream: {STATUS_NAMES[status]}")
    return rgb
