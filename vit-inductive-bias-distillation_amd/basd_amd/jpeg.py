"""The decode of the reference's loader -- ``Image.open(...).convert("RGB")`` in its workers -- on the device: the loader
ships file bytes, ``collate_jpeg`` packs the streams of a batch into one uint8 buffer, that buffer is uploaded once, and
three launches of ``basd_jpeg_decode`` (``csrc/jpeg.hip``) write the decoded images as the ``RaggedBatch`` of three
channels ``ResizeCrop`` takes.  ``JpegDecoder(device, entropy="parallel")`` takes ``basd_jpeg_decode_parallel`` instead,
whose first launch decodes inside a segment with a workgroup's lanes: the same bytes, opt-in.

``parse_jpeg`` reads a stream's header on the host and says whether the device decodes it (baseline, 8 bits, 1 or 3
components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, YCbCr by libjpeg's rules: the scope is spelled out in
``include/basd_hip.h``, which also holds the specification); every other file goes through ``pack_jpegs``'s
``fallback`` (default: Pillow, where it is importable) and travels as a "raw" record of decoded pixels in the same
buffer.  ``JpegDecoder`` builds nothing per image on the host: the record table is made by ``pack_jpegs`` in the collate
worker, vectorised search for the restart markers included.

Opt-in, ``progressive=True`` in ``parse_jpeg`` / ``pack_jpegs`` / ``collate_jpeg`` / ``decode_reference``: a progressive
file (SOF2) with a complete progression travels as its compressed bytes too, in a record of kind ``KIND_PROGRESSIVE``
with a table of its scans behind the stream, and ``basd_jpeg_decode_progressive`` decodes it with one more launch ahead of
the same three.  Without the keyword every function here returns what it returned before it existed.

The decode is Pillow's (libjpeg-turbo's integer path), byte for byte: ``decode_reference`` restates the specification in
numpy and is held to Pillow, the kernels are held to it, in ``tests/test_jpeg_decode.py``.  There is no CPU fallback of
the kernels.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._launch import RecordTable, lives_on, raw_stream, require_gpu, retire
from .resize import RaggedBatch

__all__ = ["JpegHeader", "parse_jpeg", "UnsupportedJpeg", "JpegBatch", "pack_jpegs", "collate_jpeg", "JpegDecoder",
           "decode_reference", "pillow_fallback", "RECORD_DTYPE", "SCAN_DTYPE", "JpegScan", "MAX_SIDE", "MAX_BATCH",
           "MAX_SCANS", "STATUS_NAMES", "SUB_BYTES_MIN", "SUB_BYTES_MAX"]

MAX_SIDE = 16384                    # BASD_JPEG_MAX_SIDE
MAX_BATCH = 65535                   # BASD_JPEG_MAX_BATCH
KIND_STREAM, KIND_RAW, KIND_PROGRESSIVE = 0, 1, 2   # BASD_JPEG_KIND_*
MAX_SCANS = 64                      # BASD_JPEG_MAX_SCANS
SUB_BYTES_MIN, SUB_BYTES_MAX = 8, 1024   # BASD_JPEG_SUB_BYTES_*
STATUS_NAMES = {0: "decoded", 1: "bad record", 2: "bad Huffman table", 3: "truncated", 4: "invalid Huffman code",
                5: "missing or wrong restart marker", 6: "coefficient index past 63", 7: "DC value out of range"}

# BasdJpegRecord: 128 bytes
RECORD_DTYPE = np.dtype([("src_offset", "<i8"), ("out_offset", "<i8"), ("coef_offset", "<i8"), ("plane_offset", "<i8"),
                         ("seg_offset", "<i8"), ("src_len", "<i4"), ("kind", "<i4"), ("width", "<i4"), ("height", "<i4"),
                         ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("restart", "<i4"), ("n_seg", "<i4"),
                         ("quant", "<i4", (3,)), ("dc", "<i4", (3,)), ("ac", "<i4", (3,)), ("pad", "<i4", (4,))])
assert RECORD_DTYPE.itemsize == 128
# BasdJpegScan: 64 bytes, one per scan of a progressive record (whose ``pad`` holds the scan count, the offset of the scan
# table from ``src_offset`` and the largest segment count of a scan)
SCAN_DTYPE = np.dtype([("seg_offset", "<i4"), ("n_seg", "<i4"), ("data_end", "<i4"), ("restart", "<i4"), ("ncomp", "<i4"),
                       ("comp", "<i4"), ("ss", "<i4"), ("se", "<i4"), ("ah", "<i4"), ("al", "<i4"), ("level", "<i4"),
                       ("dc", "<i4", (3,)), ("ac", "<i4"), ("pad", "<i4")])
assert SCAN_DTYPE.itemsize == 64

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                    7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                    39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)


class UnsupportedJpeg(ValueError):
    """A file the device does not decode and no fallback took: ``index`` in its batch, ``reason``."""

    def __init__(self, index: int, reason: str) -> None:
        super().__init__(f"image {index} is not decoded on the device ({reason}) and there is no fallback for it")
        self.index = index
        self.reason = reason


# ----------------------------------------------------------------------------------------------------------------
# the header
# ----------------------------------------------------------------------------------------------------------------
class JpegScan(NamedTuple):
    """One scan of a progressive stream.  ``comps``: the frame indices of its components (all of them, in frame order, or
    one); ``dc`` per frame component the offset of the DC table in force (0 where the scan reads none), ``ac`` that of
    the one AC table; ``restart`` the interval in force, in scan units (MCUs of an interleaved scan, blocks of a
    one-component scan); ``segments`` as in ``JpegHeader``, ``data_end`` the offset of the marker behind the scan's data
    (the stream's length where there is none); ``level``: 0, or one more than the largest level of an earlier scan that
    shares a component and overlaps in ``ss .. se`` (scans of one level touch disjoint coefficients)."""
    comps: tuple
    ss: int
    se: int
    ah: int
    al: int
    dc: tuple
    ac: int
    restart: int
    segments: tuple
    data_end: int
    level: int


class JpegHeader(NamedTuple):
    """What ``parse_jpeg`` found.  ``reason``: ``None`` where the device decodes the stream, else why not (the other
    fields then hold what was read up to that point).  Offsets count from the stream's first byte: ``quant`` / ``dc`` /
    ``ac`` per component the 64 bytes of its DQT table and the 16 counts of its DHT tables; ``scan_offset`` the first
    entropy-coded byte; ``segments`` the first byte of every entropy-coded segment (``scan_offset``, then the byte after
    each RSTn marker).  ``scans``: empty for a baseline stream; for a progressive one (``parse_jpeg(...,
    progressive=True)``) its ``JpegScan`` rows in stream order, with ``dc``, ``ac``, ``restart`` and ``segments`` of the
    header left empty (every scan has its own)."""
    reason: Optional[str]
    width: int = 0
    height: int = 0
    ncomp: int = 0
    hs: int = 1
    vs: int = 1
    restart: int = 0
    quant: tuple = ()
    dc: tuple = ()
    ac: tuple = ()
    scan_offset: int = 0
    segments: tuple = ()
    scans: tuple = ()

    @property
    def blocks(self) -> int:
        hs, vs = (1, 1) if self.ncomp == 1 else (self.hs, self.vs)
        mcus = -(-self.width // (8 * hs)) * -(-self.height // (8 * vs))
        return mcus * (1 if self.ncomp == 1 else hs * vs + 2)


_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)",
              0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
              0xCA: "arithmetic coding, progressive (SOF10)", 0xCB: "arithmetic coding, lossless (SOF11)",
              0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def _read_dht(buf: np.ndarray, body: int, stop: int, dc: dict, ac: dict) -> Optional[str]:
    """The tables of one DHT segment into ``dc`` / ``ac`` (id -> offset of the 16 counts); a reason where one is bad."""
    p = body
    while p < stop:
        if p + 17 > stop:
            return "a truncated Huffman table"
        tc, th = int(buf[p]) >> 4, int(buf[p]) & 15
        total = int(buf[p + 1:p + 17].sum())
        if tc > 1 or th > 3 or total > 256 or p + 17 + total > stop:
            return f"a bad Huffman table (class {tc}, id {th}, {total} values)"
        code = 0
        for l in range(1, 17):
            code += int(buf[p + l])
            if code > 1 << l:
                return f"a Huffman table that is no prefix code (class {tc}, id {th})"
            code <<= 1
        (ac if tc else dc)[th] = p + 1
        p += 17 + total
    return None


def _progressive_scans(buf: np.ndarray, base: dict, comps: list, quant: dict, dc: dict, ac: dict, restart: int,
                       at: int) -> JpegHeader:
    """The scans of a progressive stream whose frame is in scope; ``at``: the length field of its first SOS.  The scope
    and the rules of the progression are those of ``include/basd_hip.h``."""
    n, ncomp = buf.size, len(comps)
    bad = lambda reason: JpegHeader(reason, **base)                    # noqa: E731
    ids = [c[0] for c in comps]
    if len(set(ids)) != ncomp:
        return bad(f"component ids {tuple(ids)} (two components with one id)")
    for c in range(ncomp):
        if comps[c][3] not in quant:
            return bad(f"a table that is not defined ahead of the first scan (component {c}: quantisation {comps[c][3]})")
    # markers behind the first SOS: FF followed by anything but 00 (a stuffed FF) and FF (fill)
    ff = np.flatnonzero(buf[at:n - 1] == 0xFF) + at
    follow = buf[ff + 1]
    rst = ff[(follow & 0xF8) == 0xD0]
    other = ff[(follow != 0) & (follow != 0xFF) & ((follow & 0xF8) != 0xD0)]
    last_al = [[None] * 64 for _ in range(ncomp)]                      # per coefficient: not coded yet, or its last Al
    scans = []
    while True:                                                        # `at`: the length field of an SOS
        length = (int(buf[at]) << 8) | int(buf[at + 1])
        body, stop = at + 2, at + length
        ns = int(buf[body]) if length >= 3 else -1
        if not 1 <= ns <= 4 or length != 6 + 2 * ns:
            return bad("a truncated header")
        if len(scans) == MAX_SCANS:
            return bad(f"more than {MAX_SCANS} scans")
        which, tables = [], []
        for i in range(ns):
            cid = int(buf[body + 1 + 2 * i])
            if cid not in ids or ids.index(cid) in which:
                return bad(f"a scan of component id {cid}, which the frame does not have or the scan names twice")
            which.append(ids.index(cid))
            tables.append(int(buf[body + 2 + 2 * i]))
        ss, se, ahl = (int(v) for v in buf[body + 1 + 2 * ns:body + 4 + 2 * ns])
        ah, al = ahl >> 4, ahl & 15
        if ss == 0:
            if se != 0:
                return bad(f"a scan of coefficients 0..{se} (DC and AC coefficients in one progressive scan)")
            if ns != 1 and which != list(range(ncomp)):
                return bad(f"a DC scan of {ns} of the {ncomp} components" if ns != ncomp else
                           "a scan whose components are not in the frame's order")
        else:
            if not ss <= se <= 63:
                return bad(f"a scan of coefficients {ss}..{se}")
            if ns != 1:
                return bad(f"an AC scan of {ns} components")
            if last_al[which[0]][0] is None:
                return bad(f"an AC scan ahead of the first DC scan of its component ({which[0]})")
        if al > 13:
            return bad(f"a scan with Al {al} (above 13)")
        for c in which:
            seen = set(last_al[c][ss:se + 1])
            if ah == 0 and seen != {None}:
                return bad(f"a first scan (Ah 0) of coefficients {ss}..{se} of component {c}, some of which were coded "
                           "before")
            if ah != 0 and (seen != {ah} or al != ah - 1):
                was = ", ".join("none" if v is None else str(v) for v in sorted(seen, key=lambda v: -1 if v is None else v))
                return bad(f"a refinement scan with Ah {ah}, Al {al} of coefficients {ss}..{se} of component {c} whose "
                           f"previous Al is {was} (Ah must equal it, and Al be Ah - 1)")
        dc_of, ac_of = [0, 0, 0], 0
        for c, t in zip(which, tables):
            td, ta = t >> 4, t & 15
            if ss == 0 and ah == 0:
                if td not in dc:
                    return bad(f"a table that is not defined (component {c}: DC {td})")
                dc_of[c] = dc[td]
            if ss > 0:
                if ta not in ac:
                    return bad(f"a table that is not defined (component {c}: AC {ta})")
                ac_of = ac[ta]
        level = 1 + max((s.level for s in scans if set(s.comps) & set(which) and s.ss <= se and ss <= s.se), default=-1)
        for c in which:
            last_al[c][ss:se + 1] = [al] * (se + 1 - ss)
        first = int(np.searchsorted(other, stop))
        end = int(other[first]) if first < other.size else n           # no marker behind the data: libjpeg supplies EOI
        segments = [stop]
        if restart:
            lo, hi = np.searchsorted(rst, [stop, end])
            segments += (rst[lo:hi] + 2).tolist()
        scans.append(JpegScan(tuple(which), ss, se, ah, al, tuple(dc_of), ac_of, restart, tuple(segments), end, level))
        # ---- between scans: DHT, DRI, COM and APPn
        at = end
        while True:
            while at < n and buf[at] != 0xFF:
                at += 1
            while at < n and buf[at] == 0xFF:
                at += 1
            marker = int(buf[at]) if at < n else 0xD9
            at += 1
            if marker in (0xD9, 0xDA):
                break
            if at + 2 > n:
                return bad("a truncated header")
            length = (int(buf[at]) << 8) | int(buf[at + 1])
            if length < 2 or at + length > n:
                return bad("a truncated header")
            body, stop = at + 2, at + length
            if marker == 0xC4:
                why = _read_dht(buf, body, stop, dc, ac)
                if why:
                    return bad(why)
            elif marker == 0xDD:
                if length != 4:
                    return bad("a truncated header")
                restart = (int(buf[body]) << 8) | int(buf[body + 1])
            elif marker == 0xEE and length >= 7 and bytes(buf[body:body + 5]) == b"Adobe":
                return bad("an Adobe APP14 segment (its transform flag picks the colour space)")
            elif marker == 0xDB:
                return bad("a quantisation table between scans (DQT behind the first SOS)")
            elif marker != 0xFE and not 0xE0 <= marker <= 0xEF:
                return bad(f"a marker ff{marker:02x} between scans")
            at = stop
        if marker == 0xD9:
            break
        if at + 2 > n or at + ((int(buf[at]) << 8) | int(buf[at + 1])) > n:
            return bad("a truncated header")
    if any(v != 0 for row in last_al for v in row):
        return bad("an incomplete progression (Pillow smooths it): at EOI some coefficient has not been coded down to "
                   "its last bit")
    return JpegHeader(None, quant=tuple(quant[c[3]] for c in comps), scan_offset=scans[0].segments[0],
                      scans=tuple(scans), **base)


def parse_jpeg(data, progressive: bool = False) -> JpegHeader:
    """The header of a file's bytes.  Never raises on malformed input: what the device does not decode has ``reason``
    set (a PNG: "not a JPEG stream ..."; progressive, CMYK, an Adobe segment, 16-bit tables, ...: named).
    ``progressive=True``: a progressive stream (SOF2) in the device's scope has ``reason None`` and its ``scans``; one
    outside it (an incomplete progression, a DQT between scans, ...) its own reason.  Baseline streams parse alike
    either way."""
    buf =np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
    n = buf.size
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        return JpegHeader(f"not a JPEG stream (it starts with {bytes(buf[:2]).hex() or 'nothing'}, not ffd8)")
    if n > (1 << 31) - 17:
        return JpegHeader(f"a stream of {n} bytes (the limit is {(1 << 31) - 17})")
    quant, dc, ac = {}, {}, {}
    jfif = adobe = sof2 = False
    restart = 0
    frame = None                      # (width, height, [(id, h, v, tq)])
    at = 2
    while True:
        while at < n and buf[at] != 0xFF:                 # libjpeg skips garbage between segments with a warning
            at += 1
        while at < n and buf[at] == 0xFF:
            at += 1
        if at >= n:
            return JpegHeader("no scan (the header ends without SOS)")
        marker = int(buf[at])
        at += 1
        if marker in (0x01, 0xD8) or 0xD0 <= marker <= 0xD7:
            continue
        if marker == 0xD9:
            return JpegHeader("no scan (EOI before SOS)")
        if at + 2 > n:
            return JpegHeader("a truncated header")
        length = (int(buf[at]) << 8) | int(buf[at + 1])
        if length < 2 or at + length > n:
            return JpegHeader("a truncated header")
        body, stop = at + 2, at + length
        if marker in _SOF_NAMES and not (progressive and marker == 0xC2):
            return JpegHeader(f"not baseline: {_SOF_NAMES[marker]}")
        if marker in (0xC0, 0xC2):
            sof2 = marker == 0xC2
            if frame is not None:
                return JpegHeader("two frame headers")
            if length < 8:
                return JpegHeader("a truncated header")
            precision, height, width = int(buf[body]), (int(buf[body + 1]) << 8) | int(buf[body + 2]), \
                (int(buf[body + 3]) << 8) | int(buf[body + 4])
            ncomp = int(buf[body + 5])
            if precision != 8:
                return JpegHeader(f"{precision}-bit samples")
            if length != 8 + 3 * ncomp:
                return JpegHeader("a truncated header")
            comps = [(int(buf[body + 6 + 3 * c]), int(buf[body + 7 + 3 * c]) >> 4, int(buf[body + 7 + 3 * c]) & 15,
                      int(buf[body + 8 + 3 * c])) for c in range(ncomp)]
            frame = (width, height, comps)
        elif marker == 0xC4:
            why = _read_dht(buf, body, stop, dc, ac)
            if why:
                return JpegHeader(why)
        elif marker == 0xDB:
            p = body
            while p < stop:
                pq, tq = int(buf[p]) >> 4, int(buf[p]) & 15
                if pq != 0:
                    return JpegHeader(f"a 16-bit quantisation table (id {tq})")
                if tq > 3 or p + 65 > stop:
                    return JpegHeader(f"a bad quantisation table (id {tq})")
                quant[tq] = p + 1
                p += 65
        elif marker == 0xDD:
            if length != 4:
                return JpegHeader("a truncated header")
            restart = (int(buf[body]) << 8) | int(buf[body + 1])
        elif marker == 0xE0:
            if length >= 7 and bytes(buf[body:body + 5]) == b"JFIF\0":
                jfif = True
        elif marker == 0xEE:
            if length >= 7 and bytes(buf[body:body + 5]) == b"Adobe":
                adobe = True
        elif marker == 0xDC:
            return JpegHeader("a DNL segment")
        elif marker == 0xDA:
            break
        at = stop
    # ---- the scan header
    if frame is None:
        return JpegHeader("a scan before the frame header")
    width, height, comps = frame
    ncomp = len(comps)
    base = dict(width=width, height=height, ncomp=ncomp, restart=restart)
    if ncomp not in (1, 3):
        return JpegHeader(f"{ncomp} components" + (" (CMYK / YCCK)" if ncomp == 4 else ""), **base)
    if adobe:
        return JpegHeader("an Adobe APP14 segment (its transform flag picks the colour space)", **base)
    if height == 0:
        return JpegHeader("height 0 (the height comes in a DNL segment)", **base)
    if width == 0:
        return JpegHeader("width 0", **base)
    if width > MAX_SIDE or height > MAX_SIDE:
        return JpegHeader(f"{width} x {height} pixels (the device decodes sides up to {MAX_SIDE})", **base)
    hs, vs = (comps[0][1], comps[0][2]) if ncomp == 3 else (1, 1)
    if ncomp == 3:
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:]):
            return JpegHeader("sampling factors " + " ".join(f"{c[1]}x{c[2]}" for c in comps)
                              + " (decoded: 1x1, 2x1 or 2x2 luma with 1x1 chroma)", **base)
        if not jfif and tuple(c[0] for c in comps) != (1, 2, 3):
            return JpegHeader(f"component ids {tuple(c[0] for c in comps)} without a JFIF segment (libjpeg would not "
                              "read them as YCbCr)", **base)
    base.update(hs=hs, vs=vs)
    if sof2:
        return _progressive_scans(buf, base, comps, quant, dc, ac, restart, at)
    ns = int(buf[body]) if length >= 3 else -1
    if ns != ncomp:
        return JpegHeader(f"a scan of {ns} of the {ncomp} components (several scans)", **base)
    if length != 6 + 2 * ns:
        return JpegHeader("a truncated header", **base)
    q_of, dc_of, ac_of = [], [], []
    for c in range(ncomp):
        cid, tables = int(buf[body + 1 + 2 * c]), int(buf[body + 2 + 2 * c])
        if cid != comps[c][0]:
            return JpegHeader("a scan whose components are not in the frame's order", **base)
        td, ta, tq = tables >> 4, tables & 15, comps[c][3]
        if td not in dc or ta not in ac or tq not in quant:
            return JpegHeader(f"a table that is not defined (component {c}: DC {td}, AC {ta}, quantisation {tq})", **base)
        q_of.append(quant[tq]), dc_of.append(dc[td]), ac_of.append(ac[ta])
    ss, se, ahl = (int(v) for v in buf[body + 1 + 2 * ns:body + 4 + 2 * ns])
    if (ss, se, ahl) != (0, 63, 0):
        return JpegHeader(f"a scan of coefficients {ss}..{se} with approximation {ahl:#04x} (not a baseline scan)", **base)
    scan = stop
    # ---- the entropy-coded data: markers are FF followed by anything but 00 (a stuffed FF) and FF (fill)
    ff = np.flatnonzero(buf[scan:n - 1] == 0xFF) + scan
    follow = buf[ff + 1]
    rst = ff[(follow & 0xF8) == 0xD0]
    other = ff[(follow != 0) & (follow != 0xFF) & ((follow & 0xF8) != 0xD0)]
    if other.size:
        end = int(other[0])
        if buf[end + 1] != 0xD9:
            return JpegHeader(f"a marker ff{int(buf[end + 1]):02x} after the first scan (several scans, or tables between "
                              "them)", **base)
        rst = rst[rst < end]
    segments = [scan]
    if restart:
        segments += (rst + 2).tolist()
    return JpegHeader(None, quant=tuple(q_of), dc=tuple(dc_of), ac=tuple(ac_of), scan_offset=scan,
                      segments=tuple(segments), **base)


# ----------------------------------------------------------------------------------------------------------------
# batches of streams
# ----------------------------------------------------------------------------------------------------------------
def status_bytes(batch: int) -> int:
    """``basd_jpeg_status_bytes``: the per-image status words at the start of the workspace."""
    return (4 * batch + 127) & ~127


class JpegBatch:
    """``B`` files in one buffer: ``data`` a 1-D uint8 tensor (a multiple of 16 bytes) that holds the streams, the
    decoded pixels of the files the fallback took and the int32 tables of segment starts; ``records`` the ``B`` rows of
    ``RECORD_DTYPE`` (host); ``sizes`` a ``(B, 2)`` int32 CPU tensor of ``(height, width)``.  ``pin_memory()`` and
    ``to()`` act on ``data``, as a ``RaggedBatch``'s do.  ``workspace_bytes``: the workspace the batch uses (the status
    words, then 128 bytes of coefficients and 64 of samples per 8 x 8 block); ``max_blocks`` / ``max_pixels``: the
    largest image's."""

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
        # what sizes the workspace and the grids, once per batch and vectorised (the collate worker's share)
        blocks = _blocks_of(records)
        self.max_blocks = int(blocks.max(initial=0))
        self.max_pixels = int((records["width"].astype(np.int64) * records["height"]).max(initial=0))
        scanned = records["pad"][records["kind"] == KIND_PROGRESSIVE]
        self.max_scans, self.max_segments = int(scanned[:, 0].max(initial=0)), int(scanned[:, 2].max(initial=0))
        self.workspace_bytes = int(max(status_bytes(len(self)),
                                       (records["plane_offset"] + 64 * blocks)[blocks > 0].max(initial=0)))

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

    @property
    def progressive(self) -> int:
        """Records of progressive streams (``pack_jpegs(..., progressive=True)``): with one or more, the decoder issues
        one more launch."""
        return int((self.records["kind"] == KIND_PROGRESSIVE).sum())

    def pin_memory(self) -> "JpegBatch":
        return JpegBatch(self.data.pin_memory(), self.records, self.sizes)

    def to(self, *args, **kwargs) -> "JpegBatch":
        data = self.data.to(*args, **kwargs)
        if data.dtype != torch.uint8:
            raise TypeError("a JpegBatch stays uint8")
        return self if data is self.data else JpegBatch(data, self.records, self.sizes)


def _blocks_of(rec: np.ndarray) -> np.ndarray:
    """Per record the 8 x 8 blocks of its stream, baseline or progressive (int64; a raw record has none)."""
    gray = rec["ncomp"] == 1
    hs, vs = np.where(gray, 1, rec["hs"]).astype(np.int64), np.where(gray, 1, rec["vs"]).astype(np.int64)
    mcus = -(-rec["width"].astype(np.int64) // (8 * hs)) * -(-rec["height"].astype(np.int64) // (8 * vs))
    return np.where(rec["kind"] != KIND_RAW, mcus * np.where(gray, 1, hs * vs + 2), 0)


def pillow_fallback(data: bytes) -> np.ndarray:
    """``np.asarray(Image.open(...).convert("RGB"))``: the default ``fallback`` of ``pack_jpegs``."""
    import io

    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img.convert("RGB"))


def _default_fallback() -> Optional[Callable]:
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return None
    return pillow_fallback


def _pack(entries: Sequence) -> JpegBatch:
    """``entries``: per image ``(bytes, JpegHeader)`` (the header's offsets are used with these bytes, whatever their
    length: the device checks them) or ``(pixels, None)`` with ``pixels`` an (H, W, 3) uint8 array."""
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
    for i, (payload, header) in enumerate(entries):
        r = rec[i]
        if header is None:
            pixels = np.ascontiguousarray(payload)
            if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 3 or pixels.size == 0:
                raise ValueError(f"the fallback of image {i} must return an (H, W, 3) uint8 array (got "
                                 f"{pixels.dtype} {pixels.shape})")
            if max(pixels.shape[:2]) > MAX_SIDE:
                raise ValueError(f"image {i} is {pixels.shape[1]} x {pixels.shape[0]}: sides up to {MAX_SIDE} are taken")
            r["kind"], r["height"], r["width"] = KIND_RAW, pixels.shape[0], pixels.shape[1]
            r["src_offset"], r["src_len"] = put(pixels.reshape(-1), 1), pixels.size
            r["ncomp"], r["hs"], r["vs"], r["n_seg"] = 3, 1, 1, 1
        else:
            stream = np.frombuffer(payload, dtype=np.uint8)
            r["height"], r["width"] = header.height, header.width
            r["src_offset"], r["src_len"] = put(stream, 1), stream.size
            r["ncomp"], r["hs"], r["vs"] = header.ncomp, header.hs, header.vs
            r["quant"][:header.ncomp] = header.quant
            if header.scans:                                           # the scan table and the scans' segment tables
                r["kind"], r["n_seg"] = KIND_PROGRESSIVE, 1
                table = np.zeros(len(header.scans), dtype=SCAN_DTYPE)
                for row, scan in zip(table, header.scans):
                    row["seg_offset"] = put(np.asarray(scan.segments, dtype="<i4").view(np.uint8), 4) - r["src_offset"]
                    row["n_seg"], row["data_end"], row["restart"] = len(scan.segments), scan.data_end, scan.restart
                    row["ncomp"], row["comp"] = len(scan.comps), scan.comps[0]
                    row["ss"], row["se"], row["ah"], row["al"], row["level"] = scan.ss, scan.se, scan.ah, scan.al, scan.level
                    row["dc"], row["ac"] = scan.dc, scan.ac
                at_table = put(table.view(np.uint8), 8) - int(r["src_offset"])
                if at_table + table.nbytes >= 1 << 31:
                    raise ValueError(f"image {i}: its stream and segment tables take more than 2^31 bytes")
                r["pad"][:3] = len(header.scans), at_table, int(table["n_seg"].max())
            else:
                r["kind"], r["restart"] = KIND_STREAM, header.restart
                r["dc"][:header.ncomp], r["ac"][:header.ncomp] = header.dc, header.ac
                r["n_seg"] = len(header.segments)
                r["seg_offset"] = put(np.asarray(header.segments, dtype="<i4").view(np.uint8), 4)
            blocks = header.blocks
            r["coef_offset"], r["plane_offset"] = ws_at, ws_at + 128 * blocks
            ws_at += 192 * blocks
        sizes[i] = r["height"], r["width"]
        r["out_offset"] = out_at
        out_at += 3 * int(r["height"]) * int(r["width"])
    put(np.zeros(-at % 16, dtype=np.uint8), 1)
    data = torch.from_numpy(np.concatenate(chunks)) if at else torch.empty(0, dtype=torch.uint8)
    return JpegBatch(data, rec, torch.from_numpy(sizes))


def pack_jpegs(files: Sequence, fallback: Optional[Callable] = None, progressive: bool = False) -> JpegBatch:
    """A ``JpegBatch`` of a list of files' bytes.  A file the device does not decode (``parse_jpeg`` gives the reason)
    goes through ``fallback``, a function from bytes to an (H, W, 3) RGB uint8 array (default: Pillow's
    ``Image.open(...).convert("RGB")`` where Pillow is importable); its pixels travel in the same buffer.  Without a
    fallback such a file raises ``UnsupportedJpeg``.  ``progressive=True`` (opt-in): a progressive file in the
    device's scope (``parse_jpeg(data, progressive=True)``) travels as its compressed bytes too, in a record of kind
    ``KIND_PROGRESSIVE`` with its scan table, and is decoded by one more launch; by default it takes the fallback."""
    if fallback is None:
        fallback = _default_fallback()
    entries = []
    for i, data in enumerate(files):
        if not isinstance(data, (bytes, bytearray, memoryview)):
            raise TypeError(f"image {i} must be the bytes of a file (got {type(data).__name__})")
        header = parse_jpeg(data, progressive)
        if header.reason is None:
            entries.append((bytes(data), header))
        elif fallback is None:
            raise UnsupportedJpeg(i, header.reason)
        else:
            entries.append((fallback(bytes(data)), None))
    return _pack(entries)


def collate_jpeg(samples: Sequence, fallback: Optional[Callable] = None, progressive: bool = False) -> dict:
    """``collate_fn`` of a loader that does not decode (``datasets.Image(decode=False)``: a sample's ``"image"`` is the
    file's bytes, or a dict with them under ``"bytes"``): ``{"images": JpegBatch, ...}`` with every other entry collated
    as ``torch.utils.data.default_collate`` does.  ``progressive``: as in ``pack_jpegs`` (bind it with
    ``functools.partial``); this is where progressive decoding on the device is chosen, the decoder follows the batch."""
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
    batch = {"images": pack_jpegs(files, fallback, progressive)}
    if samples:
        rest = [{k: v for k, v in s.items() if k != "image"} for s in samples]
        if rest[0]:
            batch.update(default_collate(rest))
    return batch


# ----------------------------------------------------------------------------------------------------------------
# the launches
# ----------------------------------------------------------------------------------------------------------------
class JpegDecoder:
    """``JpegDecoder(device)(jpeg_batch) -> RaggedBatch`` of three channels on the device.  ``jpeg_batch.data`` lives on
    the device (one upload); the record table goes up with one non-blocking copy (``_launch.RecordTable``); then three
    launches on the current stream, no wait for the device.  ``workspace`` (coefficients and component planes, 192
    bytes per 8 x 8 block, behind the per-image status words) grows to the largest batch seen and is never cleared.
    ``status()`` reads the batch status word back (0: every image decoded; bit ``code - 1`` of ``STATUS_NAMES``
    otherwise), ``image_status()`` the last batch's per-image words; both wait for the device.

    ``entropy``: how the first launch decodes the Huffman data.  ``"serial"`` (the default, ``basd_jpeg_decode``): one
    lane per entropy-coded segment, so a file without restart markers is decoded by one lane.  ``"parallel"``
    (``basd_jpeg_decode_parallel``): a workgroup per image whose lanes decode sub-sequences of ``sub_bytes`` bytes of a
    segment speculatively and synchronise (the scheme is in ``include/basd_hip.h``); ``sub_bytes``: ``None`` (the
    built-in default) or a multiple of 8 in ``SUB_BYTES_MIN .. SUB_BYTES_MAX``.  Both give the same bytes and the same
    status words for every stream, intact or damaged.

    A batch that holds progressive records (``pack_jpegs(..., progressive=True)``) goes through
    ``basd_jpeg_decode_progressive``: one more launch ahead of the same three, a workgroup per progressive image that
    runs its scans level by level.  A batch without them issues exactly the launches above."""

    ENTROPY = ("serial", "parallel")

    def __init__(self, device, entropy: str = "serial", sub_bytes: Optional[int] = None) -> None:
        if entropy not in self.ENTROPY:
            raise ValueError(f"entropy must be one of {', '.join(repr(e) for e in self.ENTROPY)} (got {entropy!r})")
        if sub_bytes is not None:
            if entropy != "parallel":
                raise ValueError('sub_bytes belongs to entropy="parallel" (the serial stage has no sub-sequences)')
            if isinstance(sub_bytes, bool) or not isinstance(sub_bytes, int) or sub_bytes % 8 or \
                    not SUB_BYTES_MIN <= sub_bytes <= SUB_BYTES_MAX:
                raise ValueError(f"sub_bytes must be a multiple of 8 in {SUB_BYTES_MIN} .. {SUB_BYTES_MAX} "
                                 f"(got {sub_bytes!r})")
        self.device = torch.device(device)
        self.entropy = entropy
        self.sub_bytes = sub_bytes
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

    def __call__(self, batch: JpegBatch) -> RaggedBatch:
        if not isinstance(batch, JpegBatch):
            raise TypeError(f"batch must be a JpegBatch (got {type(batch).__name__}); pack_jpegs makes one")
        if not lives_on(self.device, batch.device):
            raise ValueError(f"the streams live on {batch.device}, the decoder on {self.device}")
        B = len(batch)
        rec = batch.records
        # every limit of include/basd_hip.h that the host can see (the kernels check each record again)
        for name, limit in (("width", MAX_SIDE), ("height", MAX_SIDE)):
            if B and (int(rec[name].min()) < 1 or int(rec[name].max()) > limit):
                i = int(np.flatnonzero((rec[name] < 1) | (rec[name] > limit))[0])
                raise ValueError(f"image {i} has {name} {int(rec[name][i])} (1 .. {limit} are decoded)")
        require_gpu(batch.data, f"the {B} streams")                    # the arguments are checked before the device is
        out = torch.empty(batch.out_bytes, dtype=torch.uint8, device=batch.device)
        ragged = RaggedBatch(out, batch.sizes, 3)
        self._last = B
        if B == 0:
            return ragged
        need = batch.workspace_bytes
        if bool((_blocks_of(rec) * 192 > need).any()):
            raise ValueError("a record describes more blocks than the batch's workspace holds")
        if self.workspace is None or self.workspace.numel() < need:
            retire(self.workspace)
            self.workspace =torch.empty(need, dtype=torch.uint8, device=batch.device)
        self.used_bytes = need
        self._records.stage(B, batch.device)[...] = rec
        args = (batch.data.data_ptr(), batch.data.numel(), out.data_ptr(), out.numel(), B, self._records.upload(),
                self.workspace.data_ptr(), self.workspace.numel(), self._records.status_ptr, batch.max_blocks,
                batch.max_pixels)
        if batch.progressive:                                          # one more launch, ahead of the same three
            _lib.call("basd_jpeg_decode_progressive", *args, self.sub_bytes or 0, int(self.entropy == "parallel"),
                      batch.max_scans, batch.max_segments, raw_stream(batch.device.index))
        elif self.entropy == "parallel":
            _lib.call("basd_jpeg_decode_parallel", *args, self.sub_bytes or 0, raw_stream(batch.device.index))
        else:
            _lib.call("basd_jpeg_decode", *args, raw_stream(batch.device.index))
        return ragged


# ----------------------------------------------------------------------------------------------------------------
# the specification in numpy (tests and the goldens script; the product path does not use it)
# ----------------------------------------------------------------------------------------------------------------
class _Bits:
    """MSB-first bits of ``data[pos:end]`` with FF 00 un-stuffing; a marker or the end stops the supply."""

    def __init__(self, data: bytes, pos: int, end: int) -> None:
        self.data, self.pos, self.end = data, pos, end
        self.acc, self.n = 0, 0

    def _byte(self) -> bool:
        if self.pos >= self.end:
            return False
        v = self.data[self.pos]
        if v == 0xFF:
            if self.pos + 1 >= self.end or self.data[self.pos + 1] != 0:
                return False
            self.pos += 1
        self.pos += 1
        self.acc = (self.acc << 8) | v
        self.n += 8
        return True

    def take(self, count: int) -> int:
        while self.n < count:
            if not self._byte():
                raise ValueError("the entropy-coded data ends early")
        self.n -= count
        v = (self.acc >> self.n) & ((1 << count) - 1)
        self.acc &= (1 << self.n) - 1
        return v


def _codes(data: bytes, off: int) -> dict:
    """(length, code) -> value of the DHT table whose counts start at ``off``."""
    table, code, p = {}, 0, off + 16
    for l in range(1, 17):
        for _ in range(data[off + l - 1]):
            table[(l, code)] = data[p]
            code += 1
            p += 1
        code <<= 1
    return table


def _symbol(bits: _Bits, table: dict) -> int:
    code = 0
    for l in range(1, 17):
        code = (code << 1) | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("a bit pattern that is no Huffman code")


def _extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def _idct_pass(c: np.ndarray) -> np.ndarray:
    """The 1-D transform along axis 0 of an (8, ...) int64 array, unscaled."""
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3])


def _idct(blocks: np.ndarray) -> np.ndarray:
    """(n, 8, 8) dequantised int64 blocks -> (n, 8, 8) uint8 samples."""
    cols = (_idct_pass(blocks.transpose(1, 2, 0)) + (1 << 10)) >> 11             # (row, column, n): along the columns
    rows = (_idct_pass(cols.transpose(1, 0, 2)) + (1 << 17)) >> 18               # (column, row, n): along the rows
    return np.clip(rows.transpose(2, 1, 0) + 128, 0, 255).astype(np.uint8)


def _upsample(plane: np.ndarray, hs: int, vs: int) -> np.ndarray:
    """A chroma plane of real samples (int64) on the luma grid (not yet cropped)."""
    ch, n = plane.shape
    if hs == 1:
        return plane
    if n <= 2:
        return np.repeat(np.repeat(plane, vs, axis=0), 2, axis=1)
    if vs == 1:
        left = np.concatenate([plane[:, :1], plane[:, :-1]], axis=1)
        right = np.concatenate([plane[:, 1:], plane[:, -1:]], axis=1)
        out = np.empty((ch, 2 * n), dtype=np.int64)
        out[:, 0::2] = (3 * plane + left + 1) >> 2
        out[:, 1::2] = (3 * plane + right + 2) >> 2
        out[:, 0], out[:, -1] = plane[:, 0], plane[:, -1]
        return out
    above = np.concatenate([plane[:1], plane[:-1]], axis=0)
    below = np.concatenate([plane[1:], plane[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * n), dtype=np.int64)
    for parity, neighbour in ((0, above), (1, below)):
        cs = 3 * plane + neighbour
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        rows = np.empty((ch, 2 * n), dtype=np.int64)
        rows[:, 0::2] = (3 * cs + left + 8) >> 4
        rows[:, 1::2] = (3 * cs + right + 7) >> 4
        rows[:, 0], rows[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[parity::2] = rows
    return out


def _wrap16(v: int) -> int:
    return ((v + 32768) & 0xFFFF) - 32768


def _progressive_coefficients(data: bytes, h: JpegHeader, shapes: list) -> list:
    """The scans of a progressive stream, one after the other as ``include/basd_hip.h`` states them: per component the
    (rows, columns, 64) int64 array of its int16 coefficients in zigzag order, not yet dequantised."""
    W, H, ncomp = h.width, h.height, h.ncomp
    hs, vs = (1, 1) if ncomp == 1 else (h.hs, h.vs)
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    layout = [(0, bx, by) for by in range(vs) for bx in range(hs)] + ([(1, 0, 0), (2, 0, 0)] if ncomp == 3 else [])
    coefs = [np.zeros((s[0] // 8, s[1] // 8, 64), dtype=np.int64) for s in shapes]
    for scan in h.scans:
        ss, se, ah, al = scan.ss, scan.se, scan.ah, scan.al
        if len(scan.comps) > 1:                                        # interleaved: the frame's MCUs
            units = [[(c, my * (vs if c == 0 else 1) + by, mx * (hs if c == 0 else 1) + bx) for c, bx, by in layout]
                     for my in range(mcuy) for mx in range(mcux)]
        else:                                                          # the component's own blocks, not MCU-padded
            c = scan.comps[0]
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            bw, bh = -(-(-(-W * ch // hs)) // 8), -(-(-(-H * cv // vs)) // 8)
            units = [[(c, by, bx)] for by in range(bh) for bx in range(bw)]
        total = len(units)
        per = scan.restart or total
        if len(scan.segments) != -(-total // per):
            raise ValueError(f"{len(scan.segments)} segments for {total} scan units in intervals of {per}")
        dc = {c: _codes(data, scan.dc[c]) for c in scan.comps} if ss == 0 and ah == 0 else {}
        ac = _codes(data, scan.ac) if ss > 0 else {}
        p1, m1 = 1 << al, -1 << al
        for seg, start in enumerate(scan.segments):
            end = scan.segments[seg + 1] - 2 if seg + 1 < len(scan.segments) else scan.data_end
            if seg and data[start - 2:start] != bytes([0xFF, 0xD0 + ((seg - 1) & 7)]):
                raise ValueError(f"segment {seg} does not start behind RST{(seg - 1) & 7}")
            bits = _Bits(data, start, end)
            pred, eobrun = [0] * ncomp, 0
            for unit in units[seg * per:(seg + 1) * per]:
                for c, by, bx in unit:
                    block = coefs[c][by, bx]
                    if ss == 0 and ah == 0:                            # DC first
                        s = _symbol(bits, dc[c])
                        if s > 15:
                            raise ValueError("a DC category above 15")
                        if s:
                            pred[c] += _extend(bits.take(s), s)
                        if not -32768 <= pred[c] <= 32767:
                            raise ValueError("a DC value outside 16 bits")
                        block[0] = _wrap16(pred[c] << al)
                    elif ss == 0:                                      # DC refinement
                        if bits.take(1):
                            block[0] = _wrap16(int(block[0]) | p1)
                    elif ah == 0:                                      # AC first
                        if eobrun > 0:
                            eobrun -= 1
                            continue
                        k = ss
                        while k <= se:
                            rs = _symbol(bits, ac)
                            r, s = rs >> 4, rs & 15
                            if s:
                                k += r
                                if k > se:
                                    raise ValueError("a coefficient index past the scan's band")
                                block[k] = _wrap16(_extend(bits.take(s), s) * p1)
                                k += 1
                            elif r == 15:
                                k += 16
                            else:
                                eobrun = (1 << r) - 1 + (bits.take(r) if r else 0)
                                break
                    else:                                              # AC refinement
                        def correct(k):
                            v = int(block[k])
                            if bits.take(1) and not v & p1:
                                block[k] = _wrap16(v + (p1 if v >= 0 else m1))
                        k = ss
                        if eobrun == 0:
                            while k <= se:
                                rs = _symbol(bits, ac)
                                r, s = rs >> 4, rs & 15
                                new = 0
                                if s:
                                    if s != 1:
                                        raise ValueError("a refinement symbol with a size above 1")
                                    new = p1 if bits.take(1) else m1
                                elif r != 15:
                                    eobrun = (1 << r) + (bits.take(r) if r else 0)
                                    break
                                while k <= se:
                                    if block[k]:
                                        correct(k)
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if new:
                                    if k > se:
                                        raise ValueError("a coefficient index past the scan's band")
                                    block[k] = new
                                k += 1
                        if eobrun > 0:
                            for j in range(k, se + 1):
                                if block[j]:
                                    correct(j)
                            eobrun -= 1
    return coefs


def decode_reference(data, progressive: bool = False) -> np.ndarray:
    """The specification of ``include/basd_hip.h`` in numpy: the (H, W, 3) uint8 RGB image of a stream in the device's
    scope (with ``progressive=True`` that of ``parse_jpeg(data, progressive=True)``: progressive streams too);
    ``ValueError`` for a stream outside it or a bad one."""
    data = bytes(data)
    h = parse_jpeg(data, progressive)
    if h.reason is not None:
        raise ValueError(f"not in the device's scope: {h.reason}")
    W, H, ncomp = h.width, h.height, h.ncomp
    hs, vs = (1, 1) if ncomp == 1 else (h.hs, h.vs)
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    if h.scans:
        shapes = [(mcuy * vs * 8, mcux * hs * 8)] + [(mcuy * 8, mcux * 8)] * (ncomp - 1)
        coefs = []
        for c, zz in enumerate(_progressive_coefficients(data, h, shapes)):
            q = np.frombuffer(data, dtype=np.uint8, count=64, offset=h.quant[c]).astype(np.int64)
            natural = np.zeros_like(zz)
            natural[:, :, _ZIGZAG] = zz * q
            coefs.append(natural)
        return _pixels_of(coefs, shapes, h)
    layout = [(0, bx, by) for by in range(vs) for bx in range(hs)] + ([(1, 0, 0), (2, 0, 0)] if ncomp == 3 else [])
    total = mcux * mcuy
    per = h.restart or total
    if len(h.segments) != -(-total // per):
        raise ValueError(f"{len(h.segments)} segments for {total} MCUs in intervals of {per}")
    dc = [_codes(data, off) for off in h.dc]
    ac = [_codes(data, off) for off in h.ac]
    quant = [np.frombuffer(data, dtype=np.uint8, count=64, offset=off).astype(np.int64) for off in h.quant]
    shapes = [(mcuy * vs * 8, mcux * hs * 8)] + [(mcuy * 8, mcux * 8)] * (ncomp - 1)
    coefs = [np.zeros((s[0] // 8, s[1] // 8, 64), dtype=np.int64) for s in shapes]
    for seg, start in enumerate(h.segments):
        end = h.segments[seg + 1] - 2 if seg + 1 < len(h.segments) else len(data)
        if seg and data[start - 2:start] != bytes([0xFF, 0xD0 + ((seg - 1) & 7)]):
            raise ValueError(f"segment {seg} does not start behind RST{(seg - 1) & 7}")
        bits = _Bits(data, start, end)
        pred = [0] * ncomp
        for m in range(seg * per, min((seg + 1) * per, total)):
            mx, my = m % mcux, m // mcux
            for c, bx, by in layout:
                block = coefs[c][my * (vs if c == 0 else 1) + by, mx * (hs if c == 0 else 1) + bx]
                s = _symbol(bits, dc[c])
                if s > 15:
                    raise ValueError("a DC category above 15")
                if s:
                    pred[c] += _extend(bits.take(s), s)
                block[0] = pred[c] * quant[c][0]
                k = 1
                while k < 64:
                    rs = _symbol(bits, ac[c])
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        if k > 63:
                            raise ValueError("a coefficient index past 63")
                        block[_ZIGZAG[k]] = _extend(bits.take(s), s) * quant[c][k]
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        break
    return _pixels_of(coefs, shapes, h)


def _pixels_of(coefs: list, shapes: list, h: JpegHeader) -> np.ndarray:
    """Dequantised coefficients (per component (rows, columns, 64) in natural order) to the RGB image."""
    W, H, ncomp = h.width, h.height, h.ncomp
    hs, vs = (1, 1) if ncomp == 1 else (h.hs, h.vs)
    planes = []
    for c, (ph, pw) in enumerate(shapes):
        samples = _idct(coefs[c].reshape(-1, 8, 8)).reshape(ph // 8, pw // 8, 8, 8)
        planes.append(samples.transpose(0, 2, 1, 3).reshape(ph, pw).astype(np.int64))
    Y = planes[0][:H, :W]
    if ncomp == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
    cwr, chr_ = -(-W // hs), -(-H // vs)
    cb, cr = (_upsample(p[:chr_, :cwr], hs, vs)[:H, :W] - 128 for p in planes[1:])
    F = lambda x: int(x * 65536 + 0.5)                                   # noqa: E731
    R = Y + ((F(1.402) * cr + 32768) >> 16)
    B = Y + ((F(1.772) * cb + 32768) >> 16)
    G = Y + ((-F(0.34414) * cb + 32768 - F(0.71414) * cr) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)
