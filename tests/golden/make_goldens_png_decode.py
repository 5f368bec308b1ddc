"""Writes tests/golden/png_decode.npz: 8-bit PNG files made by Pillow's encoder with Pillow's decoded RGB
(``np.asarray(Image.open(...).convert("RGB"))``) for each, a palette file whose ``PLTE`` is shorter than its indices,
and one file per class the device leaves to the fallback.  Written with Pillow 12.2.0 and zlib 1.2.11; run from the
repository root:

    python tests/golden/make_goldens_png_decode.py

Keys: ``names`` (the files' names, in order), ``stream_<name>`` (uint8), ``rgb_<name>`` (H, W, 3) uint8.

The module is also the tests' PNG writer (``tests/test_png_decode.py`` imports it; Pillow is imported only by the
functions that need it): ``write_png`` takes pixels, a filter type per row and the options of ``zlib.compressobj``,
``Deflate`` emits deflate blocks by hand for what zlib does not produce.
"""
import io
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MODES = {"L": 0, "RGB": 2, "P": 3, "LA": 4, "RGBA": 6}          # Pillow mode -> colour type
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIZES = ((1, 1), (2, 3), (7, 8), (8, 17), (17, 32), (32, 33), (33, 63), (63, 64), (64, 65), (65, 2))   # (h, w)


# ---------------------------------------------------------------------------------------------------------------------
# pictures and Pillow
# ---------------------------------------------------------------------------------------------------------------------
def picture(rng: np.random.Generator, height: int, width: int, kind: str, mode: str) -> np.ndarray:
    """(H, W) or (H, W, C) uint8 pixels of a Pillow mode: ``noise`` (every byte random) or ``ramp`` (a noisy ramp,
    which compresses: matches, long and short codes)."""
    channels = {"L": 1, "P": 1, "LA": 2, "RGB": 3, "RGBA": 4}[mode]
    shape = (height, width, channels)
    if kind == "noise":
        pixels = rng.integers(0, 256, size=shape)
    else:
        yy, xx = np.mgrid[0:height, 0:width]
        ramp = xx * 255.0 / max(width - 1, 1) + yy * 128.0 / max(height - 1, 1)
        pixels = np.clip(np.stack([ramp, ramp[::-1], 255 - ramp, ramp / 2][:channels], axis=2)
                         + rng.integers(-2, 3, size=shape) * (rng.random(shape) < 0.2), 0, 255)
    pixels = pixels.astype(np.uint8)
    return pixels[:, :, 0] if channels == 1 else pixels


def palette(rng: np.random.Generator, entries: int = 256) -> bytes:
    return rng.integers(0, 256, size=3 * entries).astype(np.uint8).tobytes()


def encode(pixels: np.ndarray, mode: str, plte: bytes = None, **options) -> bytes:
    """Pillow's PNG of the pixels (``plte``: the palette of a ``P`` image)."""
    from PIL import Image
    image = Image.fromarray(pixels, mode="P" if mode == "P" else None)
    if mode == "P":
        image.putpalette(plte)
    out = io.BytesIO()
    image.save(out, format="PNG", **options)
    return out.getvalue()


def decode(stream: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def expected_rgb(pixels: np.ndarray, color_type: int, plte: bytes = None) -> np.ndarray:
    """What ``convert("RGB")`` makes of the source pixels: PNG is lossless."""
    px = pixels.reshape(pixels.shape[0], pixels.shape[1], -1)
    if color_type == 3:
        table = np.zeros(768, dtype=np.uint8)
        table[:len(plte)] = np.frombuffer(plte, dtype=np.uint8)
        return table.reshape(256, 3)[px[:, :, 0]]
    if color_type in (0, 4):
        return np.repeat(px[:, :, :1], 3, axis=2)
    return np.ascontiguousarray(px[:, :, :3])


# ---------------------------------------------------------------------------------------------------------------------
# the PNG writer
# ---------------------------------------------------------------------------------------------------------------------
def chunk(kind: bytes, payload: bytes, crc: int = None) -> bytes:
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(
        ">I", zlib.crc32(kind + payload) if crc is None else crc)


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(pixels: np.ndarray, filters) -> list:
    """The filtered scanlines (filter byte first) of (H, W, bpp) pixels, one ``bytes`` per row.  A filter type above 4
    is written as it is, over unfiltered bytes."""
    h, w, bpp = pixels.shape
    rows, prev = [], np.zeros(w * bpp, dtype=np.int64)
    for y in range(h):
        cur = pixels[y].reshape(-1).astype(np.int64)
        left = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, dtype=np.int64), prev[:-bpp]])
        ft = int(filters[y])
        if ft == 1:
            line = cur - left
        elif ft == 2:
            line = cur - prev
        elif ft == 3:
            line = cur - ((left + prev) >> 1)
        elif ft == 4:
            line = cur - np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, prev, upleft)], dtype=np.int64)
        else:
            line = cur
        rows.append(bytes([ft]) + (line & 255).astype(np.uint8).tobytes())
        prev = cur
    return rows


def deflate(rows, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush: int = None) -> bytes:
    """The zlib stream of the rows; ``flush``: a ``zlib.Z_*_FLUSH`` mode applied after every row."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out = b""
    for row in rows:
        out += co.compress(row)
        if flush is not None:
            out += co.flush(flush)
    return out + co.flush()


def zlib_wrap(raw_deflate: bytes, data: bytes, adler: int = None) -> bytes:
    """A raw deflate stream between the zlib header and the Adler-32 of ``data``."""
    return b"\x78\x9c" + raw_deflate + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def write_png(pixels: np.ndarray, color_type: int, filters=None, *, stream: bytes = None, plte: bytes = None,
              splits=(), extra=(), interlace: int = 0, depth: int = 8, **deflate_options) -> bytes:
    """A PNG file of (H, W) or (H, W, bpp) uint8 pixels.  ``filters``: a type per row (default 0); ``stream``: the
    zlib stream to store instead of compressing the filtered rows; ``splits``: positions in the stream at which a new
    ``IDAT`` chunk begins (a position given twice makes an empty chunk); ``extra``: ``(kind, payload)`` chunks put
    ahead of the first ``IDAT``; the remaining options are ``deflate``'s."""
    px = pixels.reshape(pixels.shape[0], pixels.shape[1], -1)
    h, w, bpp = px.shape
    assert bpp == BPP[color_type]
    if stream is None:
        stream = deflate(filter_rows(px, [0] * h if filters is None else filters), **deflate_options)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))
    if plte is not None:
        out += chunk(b"PLTE", plte)
    for kind, payload in extra:
        out += chunk(kind, payload)
    cuts = [0] + sorted(splits) + [len(stream)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", stream[a:b])
    return out + chunk(b"IEND", b"")


def write_adam7(pixels: np.ndarray, color_type: int) -> bytes:
    """The same picture interlaced (filter 0 in every pass): for the fallback route."""
    px = pixels.reshape(pixels.shape[0], pixels.shape[1], -1)
    rows = []
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = px[y0::dy, x0::dx]
        if sub.size:
            rows += [b"\0" + sub[y].tobytes() for y in range(sub.shape[0])]
    return write_png(pixels, color_type, stream=deflate(rows), interlace=1)


# ---------------------------------------------------------------------------------------------------------------------
# deflate by hand
# ---------------------------------------------------------------------------------------------------------------------
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
               227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0] * 4 + [e for e in range(1, 14) for _ in range(2)]
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def length_symbol(length: int, long258: bool = False):
    """(symbol, extra bits, extra value); ``long258``: 258 as symbol 284 with extra 31 instead of symbol 285."""
    if length == 258 and long258:
        return 284, 5, 31
    i = max(k for k in range(29) if LENGTH_BASE[k] <= length and (k == 28 or length < 258))
    return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]


def dist_symbol(dist: int):
    d = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return d, DIST_EXTRA[d], dist - DIST_BASE[d]


def canonical(lengths) -> dict:
    """symbol -> (code, length) of a list of code lengths (RFC 1951, 3.2.2)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0], code, nxt = 0, 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = {}
    for s, l in enumerate(lengths):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


def flat_lengths(symbols, size: int) -> list:
    """Code lengths over ``size`` symbols that give those in ``symbols`` (padded with unused ones to a power of two)
    equal lengths: a complete code, or, for one symbol, the one code of 1 bit."""
    used = sorted(set(symbols))
    bits = max(1, (len(used) - 1).bit_length())
    spare = [s for s in range(size) if s not in used]
    used += spare[:(1 << bits) - len(used)] if len(used) > 1 else []
    lengths = [0] * size
    for s in used:
        lengths[s] = bits
    return lengths


def skewed_lengths(symbols, size: int) -> list:
    """Lengths 1, 2, ..., 14, 15, 15 for the 16 ``symbols`` in their order: complete, and the last ones have codes
    longer than any first-level look-up."""
    assert len(symbols) == 16 and len(set(symbols)) == 16
    lengths = [0] * size
    for k, s in enumerate(symbols):
        lengths[s] = min(k + 1, 15)
    return lengths


class Tokens:
    """An LZ77 parse built by hand: ``lit`` and ``match`` append a token and the bytes it stands for."""

    def __init__(self) -> None:
        self.tokens, self.data = [], bytearray()

    def lit(self, *values) -> "Tokens":
        for v in values:
            self.tokens.append(int(v))
            self.data.append(int(v))
        return self

    def match(self, length: int, dist: int) -> "Tokens":
        assert 3 <= length <= 258 and 1 <= dist <= len(self.data)
        start = len(self.data) - dist
        for j in range(length):
            self.data.append(self.data[start + j % dist])
        self.tokens.append((length, dist))
        return self


class Deflate:
    """A raw deflate stream written block by block, least significant bit first."""

    def __init__(self) -> None:
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, n: int) -> None:
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, length: int) -> None:          # Huffman codes go most significant bit first
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def header(self, final: bool, kind: int) -> None:
        self.bits(int(final), 1)
        self.bits(kind, 2)

    def stored(self, data: bytes, final: bool = False, nlen: int = None) -> None:
        self.header(final, 0)
        if self.n:
            self.bits(0, 8 - self.n)
        self.out += struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data

    def dynamic(self, tokens, lit_lengths, dist_lengths, final: bool = False, long258: bool = False, end: bool = True) -> None:
        """A dynamic block with the given code lengths (sent one by one through a code-length code of sixteen 4-bit
        codes); ``tokens``: literals (ints) and ``(length, distance)`` pairs."""
        self.header(final, 2)
        self.bits(len(lit_lengths) - 257, 5)
        self.bits(len(dist_lengths) - 1, 5)
        self.bits(15, 4)
        for s in CLEN_ORDER:
            self.bits(4 if s < 16 else 0, 3)
        for l in list(lit_lengths) + list(dist_lengths):
            self.code(l, 4)
        self.symbols(tokens, canonical(lit_lengths), canonical(dist_lengths), long258, end)

    def symbols(self, tokens, lit: dict, dist: dict, long258: bool = False, end: bool = True) -> None:
        for t in tokens:
            if isinstance(t, tuple):
                s, eb, ev = length_symbol(t[0], long258)
                self.code(*lit[s])
                self.bits(ev, eb)
                d, eb, ev = dist_symbol(t[1])
                self.code(*dist[d])
                self.bits(ev, eb)
            else:
                self.code(*lit[t])
        if end:
            self.code(*lit[256])

    def finish(self) -> bytes:
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def dynamic_stream(parse: Tokens, *, skewed: bool = False, long258: bool = False) -> bytes:
    """The zlib stream of one hand-made dynamic block that holds the parse (flat codes over the symbols it uses, or the
    skewed literal/length code of ``skewed_lengths`` over its first 16 of them)."""
    lits = [256] + [t if not isinstance(t, tuple) else length_symbol(t[0], long258)[0] for t in parse.tokens]
    dists = [dist_symbol(t[1])[0] for t in parse.tokens if isinstance(t, tuple)]
    if skewed:
        order = list(dict.fromkeys(lits))
        order += [s for s in range(286) if s not in order][:16 - len(order)]
        lit_lengths = skewed_lengths(order[::-1], 286)      # the symbols met first get the longest codes
    else:
        lit_lengths = flat_lengths(lits, 286)
    dist_lengths = flat_lengths(dists or [0], 30)
    d = Deflate()
    d.dynamic(parse.tokens, lit_lengths, dist_lengths, final=True, long258=long258)
    return zlib_wrap(d.finish(), bytes(parse.data))


# ---------------------------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------------------------
def corpus() -> dict:
    rng = np.random.default_rng(20251020)
    files = {}
    modes = ("L", "RGB", "P", "LA", "RGBA")
    levels = (0, 1, 6, 9)
    n = 0
    for repeat in range(3):
        for h, w in SIZES:
            mode = modes[(n + repeat) % 5]
            level = levels[(n // 5 + n) % 4]
            kind = "noise" if h * w <= 17 * 32 and n % 2 == 0 else "ramp"
            options = dict(compress_level=level)
            if n % 6 == 1:
                options = dict(optimize=True)
            name = f"{mode}_{w}x{h}_" + ("opt" if "optimize" in options else f"l{level}") + f"_{kind}"
            pixels = picture(rng, h, w, kind, mode)
            files[name] = encode(pixels, mode, palette(rng) if mode == "P" else None, **options)
            n += 1
    # transparency chunks, which convert("RGB") ignores
    files["RGB_17x8_l6_trns"] = encode(picture(rng, 8, 17, "noise", "RGB"), "RGB", transparency=(1, 2, 3))
    files["L_7x8_l6_trns"] = encode(picture(rng, 8, 7, "noise", "L"), "L", transparency=5)
    files["P_32x17_l6_trns"] = encode(picture(rng, 17, 32, "noise", "P"), "P", palette(rng), transparency=7)
    # a PLTE of 20 entries under indices up to 255
    files["P_8x7_plte20"] = write_png(picture(rng, 7, 8, "noise", "P"), 3, [0, 1, 2, 3, 4, 0, 1], plte=palette(rng, 20))
    # what the device leaves to the fallback
    from PIL import Image
    small = picture(rng, 9, 15, "ramp", "L")
    out = io.BytesIO()
    Image.fromarray(small > 128).save(out, format="PNG")
    files["fallback_1bit"] = out.getvalue()
    files["fallback_4bit_palette"] = encode(small % 13, "P", palette(rng, 13))
    out = io.BytesIO()
    Image.fromarray(small.astype(np.uint16) * 257).save(out, format="PNG")
    files["fallback_16bit"] = out.getvalue()
    files["fallback_interlaced"] = write_adam7(picture(rng, 9, 15, "ramp", "RGB"), 2)
    return files


def main() -> None:
    files = corpus()
    arrays = {"names": np.array(list(files))}
    for name, stream in files.items():
        arrays[f"stream_{name}"] = np.frombuffer(stream, dtype=np.uint8)
        arrays[f"rgb_{name}"] = decode(stream)
    path = os.path.join(HERE, "png_decode.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(files)} files, {os.path.getsize(path)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
