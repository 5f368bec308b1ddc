"""Writes tests/golden/jpeg_progressive.npz: progressive JPEG streams with Pillow's decoded RGB
(``np.asarray(Image.open(...).convert("RGB"))``) for each.  Written with Pillow 12.2.0 (libjpeg-turbo); run from the
repository root:

    python tests/golden/make_goldens_jpeg_progressive.py

(a) Pillow-made streams: Pillow writes them (``progressive=True``: libjpeg's own scan script, ten scans for three
    components, six for one) and Pillow decodes them.
(b) Hand-made streams: the small progressive encoder below takes the quantised coefficients of a Pillow-made stream
    (read with ``basd_amd.jpeg``'s numpy reference) and writes them under another scan script and restart interval, with
    trivial Huffman tables (16 DC symbols as 5-bit codes; 256 AC symbols, 128 as 9-bit and 128 as 10-bit codes).  The
    check on the encoder: Pillow decodes each hand-made stream to the very pixels of the stream it came from, asserted
    here.

Keys: ``names`` (in order), ``stream_<name>`` (uint8), ``origin`` (per name the name whose pixels it decodes to: itself
for a Pillow-made stream), ``rgb_<name>`` (H, W, 3) uint8 for the names that are their own origin.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "vit-inductive-bias-distillation_amd"))
sys.path.insert(0, HERE)

from basd_amd import jpeg as J  # noqa: E402
from make_goldens_jpeg_decode import SUBSAMPLING, decode, encode, picture  # noqa: E402

MODES = ("gray", "444", "422", "420")
SIZES = ((1, 1), (7, 9), (8, 8), (9, 17), (17, 33), (33, 31), (40, 24), (64, 48))          # width, height
HAND_SIZES = ((1, 1), (9, 17), (17, 33), (33, 31))
FLAT = (1456, 1448)                  # 182 x 181 = 32942 blocks: an end-of-band run reaches 32767 and a second begins


# ---- the scan scripts of the hand-made streams: rows of (components, ss, se, ah, al) ------------------------------------
def script_spectral(ncomp):
    """Spectral selection only."""
    comps = list(range(ncomp))
    return [(comps, 0, 0, 0, 0)] + [([c], a, b, 0, 0) for c in comps for a, b in ((1, 5), (6, 63))]


def script_reversed(ncomp):
    """Every DC scan of one component, the components in reversed order; one bit of DC refinement at the end."""
    comps = list(range(ncomp))[::-1]
    return [([c], 0, 0, 0, 1) for c in comps] + [([c], 1, 63, 0, 0) for c in comps] + [([c], 0, 0, 1, 0) for c in comps]


def script_al3(ncomp):
    """Al = 3 and three rounds of refinement, the bands split differently in every round."""
    comps = list(range(ncomp))
    rows = [(comps, 0, 0, 0, 3)] + [([c], a, b, 0, 3) for c in comps for a, b in ((1, 5), (6, 63))]
    for ah, bands in ((3, ((1, 9), (10, 63))), (2, ((1, 2), (3, 63))), (1, ((1, 63),))):
        rows += [(comps, 0, 0, ah, ah - 1)] + [([c], a, b, ah, ah - 1) for c in comps for a, b in bands]
    return rows


SCRIPTS = {"spectral": script_spectral, "reversed": script_reversed, "al3": script_al3}


# ---- the encoder ----------------------------------------------------------------------------------------------------
class _Writer:
    """Entropy-coded bits, MSB first, with FF 00 stuffing; ``flush`` pads the last byte with ones."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, count):
        self.acc = (self.acc << count) | (value & ((1 << count) - 1))
        self.n += count
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


DC_BITS = bytes([0, 0, 0, 0, 16] + [0] * 11) + bytes(range(16))                   # symbol s: the 5-bit code s
AC_BITS = bytes([0] * 8 + [128, 128] + [0] * 6) + bytes(range(256))               # s < 128: 9 bits; else 10 bits


def _dc_symbol(w, s):
    w.put(s, 5)


def _ac_symbol(w, s):
    if s < 128:
        w.put(s, 9)
    else:
        w.put(256 + s - 128, 10)


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def _magnitude(w, v, size):
    w.put(v if v >= 0 else v + (1 << size) - 1, size)


class _AcState:
    """The pending end-of-band run and the correction bits that wait behind it."""

    def __init__(self, w):
        self.w, self.run, self.bits = w, 0, []

    def flush(self):
        if self.run:
            size = self.run.bit_length() - 1
            _ac_symbol(self.w, size << 4)
            if size:
                self.w.put(self.run, size)
            self.run = 0
        for bit in self.bits:
            self.w.put(bit, 1)
        self.bits = []

    def end_of_band(self, bits):
        self.run += 1
        self.bits += bits
        if self.run == 0x7FFF or len(self.bits) > 900:
            self.flush()


def _ac_first(st, block, ss, se, al):
    run = 0
    for k in range(ss, se + 1):
        v = int(block[k])
        mag = abs(v) >> al
        if not mag:
            run += 1
            continue
        st.flush()
        while run > 15:
            _ac_symbol(st.w, 0xF0)
            run -= 16
        size = mag.bit_length()
        _ac_symbol(st.w, (run << 4) | size)
        _magnitude(st.w, mag if v > 0 else -mag, size)
        run = 0
    if run:
        st.end_of_band([])


def _ac_refine(st, block, ss, se, al):
    mags = [abs(int(block[k])) >> al for k in range(ss, se + 1)]
    last_new = max((i for i, m in enumerate(mags) if m == 1), default=-1)
    run, bits = 0, []
    for i, mag in enumerate(mags):
        if not mag:
            run += 1
            continue
        while run > 15 and i <= last_new:
            st.flush()
            _ac_symbol(st.w, 0xF0)
            run -= 16
            for bit in bits:
                st.w.put(bit, 1)
            bits = []
        if mag > 1:
            bits.append(mag & 1)
            continue
        st.flush()
        _ac_symbol(st.w, (run << 4) | 1)
        st.w.put(0 if int(block[ss + i]) < 0 else 1, 1)
        for bit in bits:
            st.w.put(bit, 1)
        run, bits = 0, []
    if run or bits:
        st.end_of_band(bits)


def reencode(stream: bytes, script, restart: int) -> bytes:
    """The progressive stream ``stream`` (Pillow-made) written again under ``script`` with a restart interval of
    ``restart`` scan units (0: none)."""
    h = J.parse_jpeg(stream, progressive=True)
    assert h.reason is None, h.reason
    ncomp = h.ncomp
    hs, vs = (1, 1) if ncomp == 1 else (h.hs, h.vs)
    mcux, mcuy = -(-h.width // (8 * hs)), -(-h.height // (8 * vs))
    shapes = [(mcuy * vs * 8, mcux * hs * 8)] + [(mcuy * 8, mcux * 8)] * (ncomp - 1)
    coefs = J._progressive_coefficients(stream, h, shapes)
    # the head of the stream up to and including the frame header, without Huffman tables
    out, at, ids = bytearray(stream[:2]), 2, []
    while True:
        marker, length = stream[at + 1], int.from_bytes(stream[at + 2:at + 4], "big")
        if marker in (0xE0, 0xDB, 0xC2):
            out += stream[at:at + 2 + length]
        if marker == 0xC2:
            ids = [stream[at + 10 + 3 * c] for c in range(ncomp)]
            break
        at += 2 + length
    out += _segment(0xC4, bytes([0x00]) + DC_BITS + bytes([0x10]) + AC_BITS)
    if restart:
        out += _segment(0xDD, restart.to_bytes(2, "big"))
    layout = [(0, bx, by) for by in range(vs) for bx in range(hs)] + ([(1, 0, 0), (2, 0, 0)] if ncomp == 3 else [])
    for comps, ss, se, ah, al in script(ncomp):
        out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([ids[c], 0x00]) for c in comps)
                        + bytes([ss, se, (ah << 4) | al]))
        if len(comps) > 1:
            units = [[(c, my * (vs if c == 0 else 1) + by, mx * (hs if c == 0 else 1) + bx) for c, bx, by in layout]
                     for my in range(mcuy) for mx in range(mcux)]
        else:
            c = comps[0]
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            bw, bh = -(-(-(-h.width * ch // hs)) // 8), -(-(-(-h.height * cv // vs)) // 8)
            units = [[(c, by, bx)] for by in range(bh) for bx in range(bw)]
        per = restart or len(units)
        for seg in range(-(-len(units) // per)):
            if seg:
                out += bytes([0xFF, 0xD0 + ((seg - 1) & 7)])
            w = _Writer()
            st, pred = _AcState(w), [0] * ncomp
            for unit in units[seg * per:(seg + 1) * per]:
                for c, by, bx in unit:
                    block = coefs[c][by, bx]
                    if ss == 0 and ah == 0:
                        value = int(block[0]) >> al
                        diff, pred[c] = value - pred[c], value
                        size = abs(diff).bit_length()
                        _dc_symbol(w, size)
                        if size:
                            _magnitude(w, diff, size)
                    elif ss == 0:
                        w.put((int(block[0]) >> al) & 1, 1)
                    elif ah == 0:
                        _ac_first(st, block, ss, se, al)
                    else:
                        _ac_refine(st, block, ss, se, al)
            st.flush()
            w.flush()
            out += w.out
    return bytes(out + b"\xff\xd9")


# ---- the corpus -----------------------------------------------------------------------------------------------------
def _options(mode, quality, **more):
    options = dict(quality=quality, progressive=True, **more)
    if mode != "gray":
        options["subsampling"] = SUBSAMPLING[mode]
    return options


def corpus():
    """name -> (stream, the name whose pixels it has)."""
    rng = np.random.default_rng(20261020)
    streams, n = {}, 0
    for mode in MODES:
        for w, h in SIZES:
            # qualities 1 and 100: both at the small sizes, one of them in turn at the three largest (the file's size)
            n = MODES.index(mode) + SIZES.index((w, h))
            for quality in (1, 100) if w * h < 1000 else ((1, 100)[n % 2],):
                kind = ("noise", "ramp")[(n + quality) % 2]
                name = f"{mode}_{w}x{h}_q{quality}_{kind}"
                streams[name] = (encode(picture(rng, h, w, kind, mode == "gray"), **_options(mode, quality)), name)
            # quality 75: one picture plain and with restart markers, which change no coefficient and so no pixel
            kind = ("noise", "ramp")[n % 2]
            pixels = picture(rng, h, w, kind, mode == "gray")
            plain = f"{mode}_{w}x{h}_q75_{kind}"
            streams[plain] = (encode(pixels, **_options(mode, 75)), plain)
            for tag, more in (("rst1", dict(restart_marker_blocks=1)), ("rstrow", dict(restart_marker_rows=1))):
                made = encode(pixels, **_options(mode, 75, **more))
                assert np.array_equal(decode(made), decode(streams[plain][0])), (plain, tag)
                streams[f"{mode}_{w}x{h}_q75_{tag}"] = (made, plain)
    # 81 segments in every scan: more than a wave has lanes, and the marker count wraps modulo 8
    name = "444_72x72_q75_81segments"
    streams[name] = (encode(picture(rng, 72, 72, "ramp", False), **_options("444", 75, restart_marker_blocks=1)), name)
    name = f"gray_{FLAT[0]}x{FLAT[1]}_flat"
    streams[name] = (encode(np.full((FLAT[1], FLAT[0]), 97, dtype=np.uint8), **_options("gray", 75)), name)
    # hand-made: every script at every size in every mode, and with restart intervals 1 and 3 at 17 x 33
    for mode in MODES:
        for w, h in HAND_SIZES:
            origin = f"{mode}_{w}x{h}_q75_" + ("noise" if f"{mode}_{w}x{h}_q75_noise" in streams else "ramp")
            for tag, script in SCRIPTS.items():
                for restart in ((0, 1, 3) if (w, h) == (17, 33) else (0,)):
                    made = reencode(streams[origin][0], script, restart)
                    assert np.array_equal(decode(made), decode(streams[origin][0])), (mode, w, h, tag, restart)
                    streams[f"hand_{mode}_{w}x{h}_{tag}_rst{restart}"] = (made, origin)
    return streams


def main() -> None:
    streams = corpus()
    arrays = {"names": np.array(list(streams)), "origin": np.array([origin for _, origin in streams.values()])}
    for name, (stream, origin) in streams.items():
        arrays[f"stream_{name}"] = np.frombuffer(stream, dtype=np.uint8)
        if origin == name:
            arrays[f"rgb_{name}"] = decode(stream)
    path = os.path.join(HERE, "jpeg_progressive.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(streams)} streams, {os.path.getsize(path)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
