"""Writes tests/golden/jpeg_parallel.npz: streams for the parallel entropy stage (``JpegDecoder(entropy="parallel")``)
made by Pillow's encoder, with Pillow's decoded RGB for each.  Written with Pillow 12.2.0 (libjpeg-turbo); run from the
repository root:

    python tests/golden/make_goldens_jpeg_parallel.py

Keys as in jpeg_decode.npz: ``names``, ``stream_<name>`` (uint8), ``rgb_<name>`` (H, W, 3) uint8.  What each stream is
for (a chunk is 256 sub-sequences of 128 bytes by default, of 16 bytes in the tests' small setting):

  444_160x160_q100_noise   more than three default chunks, FF 00 pairs by the hundred, blocks of 100 bytes on average
  gray_256x256_flat        periodic bit streams: a decoder that starts inside one locks onto a wrong phase and never
  420_256x256_flat           falls into step, so only the bound on the rounds makes these come out right
  420_160x120_q90_ramp     a photograph-like stream: short blocks, quick synchronisation
  422_256x24_q100_rstrow   one restart interval per MCU row, each longer than a chunk of 16-byte sub-sequences
  420_5x3_q75_ramp         both sides below 8: one MCU
  gray_64x47_q90_across1024     the last block begins before byte 1024 = 64 x 16 of the entropy-coded data (before
  gray_276x208_q98_across32768  byte 32768 = 256 x 128 = 8 x 256 x 16 = 32 x 64 x 16) and ends behind it: in the last
                           sub-sequence of one chunk and in the next chunk, which holds nothing else (the pictures are
                           turned so that the last block is not a flat one; the seeds were found by search)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "vit-inductive-bias-distillation_amd"))
from make_goldens_jpeg_decode import decode, encode, picture  # noqa: E402


def last_block(stream: bytes):
    """Of a gray stream without restart intervals: the offsets, counted from the first entropy-coded byte, of the byte
    in which the last block begins and of the end of the data (the EOI marker)."""
    from basd_amd import jpeg as J
    header = J.parse_jpeg(stream)
    assert header.reason is None and header.ncomp == 1 and len(header.segments) == 1
    dc, ac = J._codes(stream, header.dc[0]), J._codes(stream, header.ac[0])
    bits = J._Bits(stream, header.scan_offset, len(stream))
    begins = 0
    for block in range(header.blocks):
        begins = bits.pos - (bits.n + 7) // 8
        s = J._symbol(bits, dc)
        if s:
            bits.take(s)
        k = 1
        while k < 64:
            rs = J._symbol(bits, ac)
            if rs & 15:
                k += (rs >> 4) + 1
                bits.take(rs & 15)
            elif rs >> 4 == 15:
                k += 16
            else:
                break
    return begins - header.scan_offset, len(stream) - 2 - header.scan_offset


def corpus() -> dict:
    rng = np.random.default_rng(20261019)
    streams = {}
    streams["444_160x160_q100_noise"] = encode(picture(rng, 160, 160, "noise", False), quality=100, subsampling=0)
    streams["gray_256x256_flat"] = encode(np.full((256, 256), 97, dtype=np.uint8), quality=75)
    flat = np.empty((256, 256, 3), dtype=np.uint8)
    flat[...] = (200, 60, 30)
    streams["420_256x256_flat"] = encode(flat, quality=75, subsampling=2)
    streams["420_160x120_q90_ramp"] = encode(picture(rng, 120, 160, "ramp", False), quality=90, subsampling=2)
    streams["422_256x24_q100_rstrow"] = encode(picture(rng, 24, 256, "noise", False), quality=100, subsampling=1,
                                               restart_marker_rows=1)
    streams["420_5x3_q75_ramp"] = encode(picture(rng, 3, 5, "ramp", False), quality=75, subsampling=2)
    for name, (height, width, quality, seed, boundary) in {"gray_64x47_q90_across1024": (47, 64, 90, 21, 1024),
                                                          "gray_276x208_q98_across32768": (208, 276, 98, 13, 32768)}.items():
        pixels = np.ascontiguousarray(picture(np.random.default_rng(seed), height, width, "ramp", True)[::-1, ::-1])
        stream = encode(pixels, quality=quality)
        begins, ends = last_block(stream)
        assert begins <= boundary - 3 and boundary + 1 <= ends <= boundary + 20, (name, begins, ends)
        streams[name] = stream
    return streams


def main() -> None:
    streams = corpus()
    arrays = {"names": np.array(list(streams))}
    for name, stream in streams.items():
        arrays[f"stream_{name}"] = np.frombuffer(stream, dtype=np.uint8)
        arrays[f"rgb_{name}"] = decode(stream)
    path = os.path.join(HERE, "jpeg_parallel.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(streams)} streams, {os.path.getsize(path)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
