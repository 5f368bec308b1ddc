"""``basd_amd.png``: 8-bit PNG decoding on the device, byte for byte Pillow's.

The chain of evidence: ``decode_reference`` (the specification of ``include/basd_hip.h`` in plain Python) equals Pillow
on live random files and on the recorded corpus; ``inflate_reference`` accepts exactly what zlib accepts; the per-image
code of the kernels (``csrc/png_core.h``), compiled for the host under the sanitizers, gives the recorded bytes and the
restatement's status words on the corpus and on every damaged stream; the kernels equal both on the GPU.  PNG is
lossless, so the expected output of a GPU test is the source pixels (or the recorded RGB); every comparison is
``array_equal``.
"""
import importlib.util
import os
import shutil
import subprocess
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import png as P
from basd_amd.png import (PngBatch, PngDecoder, UnsupportedPng, collate_png, decode_reference, decode_stream,
                          inflate_reference, pack_pngs, parse_png)
from basd_amd.resize import RaggedBatch, ResizeCrop, draw_crop_params, pack_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_decode.npz")


def _maker():
    spec = importlib.util.spec_from_file_location("make_goldens_png_decode",
                                                  os.path.join(ROOT, "tests", "golden", "make_goldens_png_decode.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


M = _maker()


@pytest.fixture(scope="module")
def corpus():
    """name -> (file bytes, Pillow's RGB), in the file's order."""
    g = np.load(GOLDEN, allow_pickle=False)
    return {str(n): (g[f"stream_{n}"].tobytes(), g[f"rgb_{n}"]) for n in g["names"]}


def _inscope(corpus):
    return {n: v for n, v in corpus.items() if not n.startswith("fallback_")}


def _stream_of(data: bytes):
    """(concatenated IDAT payloads, header, PLTE bytes) of a file in scope."""
    h = parse_png(data)
    assert h.reason is None, h.reason
    return P._idat(data, h), h, None if h.plte is None else data[h.plte[0]:sum(h.plte)]


def _first_block_type(stream: bytes) -> int:
    return (stream[2] >> 1) & 3


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against Pillow and against zlib
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow():
    """256 seeded files from the grid modes x sizes x encoder options x transparency; the grid must keep producing all
    five filter types and all three block types."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(11)
    sizes = ((1, 1), (7, 1), (1, 5), (32, 32), (33, 17), (48, 64))                 # (h, w)
    options = (dict(compress_level=0), dict(compress_level=1), dict(compress_level=6), dict(compress_level=9),
               dict(optimize=True))
    grid = [(mode, size, kind, o, trns) for mode in M.MODES for size in sizes for kind in ("noise", "ramp")
            for o in range(5) for trns in (False, True)]
    picks = rng.permutation(len(grid))[:256]
    filters, blocks, seen = np.zeros(5, dtype=np.int64), np.zeros(3, dtype=np.int64), set()
    for n in picks:
        mode, (h, w), kind, o, trns = grid[n]
        opts = dict(options[o])
        if trns and mode in ("L", "RGB", "P"):
            opts["transparency"] = {"L": 9, "RGB": (9, 8, 7), "P": 3}[mode]
        plte = M.palette(rng) if mode == "P" else None
        pixels = M.picture(rng, h, w, kind, mode)
        if mode == "P" and pixels.max() < 17:
            pixels[0, 0] = 200                       # more than 16 colours, or Pillow writes fewer than 8 bits
        data = M.encode(pixels, mode, plte, **opts)
        stream, header, _ = _stream_of(data)
        got = decode_reference(data)
        assert np.array_equal(got, M.decode(data)), (mode, h, w, kind, opts)
        assert np.array_equal(got, M.expected_rgb(pixels, M.MODES[mode], plte)), (mode, h, w, kind, opts)
        raw = zlib.decompress(stream)
        filters += np.bincount(np.frombuffer(raw, dtype=np.uint8)[::header.filtered_bytes // h], minlength=5)[:5]
        blocks[_first_block_type(stream)] += 1
        seen.add((mode, (h, w), o))
    print(f"[png_decode] rows per filter type {filters.tolist()}, first blocks (stored, fixed, dynamic) {blocks.tolist()}")
    assert (filters > 0).all() and (blocks > 0).all() and len(seen) > 100


def test_restatement_equals_the_recorded_pillow_outputs(corpus):
    assert os.path.getsize(GOLDEN) < 256 * 1024 and 30 <= len(corpus) <= 50
    base = _inscope(corpus)
    for name, (data, rgb) in base.items():
        assert np.array_equal(decode_reference(data), rgb), name
    sides = {s for _, rgb in base.values() for s in rgb.shape[:2]}
    assert {1, 2, 3, 7, 8, 17, 32, 33, 63, 64, 65} <= sides
    for word in ("L_", "RGB_", "P_", "LA_", "RGBA_", "_l0_", "_l1_", "_l6_", "_l9_", "_opt_", "_trns", "plte20", "noise",
                 "ramp"):
        assert any(word in name for name in base), word
    for data, want in ((corpus["RGB_17x8_l6_trns"][0], b"tRNS"), (corpus["P_32x17_l6_trns"][0], b"tRNS")):
        assert want in data
    # the short palette: indices past its 20 entries read (0, 0, 0)
    data, rgb = corpus["P_8x7_plte20"]
    assert parse_png(data).plte[1] == 60 and (rgb.reshape(-1, 3).sum(axis=1) == 0).sum() > 40
    assert sorted(n for n in corpus if n.startswith("fallback_")) == [
        "fallback_16bit", "fallback_1bit", "fallback_4bit_palette", "fallback_interlaced"]


def _zlib_verdict(stream: bytes, expected: int):
    """The inflated bytes where zlib reaches the end of the raw stream with that many bytes and the four bytes behind
    it are their Adler-32; else ``None``."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream[2:])
    except zlib.error:
        return None
    if not d.eof or len(out) != expected or len(d.unused_data) < 4:
        return None
    return out if int.from_bytes(d.unused_data[:4], "big") == zlib.adler32(out) else None


def _small_dynamic():
    """A hand-made dynamic block over a 3 x 4 gray image, for the damage that the corpus's two smallest streams (a
    stored and a fixed block) do not reach: (stream, header)."""
    parse = M.Tokens().lit(0, 7, 7, 7, 1, 9).match(4, 3).lit(2).match(3, 1).lit(250, 3)
    assert len(parse.data) == 4 * 4
    return M.dynamic_stream(parse), P.PngHeader(None, width=3, height=4, color_type=0, bit_depth=8)


def _damaged(corpus):
    """Per variant ``(stream, header, palette)``: every prefix of the corpus's two smallest streams and of a small
    hand-made dynamic block, and those streams with each byte replaced by 00, by FF and by its complement."""
    base = _inscope(corpus)
    streams = sorted((_stream_of(data) for data, _ in base.values()), key=lambda e: len(e[0]))[:2]
    streams.append(_small_dynamic() + (None,))
    entries = []
    for stream, header, plte in streams:
        entries += [(stream[:n], header, plte) for n in range(len(stream))]
        for at in range(len(stream)):
            for value in (0x00, 0xFF, stream[at] ^ 0xFF):
                entries.append((stream[:at] + bytes([value]) + stream[at + 1:], header, plte))
    return streams, entries


def test_inflate_restatement_accepts_what_zlib_accepts(corpus):
    base = _inscope(corpus)
    kinds = set()
    for name, (data, _) in base.items():
        stream, header, _ = _stream_of(data)
        out, status = inflate_reference(stream, header.filtered_bytes)
        assert status == 0 and out == _zlib_verdict(stream, header.filtered_bytes) == zlib.decompress(stream), name
        kinds.add(_first_block_type(stream))
    assert kinds == {0, 1, 2}
    streams, entries = _damaged(corpus)
    assert len(entries) > 600
    codes = {}
    for stream, header, _ in entries:
        out, status = inflate_reference(stream, header.filtered_bytes)
        want = _zlib_verdict(stream, header.filtered_bytes)
        assert (status == 0) == (want is not None), (stream.hex(), status)
        assert status in P.STATUS_NAMES and status not in (1, 9)
        if status == 0:
            assert out == want
        else:
            assert out == b""
        codes[status] = codes.get(status, 0) + 1
    print(f"[png_decode] damaged streams per status {sorted(codes.items())}")
    assert set(codes) >= {0, 2, 3, 4, 5, 6, 7, 8, 10}
    # one byte too many or too few expected, and a stream that is only its header
    stream, header, _ = streams[0]
    assert inflate_reference(stream, header.filtered_bytes + 1)[1] == 8
    assert inflate_reference(stream, header.filtered_bytes - 1)[1] == 8
    assert inflate_reference(stream[:2], 4)[1] == 7 and inflate_reference(b"", 4)[1] == 7
    # bytes behind the Adler-32 are ignored
    assert inflate_reference(stream + b"\x01\x02", header.filtered_bytes)[1] == 0


def test_parse_names_what_the_device_does_not_decode(corpus):
    good = corpus["RGB_17x8_l6_trns"][0]
    header = parse_png(good)
    assert header.reason is None and (header.width, header.height, header.color_type, header.bit_depth) == (17, 8, 2, 8)
    assert header.filtered_bytes == 8 * (17 * 3 + 1) and header.plte is None and len(header.idat) == 1
    pal = parse_png(corpus["P_8x7_plte20"][0])
    assert pal.reason is None and pal.color_type == 3 and pal.plte[1] == 60
    jpeg = b"\xff\xd8\xff\xe0" + bytes(40)
    for data, reason in ((corpus["fallback_1bit"][0], "1-bit"), (corpus["fallback_4bit_palette"][0], "4-bit"),
                         (corpus["fallback_16bit"][0], "16-bit"), (corpus["fallback_interlaced"][0], "interlaced"),
                         (good[:20], "truncated header"), (jpeg, "not a PNG file"), (b"", "not a PNG file (it starts with nothing"),
                         (good[:-12], "no IEND"), (good[:60], "broken chunk structure"),
                         (M.write_png(np.zeros((2, 2), dtype=np.uint8), 3), "without PLTE"),
                         (M.write_png(np.zeros((2, 2), dtype=np.uint8), 0, stream=b"\x78\xbb" + bytes(8)), "preset dictionary"),
                         (M.write_png(np.zeros((2, 2), dtype=np.uint8), 0, stream=b"\x88\x1c" + bytes(8)), "not deflate"),
                         (M.write_png(np.zeros((2, 2), dtype=np.uint8), 0, stream=b"\x78\x9d" + bytes(8)), "fails its check"),
                         (M.write_png(np.zeros((2, 2), dtype=np.uint8), 0, depth=16), "16-bit")):
        assert reason in parse_png(data).reason, (reason, parse_png(data).reason)
    with pytest.raises(ValueError, match="not in the device's scope: interlaced"):
        decode_reference(corpus["fallback_interlaced"][0])
    wide = bytearray(good)
    wide[16:20] = (P.MAX_SIDE + 1).to_bytes(4, "big")
    assert f"{P.MAX_SIDE + 1} x 8 pixels" in parse_png(bytes(wide)).reason
    # a wrong IDAT CRC is not looked at (Pillow decodes such a file too)
    at = good.index(b"IDAT")
    crc_at = at + 4 + int.from_bytes(good[at - 4:at], "big")
    broken = good[:crc_at] + bytes(4) + good[crc_at + 4:]
    assert parse_png(broken).reason is None and np.array_equal(decode_reference(broken), corpus["RGB_17x8_l6_trns"][1])
    # IDAT chunks of one byte with an empty chunk between each two: the same stream after packing
    rng = np.random.default_rng(5)
    pixels = M.picture(rng, 5, 6, "noise", "RGB")
    whole = M.write_png(pixels, 2, [0, 1, 2, 3, 4])
    stream = _stream_of(whole)[0]
    split = M.write_png(pixels, 2, [0, 1, 2, 3, 4], splits=[p for p in range(1, len(stream)) for _ in (0, 1)])
    spans = parse_png(split).idat
    assert len(spans) == 2 * len(stream) - 1 and {l for _, l in spans} == {0, 1}
    a, b = pack_pngs([whole]), pack_pngs([split])
    assert a.data.numpy().tobytes() == b.data.numpy().tobytes() and np.array_equal(a.records, b.records)
    assert a.data.numpy()[:len(stream)].tobytes() == stream
    assert np.array_equal(decode_reference(split), pixels)


def test_pack_layout_fallback_and_collate(corpus):
    names = ["RGB_17x8_l6_trns", "fallback_16bit", "P_8x7_plte20"]
    files = [corpus[n][0] for n in names]
    calls = []

    def fallback(data):
        calls.append(data)
        return corpus["fallback_16bit"][1]

    batch = pack_pngs(files, fallback=fallback)
    assert calls == [files[1]] and isinstance(batch, PngBatch) and len(batch) == 3 and batch.fallbacks == 1
    assert batch.data.dtype == torch.uint8 and batch.data.numel() % 16 == 0
    assert batch.sizes.tolist() == [[8, 17], [9, 15], [7, 8]] and batch.out_bytes == 3 * (8 * 17 + 9 * 15 + 7 * 8)
    rec, data = batch.records, batch.data.numpy()
    assert rec.dtype == P.RECORD_DTYPE and rec.dtype.itemsize == 64
    assert rec["kind"].tolist() == [0, 1, 0] and rec["color_type"].tolist() == [2, 2, 3]
    assert rec["out_offset"].tolist() == [0, 3 * 8 * 17, 3 * (8 * 17 + 9 * 15)]
    for i in (0, 2):
        stream, header, plte = _stream_of(files[i])
        at, n = int(rec["src_offset"][i]), int(rec["src_len"][i])
        assert data[at:at + n].tobytes() == stream
    at = int(rec["plte_offset"][2])
    plte = _stream_of(files[2])[2]
    assert data[at:at + 60].tobytes() == plte and not data[at + 60:at + 768].any()
    at = int(rec["src_offset"][1])
    assert np.array_equal(data[at:at + 9 * 15 * 3].reshape(9, 15, 3), corpus["fallback_16bit"][1])
    # the workspace: the status area, then the filtered scanlines at multiples of 16
    first = 8 * (17 * 3 + 1)
    assert P.status_bytes(3) == 128 and P.status_bytes(16) == 128 and P.status_bytes(17) == 256
    assert rec["ws_offset"].tolist() == [128, 0, 128 + first + (-first % 16)]
    assert batch.workspace_bytes == int(rec["ws_offset"][2]) + 7 * 9 and batch.max_filtered == first
    assert batch.max_pixels == 8 * 17
    saved, P._default_fallback = P._default_fallback, lambda: None
    try:
        with pytest.raises(UnsupportedPng, match=r"image 1 .*16-bit.*no fallback") as e:
            pack_pngs(files)
    finally:
        P._default_fallback = saved
    assert e.value.index == 1 and "16-bit" in e.value.reason
    with pytest.raises(ValueError, match=r"fallback of image 1 must return an \(H, W, 3\) uint8"):
        pack_pngs(files, fallback=lambda data: np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(TypeError, match="image 0 must be the bytes of a file"):
        pack_pngs([np.zeros(4)])
    empty = pack_pngs([])
    assert len(empty) == 0 and empty.data.numel() == 0 and empty.out_bytes == 0
    out = collate_png([{"image": files[0], "label": 3}, {"image": {"bytes": files[2], "path": None}, "label": 5}])
    assert isinstance(out["images"], PngBatch) and len(out["images"]) == 2 and out["label"].tolist() == [3, 5]
    with pytest.raises(KeyError, match="needs an 'image' entry"):
        collate_png([{"label": 1}])
    assert out["images"].to("cpu") is out["images"]


def test_default_fallback_is_pillow_and_takes_a_jpeg(corpus):
    pytest.importorskip("PIL")
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"), allow_pickle=False)
    name = str(g["names"][0])
    batch = pack_pngs([corpus["fallback_interlaced"][0], g[f"stream_{name}"].tobytes(), corpus["L_7x8_l6_trns"][0]])
    assert batch.fallbacks == 2 and batch.records["kind"].tolist() == [1, 1, 0]
    at = int(batch.records["src_offset"][1])
    rgb = g[f"rgb_{name}"]
    assert np.array_equal(batch.data.numpy()[at:at + rgb.size].reshape(rgb.shape), rgb)
    at = int(batch.records["src_offset"][0])
    rgb = corpus["fallback_interlaced"][1]
    assert np.array_equal(batch.data.numpy()[at:at + rgb.size].reshape(rgb.shape), rgb)


def test_exported_from_the_package():
    import basd_amd
    from basd_amd import _lib
    assert "``png``" in basd_amd.__doc__
    for name in ("PngBatch", "PngDecoder", "UnsupportedPng", "collate_png", "pack_pngs", "parse_png"):
        assert name in basd_amd.__all__ and getattr(basd_amd, name) is getattr(P, name)
    for name in ("PngHeader", "parse_png", "UnsupportedPng", "PngBatch", "pack_pngs", "collate_png", "PngDecoder",
                 "decode_reference", "inflate_reference", "RECORD_DTYPE", "STATUS_NAMES"):
        assert name in P.__all__
    vp, i32, i64 = _lib.vp, _lib.i32, _lib.i64
    assert _lib.SIGNATURES["basd_png_decode"] == [vp, i64, vp, i64, i32, vp, vp, i64, vp, i64, i64, vp]
    assert "basd_png_status_bytes" in _lib.LONG_RESULTS
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    for text in ("int basd_png_decode(", "BasdPngRecord", f"#define BASD_PNG_MAX_SIDE {P.MAX_SIDE}",
                 f"#define BASD_PNG_MAX_BATCH {P.MAX_BATCH}", "B = (n + sum (n - i) b_i) mod 65521"):
        assert text in header, text
    codes = {"BAD_RECORD": 1, "BAD_BLOCK": 2, "BAD_STORED": 3, "BAD_LENGTHS": 4, "BAD_CODE": 5, "BAD_DISTANCE": 6,
             "TRUNCATED": 7, "WRONG_LENGTH": 8, "BAD_FILTER": 9, "BAD_ADLER": 10}
    for name, code in codes.items():
        assert f"#define BASD_PNG_{name} {code} " in header, name
    assert sorted(P.STATUS_NAMES) == list(range(11))


def _config(points=4, classes=10, img_size=16, crop_ratio=0.875):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=points),
                           model=SimpleNamespace(num_classes=classes, vit=SimpleNamespace(img_size=img_size)),
                           data=SimpleNamespace(eval_crop_ratio=crop_ratio))


class OracleBASD(nn.Module):
    """The oracle behind the reference constructor's signature (test-side stand-in for the loss module on CPU)."""

    def __init__(self, base_criterion, student_dim, teacher_dim, student_depth, num_student_tokens, *, config,
                 teacher_has_cls_token):
        super().__init__()
        from oracle import basd_oracle as O
        self.token_layers = O.extraction_layers(student_depth, config.num_extraction_points)
        st = O.SelectorState.create(len(self.token_layers), student_dim, teacher_dim)
        self.log_temperatures = nn.Parameter(st.log_temperatures.detach().clone())


def _toy_models(dev="cpu"):
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=16, patch_size=4, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.StockViT(img_size=16, patch_size=4, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    return student, SM.make_teacher(teacher, 16)


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STATS = {"clean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "augmented": (MEAN, STD)}
TRAINER_FILES = ("RGB_33x32_l6_ramp", "P_32x17_l6_trns", "RGBA_65x64_l1_ramp", "L_33x32_l6_ramp")


def _trainer_files(corpus):
    for name in TRAINER_FILES:
        assert name in corpus, (name, sorted(corpus))
    return [corpus[n][0] for n in TRAINER_FILES], [corpus[n][1] for n in TRAINER_FILES]


def test_trainer_and_evaluation_argument_errors_on_cpu(corpus):
    from basd_amd import trainer as T
    from basd_amd.evaluation import evaluate_model
    from tools import stock_models as SM
    student, teacher = _toy_models()
    kw = dict(student_info=SM.probe_model(student, 16), loss_cls=OracleBASD)
    with pytest.raises(ValueError, match="png_decode needs resize_crop=True"):
        T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, png_decode=True, **kw)
    tr = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, resize_crop=True, png_decode=True, **kw)
    assert isinstance(tr._png_decoder, PngDecoder) and tr._decoder is None
    files, _ = _trainer_files(corpus)
    batch = pack_pngs(files)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.prepare_views({"images": batch, "label": torch.arange(4)})
    # the default is unchanged: no decoder, and a PngBatch is not taken
    plain = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, resize_crop=True, **kw)
    assert plain._png_decoder is None
    with pytest.raises(TypeError, match="resize_crop.*RaggedBatch"):
        plain.prepare_views({"images": batch, "label": torch.arange(4)})
    criterion = nn.CrossEntropyLoss()
    with pytest.raises(ValueError, match="png_decode needs resize_crop"):
        evaluate_model(student, [], criterion, num_classes=10, image_stats=(MEAN, STD), png_decode=PngDecoder("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_model(student, [{"images": batch, "label": torch.arange(4)}], criterion, num_classes=10,
                       image_stats=(MEAN, STD), resize_crop=ResizeCrop(16, 0.875, device="cpu"),
                       png_decode=PngDecoder("cpu"))
    with pytest.raises(TypeError, match="batch must be a PngBatch"):
        PngDecoder("cpu")(pack_images([np.zeros((4, 4, 3), dtype=np.uint8)]))
    bad = pack_pngs(files[:1])
    bad.records["width"][0] = P.MAX_SIDE + 1
    with pytest.raises(ValueError, match=f"image 0 has width {P.MAX_SIDE + 1}"):
        PngDecoder("cpu")(bad)


# ---------------------------------------------------------------------------------------------------------------------
# streams made for the purpose: filters, deflate structure, damage (shared by the host check and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
COLOR_OF_BPP = {1: 0, 2: 4, 3: 2, 4: 6}


def _filter_cases():
    """(name, file, RGB) for every bpp x width 1 .. 17 x height at the band boundaries x filter choice (each of the five
    types on every row, and a seeded mix); every fourth bpp-1 image is a palette image.  Noise pixels: Paeth ties and
    Average sums above 255 occur."""
    rng = np.random.default_rng(23)
    cases, n = [], 0
    for bpp in (1, 2, 3, 4):
        for w in range(1, 18):
            for h in (1, 2, 63, 64, 65, 129):
                for choice in (0, 1, 2, 3, 4, "mix"):
                    ctype = 3 if bpp == 1 and n % 4 == 3 else COLOR_OF_BPP[bpp]
                    pixels = rng.integers(0, 256, size=(h, w, bpp), dtype=np.uint8)
                    plte = M.palette(rng, 200) if ctype == 3 else None
                    filters = rng.integers(0, 5, size=h).tolist() if choice == "mix" else [choice] * h
                    cases.append((f"bpp{bpp}_{w}x{h}_f{choice}", M.write_png(pixels, ctype, filters, plte=plte, level=1),
                                  M.expected_rgb(pixels, ctype, plte)))
                    n += 1
    return cases


def _gray_file(data: bytes, stream: bytes, width: int):
    """A gray file around a hand-made zlib stream whose inflated bytes (all of them at most 4, so any of them may be a
    filter byte) are ``data``: (file, RGB by the restatement).  zlib inflates the stream to the same bytes."""
    assert len(data) % (width + 1) == 0 and max(data) <= 4 and zlib.decompress(stream) == bytes(data)
    h = len(data) // (width + 1)
    rgb, status = decode_stream(stream, width, h, 0)
    assert status == 0
    return M.write_png(np.zeros((h, width), dtype=np.uint8), 0, stream=stream), rgb


def _padded(parse, width: int, rng):
    while len(parse.data) % (width + 1):
        parse.lit(int(rng.integers(0, 5)))
    return parse


def _structure_cases():
    """(name, file, RGB): the shapes of a deflate stream, by zlib's options and by hand."""
    rng = np.random.default_rng(29)
    cases = []

    def add(name, pixels, ctype=2, **options):
        data = M.write_png(pixels, ctype, **options)
        cases.append((name, data, M.expected_rgb(pixels, ctype)))
        return _stream_of(data)[0]

    def stored_lengths(stream):
        at, out = 2, []
        while True:
            assert stream[at] & 6 == 0
            out.append(int.from_bytes(stream[at + 1:at + 3], "little"))
            if stream[at] & 1:
                return out
            at += 5 + out[-1]

    noise = rng.integers(0, 256, size=(148, 148, 3), dtype=np.uint8)
    lengths = stored_lengths(add("stored_level0", noise, level=0))
    assert len(lengths) >= 2 and sum(lengths) == 148 * (148 * 3 + 1)            # zlib cuts where its buffer fills
    # two stored blocks of the full 65535 bytes behind an empty one, by hand
    big = rng.integers(0, 256, size=(210, 210, 3), dtype=np.uint8)
    raw = b"".join(M.filter_rows(big, [0] * 210))
    d = M.Deflate()
    d.stored(b"")
    d.stored(raw[:65535])
    d.stored(raw[65535:131070])
    d.stored(raw[131070:], final=True)
    assert stored_lengths(add("stored_empty_and_two_full", big, stream=M.zlib_wrap(d.finish(), raw))) == [
        0, 65535, 65535, len(raw) - 131070]
    ramp = M.picture(rng, 33, 40, "ramp", "RGB")
    mixed = rng.integers(0, 5, size=33).tolist()
    assert _first_block_type(add("fixed", ramp, filters=mixed, strategy=zlib.Z_FIXED)) == 1
    add("huffman_only", ramp, filters=mixed, strategy=zlib.Z_HUFFMAN_ONLY)
    flat = np.zeros((40, 300, 3), dtype=np.uint8)
    flat[20:] = 77
    assert len(add("rle", flat, strategy=zlib.Z_RLE)) < 400                     # runs of 258 at distance 1
    assert add("sync_flush_rows", ramp, filters=mixed, flush=zlib.Z_SYNC_FLUSH).count(b"\x00\x00\xff\xff") >= 33
    add("full_flush_rows", ramp, filters=mixed, flush=zlib.Z_FULL_FLUSH)
    half = rng.integers(0, 256, size=(50, 110, 3), dtype=np.uint8)
    add("second_half_repeats", np.concatenate([half, half]), level=9)
    far = rng.integers(0, 256, size=(100, 110, 3), dtype=np.uint8)
    far[98] = far[0]                                                            # 98 rows of 331 bytes back: 32438
    assert len(add("distance_32438", far, level=9)) < 99 * 331 + 200
    # by hand: every distance in {1, 2, 3, 63, 64, 65} at every length in {3, 64, 65, 258}
    parse = M.Tokens().lit(*rng.integers(0, 5, size=70).tolist())
    for dist in (1, 2, 3, 63, 64, 65):
        for length in (3, 64, 65, 258):
            parse.match(length, dist).lit(int(rng.integers(0, 5)))
    _padded(parse, 17, rng)
    cases.append(("hand_distances_lengths",) + _gray_file(parse.data, M.dynamic_stream(parse), 17))
    # a distance equal to the bytes produced, length 258 as symbol 284 with extra 31, one distance code only
    parse = M.Tokens().lit(1, 2, 3, 4, 0).match(258, 5).match(258, 5).match(9, 5)
    stream = M.dynamic_stream(_padded(parse, 9, rng), long258=True)
    assert zlib.decompress(stream) != b"" and M.flat_lengths([M.dist_symbol(5)[0]], 30).count(1) == 1
    cases.append(("hand_distance_is_position_284_31_one_distance_code",) + _gray_file(parse.data, stream, 9))
    # a literal/length code of lengths 1 .. 15, 15: the symbols met first have codes past the first-level look-up
    parse = M.Tokens().lit(3, 1, 4, 1, 0, 2).match(3, 6).match(30, 2).match(258, 1).match(100, 64).lit(4, 4, 3)
    stream = M.dynamic_stream(_padded(parse, 12, rng), skewed=True)
    cases.append(("hand_15_bit_codes",) + _gray_file(parse.data, stream, 12))
    # distances up to 32768 exactly, by hand
    parse = M.Tokens().lit(*rng.integers(0, 5, size=8).tolist())
    while len(parse.data) + 258 <= 32768:
        parse.match(258, 8)
    if 32768 - len(parse.data) >= 3:
        parse.match(32768 - len(parse.data), 8)
    while len(parse.data) < 32768:
        parse.lit(1)
    parse.match(258, 32768).match(258, 32767).match(3, 32768)
    stream = M.dynamic_stream(_padded(parse, 127, rng))
    cases.append(("hand_distance_32768",) + _gray_file(parse.data, stream, 127))
    return cases


def _damage_cases():
    """(name, stream, header, code): one stream per status code the two launches can give a stream."""
    rng = np.random.default_rng(31)
    pixels = rng.integers(0, 256, size=(6, 5, 3), dtype=np.uint8)
    header = P.PngHeader(None, width=5, height=6, color_type=2, bit_depth=8)
    rows = M.filter_rows(pixels, [0, 1, 2, 3, 4, 1])
    raw = b"".join(rows)
    good = M.deflate(rows)
    cases = [("truncated", good[:len(good) // 2], 7)]
    d = M.Deflate()
    d.header(True, 3)
    cases.append(("block_type_3", M.zlib_wrap(d.finish() + bytes(8), raw), 2))
    d = M.Deflate()
    d.stored(raw, final=True, nlen=len(raw))
    cases.append(("nlen_mismatch", M.zlib_wrap(d.finish(), raw), 3))
    d = M.Deflate()
    lit = [0] * 257
    lit[0] = lit[1] = lit[256] = 1                                              # three codes of one bit
    d.dynamic([], lit, [1, 1], final=True, end=False)
    cases.append(("over_subscribed", M.zlib_wrap(d.finish() + bytes(8), raw), 4))
    parse = M.Tokens().lit(1, 2, 3)
    parse.tokens.append((3, 4))                                                 # one byte before the first
    parse.data += bytes(len(raw) - 3)
    cases.append(("distance_past_start", M.dynamic_stream(parse), 6))
    cases.append(("one_row_too_long", M.deflate(rows + [rows[0]]), 8))
    cases.append(("one_row_too_short", M.deflate(rows[:-1]), 8))
    bad_rows = list(rows)
    bad_rows[3] = b"\x05" + rows[3][1:]
    cases.append(("filter_type_5", M.deflate(bad_rows), 9))
    cases.append(("adler_byte_flipped", good[:-1] + bytes([good[-1] ^ 0x10]), 10))
    for name, stream, code in cases:
        assert decode_stream(stream, 5, 6, 2)[1] == code, (name, decode_stream(stream, 5, 6, 2)[1])
    return [(name, stream, header, code) for name, stream, code in cases], (good, header, pixels)


def _damage_batch():
    """Every damaged stream between two intact ones, and one more record whose source range lies past the buffer."""
    cases, (good, header, pixels) = _damage_cases()
    entries, codes = [(good, header, None)], [0]
    for _, stream, h, code in cases:
        entries += [(stream, h, None), (good, header, None)]
        codes += [code, 0]
    entries.append((good, header, None))
    codes.append(1)
    batch = P._pack(entries)
    batch.records["src_offset"][-1] = batch.data.numel() - 8                     # its src_len bytes end past the buffer
    return batch, codes, pixels, [c[0] for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the kernels' per-image code, compiled for the host under the sanitizers (a stand-alone program; nothing is
# preloaded and nothing is loaded into this process)
# ---------------------------------------------------------------------------------------------------------------------
MAGIC = 0x474e504444534142


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    source = os.path.join(ROOT, "tools", "png_host_check.cpp")
    out = str(tmp_path_factory.mktemp("png_host") / "png_host_check")
    compilers = [c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)]
    if not compilers:
        pytest.skip("no host C++ compiler found")
    errors = []
    # the sanitizers' runtimes linked statically where the compiler can (the program then stands alone), else as it links
    for cxx in compilers:
        for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
            done = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all", *static, "-o", out, source], capture_output=True,
                                  text=True)
            if done.returncode == 0:
                return out
            errors.append(f"{cxx} {' '.join(static)}: {done.stderr[-400:]}")
    pytest.fail("the sanitizer build of tools/png_host_check.cpp failed:\n" + "\n".join(errors))


def _run_host(program, batch: PngBatch, tmp_path, name):
    """(images as a list of (H, W, 3) arrays, per-image status, batch status) of the host program on ``batch``."""
    B = len(batch)
    src, dst = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}.out")
    with open(src, "wb") as f:
        f.write(np.array([MAGIC, B, batch.data.numel(), batch.out_bytes, batch.workspace_bytes, 0, 0, 0],
                         dtype="<i8").tobytes())
        f.write(batch.records.tobytes())
        f.write(batch.data.numpy().tobytes())
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint8)
    assert raw.size == batch.out_bytes + 4 * B + 4
    status = raw[batch.out_bytes:].view("<i4")
    images, at = [], 0
    for h, w in batch.sizes.tolist():
        images.append(raw[at:at + 3 * h * w].reshape(h, w, 3))
        at += 3 * h * w
    return images, status[:B].copy(), int(status[B])


def _word(codes) -> int:
    return int(np.bitwise_or.reduce([1 << (c - 1) for c in codes if c] + [0]))


def test_host_build_under_the_sanitizers(host_check, corpus, tmp_path):
    base = _inscope(corpus)
    images, status, word = _run_host(host_check, pack_pngs([d for d, _ in base.values()]), tmp_path, "corpus")
    assert word == 0 and not status.any()
    for got, (name, (_, rgb)) in zip(images, base.items()):
        assert np.array_equal(got, rgb), name
    # with the fallback's pixels as raw records among them
    mixed = list(corpus)
    batch = pack_pngs([corpus[n][0] for n in mixed], fallback=lambda data: next(
        rgb for s, rgb in corpus.values() if s == data))
    images, status, word = _run_host(host_check, batch, tmp_path, "mixed")
    assert word == 0 and batch.fallbacks == 4 and all(np.array_equal(g, corpus[n][1]) for g, n in zip(images, mixed))
    # every damaged stream of the zlib comparison: the restatement's status word, and zeros where it is not 0
    _, entries = _damaged(corpus)
    images, status, word = _run_host(host_check, P._pack(entries), tmp_path, "damaged")
    want = [decode_stream(s, h.width, h.height, h.color_type, plte) for s, h, plte in entries]
    assert status.tolist() == [code for _, code in want]
    assert word == _word(status.tolist()) and (status != 0).sum() > 300 and (status == 0).sum() > 3
    for i, (rgb, code) in enumerate(want):
        assert np.array_equal(images[i], rgb) and (code == 0 or not images[i].any()), i
    # filters, deflate structure and the damage cases of the GPU tests
    for name, cases in (("filters", _filter_cases()), ("structure", _structure_cases())):
        images, status, word = _run_host(host_check, pack_pngs([c[1] for c in cases]), tmp_path, name)
        assert word == 0 and not status.any(), (name, status.tolist())
        for got, (case, _, rgb) in zip(images, cases):
            assert np.array_equal(got, rgb), case
    batch, codes, pixels, _ = _damage_batch()
    images, status, word = _run_host(host_check, batch, tmp_path, "damage")
    assert status.tolist() == codes and word == _word(codes)
    for got, code in zip(images, codes):
        assert np.array_equal(got, pixels) if code == 0 else not got.any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _images(ragged: RaggedBatch):
    host = RaggedBatch(ragged.data.cpu(), ragged.sizes, 3)
    return [host.image(i).numpy() for i in range(len(host))]


@pytest.mark.gpu
def test_the_corpus_as_one_batch_positions_and_guard_bytes(dev, corpus):
    from basd_amd import _lib
    from basd_amd._launch import raw_stream
    base = _inscope(corpus)
    decoder = PngDecoder(dev)
    ragged = decoder(pack_pngs([d for d, _ in base.values()]).to(dev))
    assert isinstance(ragged, RaggedBatch) and ragged.channels == 3 and ragged.device.type == "cuda"
    assert decoder.status() == 0 and not decoder.image_status().any()
    for got, (name, (_, rgb)) in zip(_images(ragged), base.items()):
        assert np.array_equal(got, rgb), name
    # raw records among them
    mixed = list(corpus)
    batch = pack_pngs([corpus[n][0] for n in mixed], fallback=lambda data: next(
        rgb for s, rgb in corpus.values() if s == data))
    got = _images(decoder(batch.to(dev)))
    assert decoder.status() == 0 and batch.fallbacks == 4
    assert all(np.array_equal(g, corpus[n][1]) for g, n in zip(got, mixed))
    # one file alone and at three places of a batch
    data, rgb = base["RGBA_65x64_l1_ramp"]
    assert np.array_equal(_images(decoder(pack_pngs([data]).to(dev)))[0], rgb)
    others = [d for n, (d, _) in base.items() if "noise" in n][:6]
    files = [data] + others[:3] + [data] + others[3:] + [data]
    got = _images(decoder(pack_pngs(files).to(dev)))
    assert decoder.status() == 0
    for at in (0, 4, len(files) - 1):
        assert np.array_equal(got[at], rgb), at
    # guard bytes: the output is a slice of a larger buffer, and a small batch follows the large one in the workspace
    large = decoder.workspace.numel()
    names = ["P_8x7_plte20", "LA_8x7_l6_noise"]
    small = pack_pngs([base[n][0] for n in names]).to(dev)
    assert small.workspace_bytes < large // 4
    decoder.workspace.fill_(0x5A)
    guard = 256
    out = torch.full((small.out_bytes + 2 * guard,), 0xC3, dtype=torch.uint8, device=dev)
    table = torch.from_numpy(small.records.view(np.uint8).copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("basd_png_decode", small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard, small.out_bytes, 2,
              table.data_ptr(), decoder.workspace.data_ptr(), decoder.workspace.numel(), status.data_ptr(),
              small.max_filtered, small.max_pixels, raw_stream(dev.index))
    host, ws = out.cpu().numpy(), decoder.workspace.cpu().numpy()
    assert int(status.item()) == 0
    assert (host[:guard] == 0xC3).all() and (host[-guard:] == 0xC3).all()
    assert (ws[small.workspace_bytes:] == 0x5A).all() and (ws[16:128] == 0x5A).all() and not ws[:8].any()
    want = np.concatenate([base[n][1].reshape(-1) for n in names])
    assert np.array_equal(host[guard:-guard], want)
    ragged = decoder(small)
    assert decoder.workspace.numel() == large and decoder.used_bytes == small.workspace_bytes
    assert np.array_equal(ragged.data.cpu().numpy(), want)
    assert len(decoder(pack_pngs([]).to(dev))) == 0


@pytest.mark.gpu
def test_every_filter_type_at_the_band_boundaries(dev):
    cases = _filter_cases()
    decoder = PngDecoder(dev)
    got = _images(decoder(pack_pngs([c[1] for c in cases]).to(dev)))
    assert decoder.status() == 0 and len(cases) == 4 * 17 * 6 * 6
    for image, (name, _, rgb) in zip(got, cases):
        assert np.array_equal(image, rgb), name


@pytest.mark.gpu
def test_deflate_structure(dev):
    cases = _structure_cases()
    decoder = PngDecoder(dev)
    got = _images(decoder(pack_pngs([c[1] for c in cases]).to(dev)))
    assert decoder.image_status().tolist() == [0] * len(cases) and decoder.status() == 0
    for image, (name, _, rgb) in zip(got, cases):
        assert np.array_equal(image, rgb), name


@pytest.mark.gpu
def test_damaged_streams_are_reported_and_zeroed_between_intact_ones(dev):
    """Expected-error paths: the host build has run exactly this batch under the sanitizers
    (``test_host_build_under_the_sanitizers``)."""
    batch, codes, pixels, names = _damage_batch()
    decoder = PngDecoder(dev)
    got = _images(decoder(batch.to(dev)))
    assert decoder.image_status().tolist() == codes, list(zip(names, decoder.image_status().tolist()[1::2]))
    assert decoder.status() == _word(codes)
    for image, code in zip(got, codes):
        assert np.array_equal(image, pixels) if code == 0 else not image.any()


@pytest.mark.gpu
def test_launches_and_copies_do_not_depend_on_the_batch(dev, corpus):
    """Two launches and one copy (the record table) per call for B = 1 and for B = 9, no memset.  Counted with
    ``torch.profiler`` where it sees launches made through ctypes (the output says whether it does)."""
    from torch.profiler import ProfilerActivity, profile
    files = [d for d, _ in _inscope(corpus).values()]
    decoder = PngDecoder(dev)
    counts = {}
    for B in (9, 1):
        batch = pack_pngs(files[:B]).to(dev)
        for _ in range(5):
            decoder(batch)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(7):
                decoder(batch)
            torch.cuda.synchronize()
        device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
        host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
        copies = [e for e in device_events if "memcpy" in e.name.lower()]
        memsets = [e for e in device_events if "memset" in e.name.lower()]
        kernels = [e for e in device_events if e.name not in host_names and e not in copies and e not in memsets]
        ours = [e for e in kernels if "png_" in e.name]
        assert not memsets, sorted({e.name for e in memsets})
        counts[B] = (len(kernels), len(ours), len(copies))
        print(f"[png_decode] profiler, B = {B}: {len(kernels)} kernels ({len(ours)} of the decoder), {len(copies)} "
              "copies in 7 calls")
        if ours:
            assert len(ours) == 14 and len(kernels) == 14, sorted({e.name for e in kernels})
            assert len(copies) == 7 and not any("dtoh" in e.name.lower().replace(" ", "") for e in copies)
        else:
            assert not kernels and len(copies) in (0, 7)
    assert counts[1] == counts[9] and decoder.status() == 0


@pytest.mark.gpu
def test_trainer_and_evaluation_take_the_files_bytes(dev, corpus):
    from basd_amd import trainer as T
    from basd_amd.evaluation import evaluate_model
    from tools import stock_models as SM
    files, decoded = _trainer_files(corpus)
    ragged = pack_images(decoded)
    crops = draw_crop_params(ragged.sizes, generator=torch.Generator().manual_seed(2))
    student, teacher = _toy_models(dev)
    kw = dict(student_info=SM.probe_model(student, 16), mixup="fused", image_stats=STATS, resize_crop=True)
    tr = T.Trainer(student, _config(), teacher, png_decode=True, **kw)
    label = torch.arange(4) % 10
    got = tr.prepare_views({"images": pack_pngs(files), "label": label, "crop_params": crops})
    want = tr.prepare_views({"images": ragged, "label": label, "crop_params": crops})        # a RaggedBatch still works
    for g, w in zip(got, want):
        assert g.dtype == torch.uint8 and g.shape == (4, 3, 16, 16) and torch.equal(g, w)
    torch.manual_seed(77)
    assert torch.isfinite(tr.train_step({"images": pack_pngs(files), "label": label})["loss"])
    assert tr._png_decoder.status() == 0 and tr._resizer.status() == 0
    # prefetch=1 prepares the same bytes as prefetch=0 under a seed
    batches = [{"images": pack_pngs(files).pin_memory(), "label": label},
               {"images": pack_pngs(files[:2]).pin_memory(), "label": label[:2]},
               {"images": pack_pngs(files[::-1]).pin_memory(), "label": label}]
    prepared = {}
    for depth in (0, 1):
        t = T.Trainer(student, _config(), teacher, png_decode=True, trivial_augment=True, prefetch=depth, **kw)
        torch.manual_seed(11)
        copies = [{k: v.clone() for k, v in p.items()} for p in t._prefetcher.iterate(batches)]
        torch.cuda.synchronize()
        assert t._png_decoder.status() == 0
        prepared[depth] = [{k: v.cpu() for k, v in c.items()} for c in copies]
    assert len(prepared[0]) == 3
    for a, b in zip(prepared[0], prepared[1]):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    # validation: the same metrics from the bytes and from the decoded images
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    rc = ResizeCrop(16, 0.875, device=dev)
    ekw = dict(num_classes=10, image_stats=(MEAN, STD), resize_crop=rc)
    labels = [torch.tensor([1, 2, 3, 4]), torch.tensor([5, 6])]
    from_bytes = [{"images": pack_pngs(files), "label": labels[0]}, {"images": pack_pngs(files[:2]), "label": labels[1]}]
    from_pixels = [{"images": ragged, "label": labels[0]}, {"images": pack_images(decoded[:2]), "label": labels[1]}]
    decoder = PngDecoder(dev)
    got = evaluate_model(student, from_bytes, criterion, png_decode=decoder, **ekw)
    assert got == evaluate_model(student, from_pixels, criterion, **ekw) and np.isfinite(got["loss"])
    assert decoder.status() == 0 and got == tr.evaluate(student, from_bytes)
