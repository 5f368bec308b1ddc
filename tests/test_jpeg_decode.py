"""``basd_amd.jpeg``: baseline JPEG decoding on the device, byte for byte Pillow's.

The chain of evidence: ``decode_reference`` (the specification of ``include/basd_hip.h`` in numpy) equals Pillow on
live random streams and on the recorded corpus; the per-image code of the kernels (``csrc/jpeg_core.h``), compiled for
the host under the sanitizers, equals the recorded bytes and survives every prefix and every corrupted scan byte of
the two smallest streams; the kernels equal both on the GPU.  Every comparison is ``array_equal``.
"""
import importlib.util
import io
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import jpeg as J
from basd_amd.jpeg import (JpegBatch, JpegDecoder, UnsupportedJpeg, collate_jpeg, decode_reference, pack_jpegs,
                           parse_jpeg)
from basd_amd.resize import RaggedBatch, ResizeCrop, draw_crop_params, pack_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
PNG = b"\x89PNG\r\n\x1a\n" + bytes(32)


@pytest.fixture(scope="module")
def corpus():
    """name -> (stream bytes, Pillow's RGB), in the file's order."""
    g = np.load(GOLDEN, allow_pickle=False)
    return {str(n): (g[f"stream_{n}"].tobytes(), g[f"rgb_{n}"]) for n in g["names"]}


def _baseline(corpus):
    return {n: v for n, v in corpus.items() if not n.startswith("fallback_")}


def _maker():
    spec = importlib.util.spec_from_file_location("make_goldens_jpeg_decode",
                                                  os.path.join(ROOT, "tests", "golden", "make_goldens_jpeg_decode.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against Pillow
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow():
    """320 seeded random streams up to 48 px from the corpus's option grid, widths and heights 1..6 among them."""
    pytest.importorskip("PIL")
    M = _maker()
    rng = np.random.default_rng(7)
    modes, seen = ("gray", "444", "422", "420"), set()
    for n in range(320):
        small = n % 4 == 0
        w, h = (int(rng.integers(1, 7)), int(rng.integers(1, 7))) if small else \
            (int(rng.integers(1, 49)), int(rng.integers(1, 49)))
        if n % 16 == 2:
            w = int(rng.integers(1, 7))
        mode, quality = modes[int(rng.integers(0, 4))], (1, 30, 75, 90, 100)[int(rng.integers(0, 5))]
        options = dict(quality=quality)
        if mode != "gray":
            options["subsampling"] = M.SUBSAMPLING[mode]
        extra = int(rng.integers(0, 6))
        if extra == 1:
            options["optimize"] = True
        elif extra == 2:
            options["restart_marker_blocks"] = int(rng.integers(1, 4))
        elif extra == 3:
            options["restart_marker_rows"] = 1
        stream = M.encode(M.picture(rng, h, w, ("noise", "ramp")[n % 2], mode == "gray"), **options)
        header = parse_jpeg(stream)
        assert header.reason is None, (n, w, h, mode, options, header.reason)
        assert np.array_equal(decode_reference(stream), M.decode(stream)), (n, w, h, mode, options)
        seen.add((mode, extra, small))
    assert len(seen) > 40


def test_restatement_equals_the_recorded_pillow_outputs(corpus):
    assert os.path.getsize(GOLDEN) < 256 * 1024 and 30 <= len(corpus) <= 60
    base = _baseline(corpus)
    for name, (stream, rgb) in base.items():
        assert np.array_equal(decode_reference(stream), rgb), name
    sides = {s for _, rgb in base.values() for s in rgb.shape[:2]}
    assert {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33} <= sides
    for word in ("gray", "444", "422", "420", "q1_", "q75", "q100", "_opt", "rst1", "rst2", "rstrow", "noise", "ramp"):
        assert any(word in name for name in base), word
    # the same picture with and without restart intervals
    for mode in ("gray", "444", "422", "420"):
        same = [rgb for name, (_, rgb) in base.items() if name.startswith(mode) and ("_rst" in name or "_plain" in name)]
        assert len(same) == 4 and all(np.array_equal(same[0], other) for other in same[1:])


def _with_adobe(stream: bytes) -> bytes:
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    return stream[:2] + app14 + stream[2:]


def _with_wide_table(stream: bytes) -> bytes:
    """The first DQT segment rewritten with 16-bit entries (what a 12-bit stream carries)."""
    at = stream.index(b"\xff\xdb")
    length = (stream[at + 2] << 8) | stream[at + 3]
    body = stream[at + 4:at + 2 + length]
    wide = b""
    for t in range(len(body) // 65):
        wide += bytes([0x10 | body[65 * t]]) + b"".join(bytes([0, v]) for v in body[65 * t + 1:65 * t + 65])
    return stream[:at + 2] + (len(wide) + 2).to_bytes(2, "big") + wide + stream[at + 2 + length:]


def test_parse_classifies_what_the_device_does_not_decode(corpus):
    good = corpus["420_33x31_q75_plain"][0]
    header = parse_jpeg(good)
    assert header.reason is None and (header.width, header.height, header.ncomp, header.hs, header.vs) == (33, 31, 3, 2, 2)
    assert header.segments == (header.scan_offset,) and header.restart == 0 and header.blocks == 6 * 6
    assert good[header.scan_offset - 14:header.scan_offset - 12] == b"\xff\xda"
    restarts = parse_jpeg(corpus["420_33x31_q75_rst1"][0])
    assert restarts.restart == 1 and len(restarts.segments) == 6
    assert all(corpus["420_33x31_q75_rst1"][0][s - 2:s] == bytes([0xFF, 0xD0 + i]) for i, s in
               enumerate(restarts.segments[1:]))
    gray = parse_jpeg(corpus["gray_17x9_q75_plain"][0])
    assert gray.reason is None and (gray.ncomp, gray.hs, gray.vs, gray.blocks) == (1, 1, 1, 6)
    for stream, reason in ((corpus["fallback_progressive"][0], "progressive"), (corpus["fallback_cmyk"][0], "CMYK"),
                           (_with_adobe(good), "Adobe APP14"), (_with_wide_table(good), "16-bit quantisation table"),
                           (PNG, "not a JPEG stream"), (b"", "not a JPEG stream"), (good[:40], "truncated header"),
                           (good[:header.scan_offset - 14], "no scan")):
        assert reason in parse_jpeg(stream).reason, (reason, parse_jpeg(stream).reason)
    with pytest.raises(ValueError, match="not in the device's scope: not baseline: progressive"):
        decode_reference(corpus["fallback_progressive"][0])
    # the limit on the sides names the value
    wide = bytearray(good)
    sof = good.index(b"\xff\xc0")
    wide[sof + 5:sof + 9] = (J.MAX_SIDE + 1).to_bytes(2, "big") + (40).to_bytes(2, "big")
    assert f"40 x {J.MAX_SIDE + 1} pixels" in parse_jpeg(bytes(wide)).reason


def test_pack_layout_fallback_and_collate(corpus):
    names = ["420_33x31_q75_rst2", "fallback_cmyk", "gray_17x9_q75_plain"]
    files = [corpus[n][0] for n in names]
    calls = []

    def fallback(data):
        calls.append(data)
        return corpus["fallback_cmyk"][1]

    batch = pack_jpegs(files, fallback=fallback)
    assert calls == [files[1]] and isinstance(batch, JpegBatch) and len(batch) == 3 and batch.fallbacks == 1
    assert batch.data.dtype == torch.uint8 and batch.data.numel() % 16 == 0
    assert batch.sizes.tolist() == [[31, 33], [9, 15], [9, 17]] and batch.out_bytes == 3 * (31 * 33 + 9 * 15 + 9 * 17)
    rec, data = batch.records, batch.data.numpy()
    assert rec.dtype == J.RECORD_DTYPE and rec.dtype.itemsize == 128
    assert rec["kind"].tolist() == [0, 1, 0] and rec["out_offset"].tolist() == [0, 3 * 31 * 33, 3 * (31 * 33 + 9 * 15)]
    for i in (0, 2):
        at, n = int(rec["src_offset"][i]), int(rec["src_len"][i])
        assert data[at:at + n].tobytes() == files[i]
        header = parse_jpeg(files[i])
        seg = data[int(rec["seg_offset"][i]):int(rec["seg_offset"][i]) + 4 * int(rec["n_seg"][i])].view(np.int32)
        assert rec["seg_offset"][i] % 4 == 0 and tuple(seg.tolist()) == header.segments
        assert tuple(rec["quant"][i][:header.ncomp]) == header.quant and rec["restart"][i] == header.restart
    at = int(rec["src_offset"][1])
    assert np.array_equal(data[at:at + 9 * 15 * 3].reshape(9, 15, 3), corpus["fallback_cmyk"][1])
    # the workspace: the status words, then 128 + 64 bytes per block, image after image
    assert J.status_bytes(3) == 128 and rec["coef_offset"].tolist() == [128, 0, 128 + 192 * 36]
    assert rec["plane_offset"].tolist() == [128 + 128 * 36, 0, 128 + 192 * 36 + 128 * 6]
    assert batch.workspace_bytes == 128 + 192 * 42 and batch.max_blocks == 36 and batch.max_pixels == 31 * 33
    # without a fallback the image is named
    saved, J._default_fallback = J._default_fallback, lambda: None
    try:
        with pytest.raises(UnsupportedJpeg, match=r"image 1 .*CMYK.*no fallback") as e:
            pack_jpegs(files)
    finally:
        J._default_fallback = saved
    assert e.value.index == 1 and "CMYK" in e.value.reason
    with pytest.raises(ValueError, match=r"fallback of image 1 must return an \(H, W, 3\) uint8"):
        pack_jpegs(files, fallback=lambda data: np.zeros((4, 4), dtype=np.uint8))
    with pytest.raises(TypeError, match="image 0 must be the bytes of a file"):
        pack_jpegs([np.zeros(4)])
    empty = pack_jpegs([])
    assert len(empty) == 0 and empty.data.numel() == 0 and empty.out_bytes == 0
    # collate_jpeg: bytes, or the dict a dataset column of undecoded images yields
    out = collate_jpeg([{"image": files[0], "label": 3}, {"image": {"bytes": files[2], "path": None}, "label": 5}])
    assert isinstance(out["images"], JpegBatch) and len(out["images"]) == 2 and out["label"].tolist() == [3, 5]
    with pytest.raises(KeyError, match="needs an 'image' entry"):
        collate_jpeg([{"label": 1}])
    pinned = out["images"].to("cpu")
    assert pinned is out["images"]


def test_default_fallback_is_pillow(corpus):
    pytest.importorskip("PIL")
    batch = pack_jpegs([corpus["fallback_progressive"][0], PNG_IMAGE()])
    assert batch.fallbacks == 2 and batch.sizes.tolist() == [[9, 15], [3, 5]]
    at = int(batch.records["src_offset"][0])
    assert np.array_equal(batch.data.numpy()[at:at + 9 * 15 * 3].reshape(9, 15, 3), corpus["fallback_progressive"][1])


def PNG_IMAGE() -> bytes:
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(np.arange(45, dtype=np.uint8).reshape(3, 5, 3)).save(out, format="PNG")
    return out.getvalue()


def test_exported_from_the_package():
    import basd_amd
    from basd_amd import _lib
    assert "``jpeg``" in basd_amd.__doc__
    for name in ("JpegBatch", "JpegDecoder", "UnsupportedJpeg", "collate_jpeg", "decode_reference", "pack_jpegs",
                 "parse_jpeg"):
        assert name in basd_amd.__all__ and getattr(basd_amd, name) is getattr(J, name)
    vp, i32, i64 = _lib.vp, _lib.i32, _lib.i64
    assert _lib.SIGNATURES["basd_jpeg_decode"] == [vp, i64, vp, i64, i32, vp, vp, i64, vp, i64, i64, vp]
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    for text in ("int basd_jpeg_decode(", "BasdJpegRecord", f"#define BASD_JPEG_MAX_SIDE {J.MAX_SIDE}",
                 f"#define BASD_JPEG_MAX_BATCH {J.MAX_BATCH}", "(x + 2^17) >> 18", "F(1.402)"):
        assert text in header, text
    assert J.MAX_SIDE >= 4096


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
TRAINER_STREAMS = ("420_33x31_q75_rst1", "444_33x17_q75_plain", "422_31x33_q75_rstrow", "420_64x96_q100_noise")


def _trainer_files(corpus):
    return [corpus[n][0] for n in TRAINER_STREAMS], [corpus[n][1] for n in TRAINER_STREAMS]


def test_trainer_and_evaluation_argument_errors_on_cpu(corpus):
    from basd_amd import trainer as T
    from basd_amd.evaluation import evaluate_model
    from tools import stock_models as SM
    student, teacher = _toy_models()
    kw = dict(student_info=SM.probe_model(student, 16), loss_cls=OracleBASD)
    with pytest.raises(ValueError, match="jpeg_decode needs resize_crop=True"):
        T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, jpeg_decode=True, **kw)
    tr = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, resize_crop=True, jpeg_decode=True,
                   **kw)
    assert isinstance(tr._decoder, JpegDecoder)
    files, _ = _trainer_files(corpus)
    batch = pack_jpegs(files)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.prepare_views({"images": batch, "label": torch.arange(4)})
    with pytest.raises(TypeError, match="resize_crop.*RaggedBatch"):
        tr.prepare_views({"images": files, "label": torch.arange(4)})
    # the default is unchanged: no decoder, and a JpegBatch is not taken
    plain = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, resize_crop=True, **kw)
    assert plain._decoder is None
    with pytest.raises(TypeError, match="resize_crop.*RaggedBatch"):
        plain.prepare_views({"images": batch, "label": torch.arange(4)})
    criterion = nn.CrossEntropyLoss()
    with pytest.raises(ValueError, match="jpeg_decode needs resize_crop"):
        evaluate_model(student, [], criterion, num_classes=10, image_stats=(MEAN, STD), jpeg_decode=JpegDecoder("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_model(student, [{"images": batch, "label": torch.arange(4)}], criterion, num_classes=10,
                       image_stats=(MEAN, STD), resize_crop=ResizeCrop(16, 0.875, device="cpu"),
                       jpeg_decode=JpegDecoder("cpu"))
    with pytest.raises(TypeError, match="batch must be a JpegBatch"):
        JpegDecoder("cpu")(pack_images([np.zeros((4, 4, 3), dtype=np.uint8)]))
    bad = pack_jpegs(files[:1])
    bad.records["width"][0] = J.MAX_SIDE + 1
    with pytest.raises(ValueError, match=f"image 0 has width {J.MAX_SIDE + 1}"):
        JpegDecoder("cpu")(bad)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the kernels' per-image code, compiled for the host under the sanitizers (a stand-alone program; nothing is
# preloaded and nothing is loaded into this process)
# ---------------------------------------------------------------------------------------------------------------------
MAGIC = 0x4745504a44534142


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    source = os.path.join(ROOT, "tools", "jpeg_host_check.cpp")
    out = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_host_check")
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
    pytest.fail("the sanitizer build of tools/jpeg_host_check.cpp failed:\n" + "\n".join(errors))


def _run_host(program, batch: JpegBatch, tmp_path, name):
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


def _damaged(corpus):
    """Per variant (bytes, header of the whole stream): every prefix of the two smallest streams, and those streams
    with each scan byte replaced by 0x00, by 0xFF and by its complement."""
    base = _baseline(corpus)
    smallest = sorted(base, key=lambda n: (len(base[n][0]), n))[:2]
    entries = []
    for name in smallest:
        stream = base[name][0]
        header = parse_jpeg(stream)
        entries += [(stream[:n], header) for n in range(len(stream))]
        for at in range(header.scan_offset, len(stream)):
            for value in (0x00, 0xFF, stream[at] ^ 0xFF):
                entries.append((stream[:at] + bytes([value]) + stream[at + 1:], header))
    return smallest, entries


def test_host_build_under_the_sanitizers(host_check, corpus, tmp_path):
    base = _baseline(corpus)
    images, status, word = _run_host(host_check, pack_jpegs([s for s, _ in base.values()]), tmp_path, "corpus")
    assert word == 0 and not status.any()
    for got, (name, (_, rgb)) in zip(images, base.items()):
        assert np.array_equal(got, rgb), name
    # with the fallback's pixels as raw records among them
    mixed = list(corpus)
    batch = pack_jpegs([corpus[n][0] for n in mixed], fallback=lambda data: next(
        rgb for s, rgb in corpus.values() if s == data))
    images, status, word = _run_host(host_check, batch, tmp_path, "mixed")
    assert word == 0 and batch.fallbacks == 2 and all(np.array_equal(g, corpus[n][1]) for g, n in zip(images, mixed))
    # damaged streams under the whole stream's header: each decodes or reports an error, and then is all zero
    smallest, entries = _damaged(corpus)
    assert len(entries) > 600
    images, status, word = _run_host(host_check, J._pack(entries), tmp_path, "damaged")
    assert set(status.tolist()) <= set(J.STATUS_NAMES) and word == int(np.bitwise_or.reduce(
        [1 << (s - 1) for s in status.tolist() if s] + [0]))
    failed = status != 0
    assert failed.sum() > 300 and (~failed).sum() > 10
    assert all(not images[i].any() for i in np.flatnonzero(failed))
    # a prefix that cuts the header or the scan short fails; the whole stream less its EOI marker still decodes
    at = 0
    for name in smallest:
        stream, rgb = base[name]
        header = parse_jpeg(stream)
        n = len(stream)
        assert status[at:at + header.scan_offset + 1].all(), name
        assert status[at + n - 2] == 0 and np.array_equal(images[at + n - 2], rgb), name
        at += n + 3 * (n - header.scan_offset)
    assert at == len(entries)


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


def _lookup(corpus):
    return lambda data: next(rgb for s, rgb in corpus.values() if s == data)


@pytest.mark.gpu
def test_the_corpus_as_one_batch(dev, corpus):
    base = _baseline(corpus)
    decoder = JpegDecoder(dev)
    ragged = decoder(pack_jpegs([s for s, _ in base.values()]).to(dev))
    assert isinstance(ragged, RaggedBatch) and ragged.channels == 3 and ragged.device.type == "cuda"
    assert decoder.status() == 0 and not decoder.image_status().any()
    for got, (name, (stream, rgb)) in zip(_images(ragged), base.items()):
        assert np.array_equal(got, rgb), name
        assert np.array_equal(got, decode_reference(stream)), name


@pytest.mark.gpu
def test_one_image_and_positions_in_a_batch(dev, corpus):
    base = _baseline(corpus)
    decoder = JpegDecoder(dev)
    for name in ("420_64x96_q100_noise", "444_72x72_q75_81segments", "gray_1x7_q1_noise"):
        stream, rgb = base[name]
        assert np.array_equal(_images(decoder(pack_jpegs([stream]).to(dev)))[0], rgb), name
    stream, rgb = base["444_72x72_q75_81segments"]                 # 81 segments: more than the lanes of the workgroup
    assert len(parse_jpeg(stream).segments) == 81
    others = [s for n, (s, _) in base.items() if "q1_" in n][:6]
    files = [stream] + others[:3] + [stream] + others[3:] + [stream]
    got = _images(decoder(pack_jpegs(files).to(dev)))
    assert decoder.status() == 0
    for at in (0, 4, len(files) - 1):
        assert np.array_equal(got[at], rgb), at
    # restart intervals do not change the picture
    for mode in ("gray", "444", "422", "420"):
        same = [s for n, (s, _) in base.items() if n.startswith(mode) and ("_rst" in n or "_plain" in n)]
        got = _images(decoder(pack_jpegs(same).to(dev)))
        assert len(got) == 4 and all(np.array_equal(got[0], other) for other in got[1:]), mode


@pytest.mark.gpu
def test_guard_bytes_and_the_workspace_past_its_used_part(dev, corpus):
    """The output is a slice of a larger buffer filled with a pattern, and a small batch follows a large one in the
    same decoder: the bytes around the output and the workspace behind the small batch's part keep their values."""
    from basd_amd import _lib
    from basd_amd._launch import raw_stream
    base = _baseline(corpus)
    decoder = JpegDecoder(dev)
    decoder(pack_jpegs([s for s, _ in base.values()]).to(dev))
    large = decoder.used_bytes
    assert decoder.workspace.numel() == large
    small = pack_jpegs([base["420_33x31_q75_rst1"][0], base["gray_17x9_q75_plain"][0]]).to(dev)
    assert small.workspace_bytes < large // 4
    decoder.workspace.fill_(0x5A)
    guard = 256
    out = torch.full((small.out_bytes + 2 * guard,), 0xC3, dtype=torch.uint8, device=dev)
    table = torch.from_numpy(small.records.view(np.uint8).copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("basd_jpeg_decode", small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard, small.out_bytes, 2,
              table.data_ptr(), decoder.workspace.data_ptr(), decoder.workspace.numel(), status.data_ptr(),
              small.max_blocks, small.max_pixels, raw_stream(dev.index))
    host, ws = out.cpu().numpy(), decoder.workspace.cpu().numpy()
    assert int(status.item()) == 0
    assert (host[:guard] == 0xC3).all() and (host[-guard:] == 0xC3).all()
    assert (ws[small.workspace_bytes:] == 0x5A).all() and (ws[8:128] == 0x5A).all() and not ws[:8].any()
    want = np.concatenate([base["420_33x31_q75_rst1"][1].reshape(-1), base["gray_17x9_q75_plain"][1].reshape(-1)])
    assert np.array_equal(host[guard:-guard], want)
    # the decoder itself keeps the larger workspace for the smaller batch
    ragged = decoder(small)
    assert decoder.workspace.numel() == large and decoder.used_bytes == small.workspace_bytes
    assert np.array_equal(ragged.data.cpu().numpy(), want)


@pytest.mark.gpu
def test_fallback_images_travel_as_raw_records(dev, corpus):
    names = ["422_31x33_q75_rst2", "fallback_progressive", "gray_17x9_q75_plain", "fallback_cmyk", "420_33x31_q75_plain"]
    batch = pack_jpegs([corpus[n][0] for n in names], fallback=_lookup(corpus))
    assert batch.records["kind"].tolist() == [0, 1, 0, 1, 0]
    decoder = JpegDecoder(dev)
    got = _images(decoder(batch.to(dev)))
    assert decoder.status() == 0
    for image, name in zip(got, names):
        assert np.array_equal(image, corpus[name][1]), name
    # a batch of raw records alone
    only = pack_jpegs([corpus["fallback_cmyk"][0]], fallback=_lookup(corpus))
    assert only.max_blocks == 0 and np.array_equal(_images(decoder(only.to(dev)))[0], corpus["fallback_cmyk"][1])


@pytest.mark.gpu
def test_a_truncated_stream_between_two_good_ones(dev, corpus):
    """The cut stream is a prefix the sanitizer run of the host build has been through (every prefix of the two
    smallest streams is)."""
    base = _baseline(corpus)
    name = sorted(base, key=lambda n: (len(base[n][0]), n))[0]
    stream = base[name][0]
    header = parse_jpeg(stream)
    cut = stream[:(header.scan_offset + len(stream)) // 2]
    entries = [(base["420_33x31_q75_rst1"][0], parse_jpeg(base["420_33x31_q75_rst1"][0])), (cut, header),
               (base["444_33x17_q75_plain"][0], parse_jpeg(base["444_33x17_q75_plain"][0]))]
    decoder = JpegDecoder(dev)
    got = _images(decoder(J._pack(entries).to(dev)))
    per_image = decoder.image_status().tolist()
    assert per_image[0] == 0 and per_image[2] == 0 and per_image[1] == 3, per_image          # BASD_JPEG_TRUNCATED
    assert decoder.status() == 1 << 2
    assert got[1].shape == base[name][1].shape and not got[1].any()
    assert np.array_equal(got[0], base["420_33x31_q75_rst1"][1]) and np.array_equal(got[2], base["444_33x17_q75_plain"][1])
    # a wrong restart marker, and a record whose table offsets point past its stream
    rst = bytearray(base["420_33x31_q75_rst1"][0])
    seg = parse_jpeg(bytes(rst)).segments
    rst[seg[2] - 1] = 0xD5
    bad = J._pack([(bytes(rst), parse_jpeg(base["420_33x31_q75_rst1"][0])), (stream[:40], header)])
    fresh = JpegDecoder(dev)
    got = _images(fresh(bad.to(dev)))
    assert fresh.image_status().tolist() == [5, 1] and fresh.status() == (1 << 4) | 1 and not got[0].any() \
        and not got[1].any()


@pytest.mark.gpu
def test_launches_and_copies_do_not_depend_on_the_batch(dev, corpus):
    """Three launches and one copy (the record table) per call for B = 1 and for B = 9, no memset.  Counted with
    ``torch.profiler`` where it sees launches made through ctypes (the output says whether it does)."""
    from torch.profiler import ProfilerActivity, profile
    base = _baseline(corpus)
    files = [s for s, _ in base.values()]
    decoder = JpegDecoder(dev)
    counts = {}
    for B in (9, 1):
        batch = pack_jpegs(files[:B]).to(dev)
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
        ours = [e for e in kernels if "jpeg_" in e.name]
        assert not memsets, sorted({e.name for e in memsets})
        counts[B] = (len(kernels), len(ours), len(copies))
        print(f"[jpeg_decode] profiler, B = {B}: {len(kernels)} kernels ({len(ours)} of the decoder), {len(copies)} "
              "copies in 7 calls")
        if ours:
            assert len(ours) == 21 and len(kernels) == 21, sorted({e.name for e in kernels})
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
    for stream, rgb in zip(files, decoded):
        assert np.array_equal(decode_reference(stream), rgb)
    ragged = pack_images(decoded)
    crops = draw_crop_params(ragged.sizes, generator=torch.Generator().manual_seed(2))
    student, teacher = _toy_models(dev)
    kw = dict(student_info=SM.probe_model(student, 16), mixup="fused", image_stats=STATS, resize_crop=True)
    tr = T.Trainer(student, _config(), teacher, jpeg_decode=True, **kw)
    label = torch.arange(4) % 10
    got = tr.prepare_views({"images": pack_jpegs(files), "label": label, "crop_params": crops})
    want = tr.prepare_views({"images": ragged, "label": label, "crop_params": crops})       # a RaggedBatch still works
    plain = T.Trainer(student, _config(), teacher, **kw).prepare_views({"images": ragged, "label": label,
                                                                        "crop_params": crops})
    for g, w, p in zip(got, want, plain):
        assert g.dtype == torch.uint8 and g.shape == (4, 3, 16, 16) and torch.equal(g, w) and torch.equal(g, p)
    torch.manual_seed(77)
    assert torch.isfinite(tr.train_step({"images": pack_jpegs(files), "label": label})["loss"])
    assert tr._decoder.status() == 0 and tr._resizer.status() == 0
    # validation: the same metrics from the bytes and from the decoded images
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    rc = ResizeCrop(16, 0.875, device=dev)
    ekw = dict(num_classes=10, image_stats=(MEAN, STD), resize_crop=rc)
    labels = [torch.tensor([1, 2, 3, 4]), torch.tensor([5, 6])]
    from_bytes = [{"images": pack_jpegs(files), "label": labels[0]}, {"images": pack_jpegs(files[:2]), "label": labels[1]}]
    from_pixels = [{"images": ragged, "label": labels[0]}, {"images": pack_images(decoded[:2]), "label": labels[1]}]
    decoder = JpegDecoder(dev)
    got = evaluate_model(student, from_bytes, criterion, jpeg_decode=decoder, **ekw)
    assert got == evaluate_model(student, from_pixels, criterion, **ekw) and np.isfinite(got["loss"])
    assert got == evaluate_model(student, from_bytes[:1] + from_pixels[1:], criterion, jpeg_decode=decoder, **ekw)
    assert decoder.status() == 0 and got == tr.evaluate(student, from_bytes)
