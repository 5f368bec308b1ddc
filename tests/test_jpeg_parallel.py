"""``JpegDecoder(entropy="parallel")`` / ``basd_jpeg_decode_parallel``: the entropy stage that decodes inside a segment
with a workgroup's lanes gives the serial stage's bytes and status words.

The chain of evidence: the new streams' recorded pixels are Pillow's and ``decode_reference``'s; the lanes' passes
(``csrc/jpeg_core.h``), run lane after lane by ``tools/jpeg_parallel_host_check.cpp`` under the sanitizers, equal the
recorded bytes and, on every prefix and every corrupted scan byte of the two smallest streams, the serial host
program's status words and bytes; the kernel equals the recorded bytes and the serial kernels on the GPU.  Every
comparison is ``array_equal``.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import jpeg as J
from basd_amd.jpeg import JpegBatch, JpegDecoder, decode_reference, pack_jpegs, parse_jpeg
from basd_amd.resize import RaggedBatch, ResizeCrop, draw_crop_params, pack_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
NEW = os.path.join(ROOT, "tests", "golden", "jpeg_parallel.npz")
MAGIC = 0x4745504a44534142
DEFAULT_LANES, DEFAULT_SUB_BYTES = 256, 128
# streams whose last block crosses byte `boundary` of the entropy-coded data: 1024 = 64 x 16, 32768 = 256 x 128 = 8 x 256 x 16
BOUNDARIES = {"gray_64x47_q90_across1024": 1024, "gray_276x208_q98_across32768": 32768}                     # kJpegParLanes, kJpegParSubBytes of csrc/jpeg.hip


def _load(path):
    g = np.load(path, allow_pickle=False)
    return {str(n): (g[f"stream_{n}"].tobytes(), g[f"rgb_{n}"]) for n in g["names"]}


@pytest.fixture(scope="module")
def old():
    """The corpus of tests/test_jpeg_decode.py: name -> (stream bytes, Pillow's RGB)."""
    return _load(OLD)


@pytest.fixture(scope="module")
def new():
    return _load(NEW)


@pytest.fixture(scope="module")
def both(old, new):
    """The old corpus's baseline streams, then the new ones."""
    streams = {n: v for n, v in old.items() if not n.startswith("fallback_")}
    streams.update(new)
    return streams


def _segment_lengths(stream):
    header = parse_jpeg(stream)
    starts = list(header.segments) + [len(stream) + 2]
    return [b - 2 - a for a, b in zip(starts, starts[1:])]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_parallel_stage_needs(new):
    assert os.path.getsize(NEW) < 400 * 1024
    for name, (stream, rgb) in new.items():
        assert parse_jpeg(stream).reason is None, name
        assert np.array_equal(decode_reference(stream), rgb), name
    try:
        from PIL import Image  # noqa: F401
    except ImportError:
        pass
    else:
        for name, (stream, rgb) in new.items():
            assert np.array_equal(J.pillow_fallback(stream), rgb), name
    chunk = DEFAULT_LANES * DEFAULT_SUB_BYTES
    noise, header = new["444_160x160_q100_noise"][0], parse_jpeg(new["444_160x160_q100_noise"][0])
    assert (header.width, header.height, header.hs, header.vs, len(header.segments)) == (160, 160, 1, 1, 1)
    assert len(noise) - header.scan_offset > 3 * chunk and noise.count(b"\xff\x00") > 500
    assert (len(noise) - header.scan_offset) / header.blocks > 6 * 16      # a mean block spans seven of 16 bytes
    for name, shape, ncomp in (("gray_256x256_flat", (256, 256, 3), 1), ("420_256x256_flat", (256, 256, 3), 3)):
        stream, rgb = new[name]
        assert rgb.shape == shape and parse_jpeg(stream).ncomp == ncomp and (rgb == rgb[0, 0]).all(), name
    ramp = parse_jpeg(new["420_160x120_q90_ramp"][0])
    assert (ramp.width, ramp.height, ramp.hs, ramp.vs) == (160, 120, 2, 2)
    rows = parse_jpeg(new["422_256x24_q100_rstrow"][0])
    assert (rows.hs, rows.vs, rows.restart, len(rows.segments)) == (2, 1, 16, 3)
    assert min(_segment_lengths(new["422_256x24_q100_rstrow"][0])) > DEFAULT_LANES * 16    # a chunk at sub_bytes=16
    assert any(max(rgb.shape[:2]) <= 7 for _, rgb in new.values())
    # the last block of these two begins before a chunk's end and ends behind it (the generator checks where it begins)
    for name, boundary in BOUNDARIES.items():
        header = parse_jpeg(new[name][0])
        ends = len(new[name][0]) - 2 - header.scan_offset
        assert header.ncomp == 1 and len(header.segments) == 1 and boundary < ends <= boundary + 20, (name, ends)


class OracleBASD(nn.Module):
    """The oracle behind the reference constructor's signature (test-side stand-in for the loss module on CPU)."""

    def __init__(self, base_criterion, student_dim, teacher_dim, student_depth, num_student_tokens, *, config,
                 teacher_has_cls_token):
        super().__init__()
        from oracle import basd_oracle as O
        self.token_layers = O.extraction_layers(student_depth, config.num_extraction_points)
        st = O.SelectorState.create(len(self.token_layers), student_dim, teacher_dim)
        self.log_temperatures = nn.Parameter(st.log_temperatures.detach().clone())


def _config():
    from types import SimpleNamespace
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=4),
                           model=SimpleNamespace(num_classes=10, vit=SimpleNamespace(img_size=16)),
                           data=SimpleNamespace(eval_crop_ratio=0.875))


def _toy_models(dev="cpu"):
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=16, patch_size=4, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.StockViT(img_size=16, patch_size=4, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    return student, SM.make_teacher(teacher, 16)


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STATS = {"clean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "augmented": (MEAN, STD)}


def test_argument_errors_and_what_is_exported():
    from basd_amd import _lib
    from basd_amd import trainer as T
    from tools import stock_models as SM
    assert JpegDecoder("cpu").entropy == "serial" and JpegDecoder("cpu").sub_bytes is None
    assert JpegDecoder("cpu", entropy="parallel").entropy == "parallel"
    assert JpegDecoder("cpu", "parallel", sub_bytes=16).sub_bytes == 16
    with pytest.raises(ValueError, match="entropy must be one of 'serial', 'parallel'"):
        JpegDecoder("cpu", entropy="speculative")
    with pytest.raises(ValueError, match='sub_bytes belongs to entropy="parallel"'):
        JpegDecoder("cpu", sub_bytes=64)
    for bad in (12, 0, J.SUB_BYTES_MAX + 8, 64.0, True):
        with pytest.raises(ValueError, match=f"sub_bytes must be a multiple of 8 in {J.SUB_BYTES_MIN} .. {J.SUB_BYTES_MAX}"):
            JpegDecoder("cpu", entropy="parallel", sub_bytes=bad)
    assert J.SUB_BYTES_MIN <= 16 and DEFAULT_SUB_BYTES % 8 == 0
    assert "``entropy``" in JpegDecoder.__doc__ and '"parallel"' in JpegDecoder.__doc__
    vp, i32, i64 = _lib.vp, _lib.i32, _lib.i64
    assert _lib.SIGNATURES["basd_jpeg_decode_parallel"] == [vp, i64, vp, i64, i32, vp, vp, i64, vp, i64, i64, i32, vp]
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    for text in ("int basd_jpeg_decode_parallel(", f"#define BASD_JPEG_SUB_BYTES_MIN {J.SUB_BYTES_MIN}",
                 f"#define BASD_JPEG_SUB_BYTES_MAX {J.SUB_BYTES_MAX}", f"AT MOST {DEFAULT_LANES // 4 + 2} rounds",
                 f"(the built-in default, {DEFAULT_SUB_BYTES})", "the same per-image status word and the same\n * bytes"):
        assert text in header, text
    with open(os.path.join(ROOT, "vit-inductive-bias-distillation_amd", "csrc", "jpeg.hip")) as f:
        kernel = f.read()
    assert f"#define BASD_JPEG_PAR_LANES {DEFAULT_LANES} " in kernel
    assert f"constexpr int kJpegParSubBytes = {DEFAULT_SUB_BYTES};" in kernel
    # the trainer
    student, teacher = _toy_models()
    kw = dict(student_info=SM.probe_model(student, 16), loss_cls=OracleBASD, mixup="fused", image_stats=STATS)
    with pytest.raises(ValueError, match="jpeg_decode needs resize_crop=True"):
        T.Trainer(student, _config(), teacher, jpeg_decode="parallel", **kw)
    for bad in ("serial", "Parallel", 2, None):
        with pytest.raises(ValueError, match="jpeg_decode must be True, False or 'parallel'"):
            T.Trainer(student, _config(), teacher, resize_crop=True, jpeg_decode=bad, **kw)
    tr = T.Trainer(student, _config(), teacher, resize_crop=True, jpeg_decode="parallel", **kw)
    assert isinstance(tr._decoder, JpegDecoder) and tr._decoder.entropy == "parallel"
    assert T.Trainer(student, _config(), teacher, resize_crop=True, jpeg_decode=True, **kw)._decoder.entropy == "serial"
    assert T.Trainer(student, _config(), teacher, resize_crop=True, **kw)._decoder is None
    assert '``"parallel"``' in T.Trainer.__doc__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.prepare_views({"images": pack_jpegs([_load(OLD)["gray_17x9_q75_plain"][0]]), "label": torch.arange(1)})


# ---- the lanes' passes on the host, under the sanitizers (stand-alone programs; nothing is preloaded and nothing is
# loaded into this process)
def _sanitizer_build(source, out):
    compilers = [c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)]
    if not compilers:
        pytest.skip("no host C++ compiler found")
    errors = []
    for cxx in compilers:
        for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
            done = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all", *static, "-o", out, source], capture_output=True,
                                  text=True)
            if done.returncode == 0:
                return out
            errors.append(f"{cxx} {' '.join(static)}: {done.stderr[-400:]}")
    pytest.fail(f"the sanitizer build of {source} failed:\n" + "\n".join(errors))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(the parallel host program, the serial one)."""
    where = tmp_path_factory.mktemp("jpeg_parallel_host")
    return tuple(_sanitizer_build(os.path.join(ROOT, "tools", f"{name}.cpp"), str(where / name))
                 for name in ("jpeg_parallel_host_check", "jpeg_host_check"))


def _write_batch(batch: JpegBatch, path):
    with open(path, "wb") as f:
        f.write(np.array([MAGIC, len(batch), batch.data.numel(), batch.out_bytes, batch.workspace_bytes, 0, 0, 0],
                         dtype="<i8").tobytes())
        f.write(batch.records.tobytes())
        f.write(batch.data.numpy().tobytes())


def _run(program, batch: JpegBatch, src, dst, *extra):
    """(the output bytes, per-image status, batch status, standard output) of a host program on the batch in ``src``."""
    done = subprocess.run([program, src, dst, *(str(e) for e in extra)], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint8)
    B = len(batch)
    assert raw.size == batch.out_bytes + 4 * B + 4
    status = raw[batch.out_bytes:].view("<i4")
    return raw[:batch.out_bytes], status[:B].copy(), int(status[B]), done.stdout


def _split(flat, batch):
    images, at = [], 0
    for h, w in batch.sizes.tolist():
        images.append(flat[at:at + 3 * h * w].reshape(h, w, 3))
        at += 3 * h * w
    return images


def _rounds(stdout):
    """image index -> the largest number of rounds a chunk of it took; and the program's overall maximum."""
    found = re.findall(r"^image (\d+) chunks \d+ max_rounds (\d+) swept (\d+)$", stdout, re.M)
    _rounds.swept = {int(i): int(w) for i, _, w in found}             # image index -> chunks that went through the sweep
    return {int(i): int(r) for i, r, _ in found}, int(re.search(r"^max_rounds (\d+)$", stdout, re.M).group(1))


def _damaged(old):
    """The damaged set of tests/test_jpeg_decode.py: every prefix of the two smallest streams, and those streams with
    each scan byte replaced by 0x00, by 0xFF and by its complement, under the whole stream's header."""
    base = {n: v for n, v in old.items() if not n.startswith("fallback_")}
    entries = []
    for name in sorted(base, key=lambda n: (len(base[n][0]), n))[:2]:
        stream = base[name][0]
        header = parse_jpeg(stream)
        entries += [(stream[:n], header) for n in range(len(stream))]
        for at in range(header.scan_offset, len(stream)):
            for value in (0x00, 0xFF, stream[at] ^ 0xFF):
                entries.append((stream[:at] + bytes([value]) + stream[at + 1:], header))
    return entries


def _damaged_tails(new):
    """Damage where a chunk ends: the two streams whose last block crosses a chunk's end with each byte from two ahead
    of that end to the end of the data replaced by 0x00, by 0xFF and by its complement, and cut at each of them."""
    entries = []
    for name, boundary in BOUNDARIES.items():
        stream = new[name][0]
        header = parse_jpeg(stream)
        for at in range(header.scan_offset + boundary - 2, len(stream) - 2):
            entries.append((stream[:at], header))
            for value in (0x00, 0xFF, stream[at] ^ 0xFF):
                entries.append((stream[:at] + bytes([value]) + stream[at + 1:], header))
    return entries


@pytest.fixture(scope="module")
def host_batches(old, both, tmp_path_factory):
    """name -> (batch, its file), written once for the three settings."""
    where = tmp_path_factory.mktemp("jpeg_parallel_batches")
    lookup = lambda data: next(rgb for s, rgb in old.values() if s == data)            # noqa: E731
    batches = {"good": pack_jpegs([s for s, _ in both.values()]),
               "mixed": pack_jpegs([s for s, _ in both.values()] + [old[n][0] for n in old if n.startswith("fallback_")],
                                   fallback=lookup),
               "damaged": J._pack(_damaged(old)), "tails": J._pack(_damaged_tails(both))}
    out = {}
    for name, batch in batches.items():
        path = str(where / f"{name}.in")
        _write_batch(batch, path)
        out[name] = (batch, path)
    return out


@pytest.fixture(scope="module")
def serial_damaged(programs, host_batches, tmp_path_factory):
    batch, path = host_batches["damaged"]
    return _run(programs[1], batch, path, str(tmp_path_factory.mktemp("jpeg_serial_out") / "damaged.out"))[:3]


SETTINGS = [(64, 16), (256, 16), (DEFAULT_LANES, DEFAULT_SUB_BYTES)]
_good_runs = {}


def _good_run(programs, host_batches, tmp_path_factory, lanes, sub_bytes):
    """The good batch through the parallel host program at one setting, run once for the tests that look at it."""
    if (lanes, sub_bytes) not in _good_runs:
        batch, path = host_batches["good"]
        _good_runs[lanes, sub_bytes] = _run(programs[0], batch, path, str(tmp_path_factory.mktemp("jpeg_good") / "out"),
                                            lanes, sub_bytes)
    return _good_runs[lanes, sub_bytes]


@pytest.fixture(scope="module")
def serial_tails(programs, host_batches, tmp_path_factory):
    batch, path = host_batches["tails"]
    return _run(programs[1], batch, path, str(tmp_path_factory.mktemp("jpeg_serial_out") / "tails.out"))[:3]


@pytest.mark.parametrize("lanes,sub_bytes", SETTINGS)
def test_damage_where_a_chunk_ends(programs, host_batches, serial_tails, tmp_path, lanes, sub_bytes):
    """A last block that crosses a chunk's end, damaged ahead of, at and behind that end: the serial host program's status
    words and bytes.  (The intact streams are part of the good batch of the test below.)"""
    batch, path = host_batches["tails"]
    flat, status, word, _ = _run(programs[0], batch, path, str(tmp_path / "tails.out"), lanes, sub_bytes)
    assert len(batch) >= 80 and (serial_tails[1] != 0).sum() > 30 and (serial_tails[1] == 0).sum() > 10
    assert np.array_equal(status, serial_tails[1]) and word == serial_tails[2]
    assert np.array_equal(flat, serial_tails[0])


def test_random_streams_in_small_chunks(programs, tmp_path):
    """150 seeded random Pillow streams up to 64 px, each also with one scan byte changed and cut at a random place, in
    chunks so small (3 lanes of 8 bytes, 8 of 8, 64 of 16) that blocks, errors and ends of data cross chunk ends
    everywhere: the serial host program's status words and bytes."""
    pytest.importorskip("PIL")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_goldens_jpeg_decode",
                                                  os.path.join(ROOT, "tests", "golden", "make_goldens_jpeg_decode.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    rng = np.random.default_rng(99)
    modes, entries = ("gray", "444", "422", "420"), []
    for n in range(150):
        w, h = int(rng.integers(8, 65)), int(rng.integers(8, 65))
        mode = modes[int(rng.integers(0, 4))]
        options = dict(quality=(30, 75, 90, 100)[int(rng.integers(0, 4))])
        if mode != "gray":
            options["subsampling"] = M.SUBSAMPLING[mode]
        if n % 7 == 3:
            options["restart_marker_rows"] = 1
        stream = M.encode(M.picture(rng, h, w, ("noise", "ramp")[n % 2], mode == "gray"), **options)
        header = parse_jpeg(stream)
        at = int(rng.integers(header.scan_offset, len(stream)))
        entries += [(stream, header), (stream[:at] + bytes([int(rng.integers(0, 256))]) + stream[at + 1:], header),
                    (stream[:int(rng.integers(header.scan_offset, len(stream)))], header)]
    batch = J._pack(entries)
    path = str(tmp_path / "random.in")
    _write_batch(batch, path)
    want = _run(programs[1], batch, path, str(tmp_path / "serial.out"))
    assert not want[1][0::3].any() and (want[1] != 0).sum() > 100
    for lanes, sub_bytes in ((3, 8), (8, 8), (64, 16)):
        got = _run(programs[0], batch, path, str(tmp_path / "parallel.out"), lanes, sub_bytes)
        assert np.array_equal(got[1], want[1]) and got[2] == want[2], (lanes, sub_bytes)
        assert np.array_equal(got[0], want[0]), (lanes, sub_bytes)


@pytest.mark.parametrize("lanes,sub_bytes", SETTINGS)
def test_host_build_under_the_sanitizers(programs, host_batches, serial_damaged, old, both, tmp_path, tmp_path_factory,
                                         lanes, sub_bytes):
    """Inside the program, every chunk also holds the handover to its word (it exits with status 3 otherwise)."""
    names = list(both)
    batch = host_batches["good"][0]
    flat, status, word, stdout = _good_run(programs, host_batches, tmp_path_factory, lanes, sub_bytes)
    assert word == 0 and not status.any()
    for got, name in zip(_split(flat, batch), names):
        assert np.array_equal(got, both[name][1]), name
    per_image, most = _rounds(stdout)
    assert "444_72x72_q75_81segments" not in {names[i] for i in per_image}         # a lane per segment, as the kernel
    assert len(per_image) == len(names) - 1
    assert 1 <= most <= lanes // 4 + 2 <= lanes                                     # the bound of include/basd_hip.h
    assert all(1 <= r <= lanes for r in per_image.values())                         # the flat streams among them
    # the fallback's pixels as raw records among them
    mixed, path = host_batches["mixed"]
    assert mixed.fallbacks == 2
    more, status, word, _ = _run(programs[0], mixed, path, str(tmp_path / "mixed.out"), lanes, sub_bytes)
    assert word == 0 and not status.any() and np.array_equal(more[:flat.size], flat)
    for got, name in zip(_split(more, mixed)[len(names):], [n for n in old if n.startswith("fallback_")]):
        assert np.array_equal(got, old[name][1]), name
    # damaged streams: the serial host program's status words and bytes
    damaged, path = host_batches["damaged"]
    flat, status, word, _ = _run(programs[0], damaged, path, str(tmp_path / "damaged.out"), lanes, sub_bytes)
    assert len(damaged) > 600 and (status != 0).sum() > 300 and (status == 0).sum() > 10
    assert np.array_equal(status, serial_damaged[1]) and word == serial_damaged[2]
    assert np.array_equal(flat, serial_damaged[0])


@pytest.mark.parametrize("lanes,sub_bytes", SETTINGS)
def test_rounds_stay_below_the_bound_on_noise_and_ramps(programs, host_batches, both, tmp_path_factory, lanes, sub_bytes):
    """Every chunk of a noise or ramp stream takes fewer rounds than it has lanes.

    The ramps fall into step (the 160 x 120 one: 8 rounds at the default).  Two-level noise at quality 100 does not at
    16-byte sub-sequences: it has no zero coefficient, so its blocks carry no end-of-block code, a block ends where the
    zigzag index reaches 64, and a decoder that starts inside one with index 0 never learns the true index.  What keeps
    such a chunk below the lane count is the stage's own bound: lanes / 4 rounds, then one lane's walk through the rest
    (lanes / 4 + 2 rounds with the first pass; the time is still that of up to ``lanes`` passes)."""
    names = list(both)
    per_image, _ = _rounds(_good_run(programs, host_batches, tmp_path_factory, lanes, sub_bytes)[3])
    figures = {names[i]: r for i, r in per_image.items() if "noise" in names[i] or "ramp" in names[i] or "rstrow" in names[i]}
    print(f"[jpeg_parallel] lanes {lanes}, sub_bytes {sub_bytes}: most rounds of a chunk",
          {n: r for n, r in figures.items() if r > 8 or n in ("444_160x160_q100_noise", "420_160x120_q90_ramp")})
    for name in ("444_160x160_q100_noise", "420_160x120_q90_ramp"):
        assert name in figures
    late = {n: r for n, r in figures.items() if ("noise" in n or "ramp" in n) and r >= lanes}
    assert not late, late
    # the ramps fall into step by themselves: no chunk of theirs needs the sweep at the default, and the first pass and
    # the rounds stay within lanes / 4 + 1 (a handover that were not canonical would keep every chunk from settling)
    if (lanes, sub_bytes) == (DEFAULT_LANES, DEFAULT_SUB_BYTES):
        ramps = [i for i, n in enumerate(names) if "ramp" in n and i in per_image]
        assert len(ramps) > 10 and names.index("420_160x120_q90_ramp") in ramps
        for i in ramps:
            assert _rounds.swept[i] == 0 and per_image[i] <= lanes // 4 + 1, (names[i], per_image[i], _rounds.swept[i])
        assert per_image[names.index("420_160x120_q90_ramp")] <= 16


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
@pytest.mark.parametrize("sub_bytes", [None, 16])
def test_both_corpora_as_one_batch(dev, both, sub_bytes):
    batch = pack_jpegs([s for s, _ in both.values()]).to(dev)
    decoder = JpegDecoder(dev, entropy="parallel", sub_bytes=sub_bytes)
    got = decoder(batch)
    assert decoder.status() == 0 and not decoder.image_status().any()
    serial = JpegDecoder(dev)
    want = serial(batch)
    assert serial.status() == 0 and torch.equal(got.data, want.data)
    for image, (name, (_, rgb)) in zip(_images(got), both.items()):
        assert np.array_equal(image, rgb), name


@pytest.mark.gpu
@pytest.mark.parametrize("sub_bytes", [None, 16])
def test_one_image_and_positions_in_a_batch(dev, both, sub_bytes):
    decoder = JpegDecoder(dev, entropy="parallel", sub_bytes=sub_bytes)
    largest = max(both, key=lambda n: len(both[n][0]))
    assert largest == "444_160x160_q100_noise" and len(parse_jpeg(both["444_72x72_q75_81segments"][0]).segments) == 81
    others = [s for n, (s, _) in both.items() if "q1_" in n][:6]
    for name in (largest, "444_72x72_q75_81segments", "gray_1x7_q1_noise"):
        stream, rgb = both[name]
        assert np.array_equal(_images(decoder(pack_jpegs([stream]).to(dev)))[0], rgb), name
        files = [stream] + others[:3] + [stream] + others[3:] + [stream]
        got = _images(decoder(pack_jpegs(files).to(dev)))
        assert decoder.status() == 0
        for at in (0, 4, len(files) - 1):
            assert np.array_equal(got[at], rgb), (name, at)


@pytest.mark.gpu
@pytest.mark.parametrize("sub_bytes", [None, 16])
def test_bad_streams_between_good_ones(dev, both, sub_bytes):
    """The cut stream is a prefix the sanitizer run of the host build has been through."""
    name = sorted((n for n in both if n in _load(OLD)), key=lambda n: (len(both[n][0]), n))[0]
    stream = both[name][0]
    header = parse_jpeg(stream)
    good = [both[n][0] for n in ("420_33x31_q75_rst1", "444_33x17_q75_plain", "420_160x120_q90_ramp")]
    rst = bytearray(good[0])
    rst[parse_jpeg(good[0]).segments[2] - 1] = 0xD5
    long_cut = both["444_160x160_q100_noise"][0]
    long_cut = long_cut[:(parse_jpeg(long_cut).scan_offset + len(long_cut)) // 2]      # ends in its second default chunk
    entries = [(good[0], parse_jpeg(good[0])),
               (stream[:(header.scan_offset + len(stream)) // 2], header),                 # truncated
               (good[1], parse_jpeg(good[1])),
               (bytes(rst), parse_jpeg(good[0])),                                          # a wrong restart marker
               (good[2], parse_jpeg(good[2])),
               (stream[:40], header),                                                      # tables past the stream
               (long_cut, parse_jpeg(both["444_160x160_q100_noise"][0])),                  # truncated, chunks in
               (good[0], parse_jpeg(good[0]))]
    batch = J._pack(entries).to(dev)
    decoder, serial = JpegDecoder(dev, entropy="parallel", sub_bytes=sub_bytes), JpegDecoder(dev)
    got, want = decoder(batch), serial(batch)
    per_image = decoder.image_status().tolist()
    assert per_image == [0, 3, 0, 5, 0, 1, 3, 0] and per_image == serial.image_status().tolist()
    assert decoder.status() == serial.status() == (1 << 2) | (1 << 4) | 1
    assert torch.equal(got.data, want.data)
    images = _images(got)
    for at in (1, 3, 5, 6):
        assert not images[at].any(), at
    for at, n in ((0, "420_33x31_q75_rst1"), (2, "444_33x17_q75_plain"), (4, "420_160x120_q90_ramp"),
                  (7, "420_33x31_q75_rst1")):
        assert np.array_equal(images[at], both[n][1]), at


@pytest.mark.gpu
@pytest.mark.parametrize("sub_bytes", [None, 16])
def test_a_last_block_across_a_chunks_end(dev, both, sub_bytes):
    """Byte 32768 of the larger stream's data ends a chunk at the default and at ``sub_bytes=16``: intact and damaged
    around that byte, the serial kernels' status words and bytes."""
    entries = [(both[n][0], parse_jpeg(both[n][0])) for n in BOUNDARIES] + _damaged_tails(both)
    batch = J._pack(entries).to(dev)
    decoder, serial = JpegDecoder(dev, entropy="parallel", sub_bytes=sub_bytes), JpegDecoder(dev)
    got, want = decoder(batch), serial(batch)
    status = serial.image_status()
    assert status[:2].tolist() == [0, 0] and (status != 0).sum() > 30 and (status == 0).sum() > 10
    assert torch.equal(decoder.image_status(), status) and decoder.status() == serial.status()
    assert torch.equal(got.data, want.data)
    for image, name in zip(_images(got)[:2], BOUNDARIES):
        assert np.array_equal(image, both[name][1]), name


@pytest.mark.gpu
def test_guard_bytes_and_the_workspace_past_its_used_part(dev, both):
    from basd_amd import _lib
    from basd_amd._launch import raw_stream
    decoder = JpegDecoder(dev, entropy="parallel")
    decoder(pack_jpegs([s for s, _ in both.values()]).to(dev))
    large = decoder.used_bytes
    small = pack_jpegs([both["420_33x31_q75_rst1"][0], both["420_160x120_q90_ramp"][0]]).to(dev)
    assert small.workspace_bytes < large // 4
    decoder.workspace.fill_(0x5A)
    guard = 256
    out = torch.full((small.out_bytes + 2 * guard,), 0xC3, dtype=torch.uint8, device=dev)
    table = torch.from_numpy(small.records.view(np.uint8).copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for sub_bytes in (0, 16):
        _lib.call("basd_jpeg_decode_parallel", small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard,
                  small.out_bytes, 2, table.data_ptr(), decoder.workspace.data_ptr(), decoder.workspace.numel(),
                  status.data_ptr(), small.max_blocks, small.max_pixels, sub_bytes, raw_stream(dev.index))
        host, ws = out.cpu().numpy(), decoder.workspace.cpu().numpy()
        assert int(status.item()) == 0
        assert (host[:guard] == 0xC3).all() and (host[-guard:] == 0xC3).all()
        assert (ws[small.workspace_bytes:] == 0x5A).all() and (ws[8:128] == 0x5A).all() and not ws[:8].any()
        want = np.concatenate([both["420_33x31_q75_rst1"][1].reshape(-1), both["420_160x120_q90_ramp"][1].reshape(-1)])
        assert np.array_equal(host[guard:-guard], want)
    # the argument rule of sub_bytes, ahead of every launch
    lib = _lib.load()
    for bad in (4, 12, J.SUB_BYTES_MAX + 8, -8):
        assert lib.basd_jpeg_decode_parallel(small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard,
                                             small.out_bytes, 2, table.data_ptr(), decoder.workspace.data_ptr(),
                                             decoder.workspace.numel(), status.data_ptr(), small.max_blocks,
                                             small.max_pixels, bad, raw_stream(dev.index)) == _lib.EINVAL, bad


@pytest.mark.gpu
def test_launches_and_copies_do_not_depend_on_the_batch(dev, both):
    """Three launches and one copy (the record table) per call for B = 1 and for B = 9, no memset, as the serial
    stage.  Counted with ``torch.profiler`` where it sees launches made through ctypes (the output says whether)."""
    from torch.profiler import ProfilerActivity, profile
    files = [s for s, _ in both.values()]
    decoder = JpegDecoder(dev, entropy="parallel")
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
        print(f"[jpeg_parallel] profiler, B = {B}: {len(kernels)} kernels ({len(ours)} of the decoder), {len(copies)} "
              "copies in 7 calls")
        if ours:
            assert len(ours) == 21 and len(kernels) == 21, sorted({e.name for e in kernels})
            assert sum("jpeg_entropy_parallel_kernel" in e.name for e in ours) == 7
            assert len(copies) == 7 and not any("dtoh" in e.name.lower().replace(" ", "") for e in copies)
        else:
            assert not kernels and len(copies) in (0, 7)
    assert counts[1] == counts[9] and decoder.status() == 0


@pytest.mark.gpu
def test_fallback_images_travel_as_raw_records(dev, old, new):
    names = ["422_31x33_q75_rst2", "fallback_progressive", "420_160x120_q90_ramp", "fallback_cmyk", "420_33x31_q75_plain"]
    corpus = dict(old, **new)
    lookup = lambda data: next(rgb for s, rgb in old.values() if s == data)            # noqa: E731
    batch = pack_jpegs([corpus[n][0] for n in names], fallback=lookup)
    assert batch.records["kind"].tolist() == [0, 1, 0, 1, 0]
    decoder = JpegDecoder(dev, entropy="parallel")
    got = _images(decoder(batch.to(dev)))
    assert decoder.status() == 0
    for image, name in zip(got, names):
        assert np.array_equal(image, corpus[name][1]), name
    only = pack_jpegs([old["fallback_cmyk"][0]], fallback=lookup)
    assert only.max_blocks == 0 and np.array_equal(_images(decoder(only.to(dev)))[0], old["fallback_cmyk"][1])


@pytest.mark.gpu
def test_trainer_and_evaluation_in_parallel_mode(dev, both):
    from basd_amd import trainer as T
    from basd_amd.evaluation import evaluate_model
    from tools import stock_models as SM
    names = ("420_33x31_q75_rst1", "444_33x17_q75_plain", "420_160x120_q90_ramp", "420_64x96_q100_noise")
    files = [both[n][0] for n in names]
    crops = draw_crop_params(pack_images([both[n][1] for n in names]).sizes, generator=torch.Generator().manual_seed(2))
    student, teacher = _toy_models(dev)
    kw = dict(student_info=SM.probe_model(student, 16), mixup="fused", image_stats=STATS, resize_crop=True)
    label = torch.arange(4) % 10
    views = {}
    for mode in (True, "parallel"):
        tr = T.Trainer(student, _config(), teacher, jpeg_decode=mode, **kw)
        views[mode] = tr.prepare_views({"images": pack_jpegs(files), "label": label, "crop_params": crops})
        assert tr._decoder.status() == 0 and tr._resizer.status() == 0
    for p, s in zip(views["parallel"], views[True]):
        assert p.dtype == torch.uint8 and p.shape == (4, 3, 16, 16) and torch.equal(p, s)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    ekw = dict(num_classes=10, image_stats=(MEAN, STD), resize_crop=ResizeCrop(16, 0.875, device=dev))
    batches = [{"images": pack_jpegs(files), "label": torch.tensor([1, 2, 3, 4])},
               {"images": pack_jpegs(files[:2]), "label": torch.tensor([5, 6])}]
    parallel = JpegDecoder(dev, entropy="parallel")
    got = evaluate_model(student, batches, criterion, jpeg_decode=parallel, **ekw)
    assert got == evaluate_model(student, batches, criterion, jpeg_decode=JpegDecoder(dev), **ekw)
    assert np.isfinite(got["loss"]) and parallel.status() == 0
