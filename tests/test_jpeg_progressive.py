"""Progressive JPEG on the device (opt-in): ``parse_jpeg`` / ``pack_jpegs`` / ``collate_jpeg`` / ``decode_reference``
with ``progressive=True`` and ``basd_jpeg_decode_progressive``.

The chain of evidence: the recorded pixels are Pillow's, of streams Pillow wrote and of hand-made streams under other
scan scripts that Pillow decodes to the same pixels (``tests/golden/make_goldens_jpeg_progressive.py``);
``decode_reference(..., progressive=True)`` (the specification of ``include/basd_hip.h`` in numpy) equals them; the
per-scan code of the kernel (``csrc/jpeg_core.h``), run scan after scan by ``tools/jpeg_progressive_host_check.cpp``
under the sanitizers, equals them and gives every damaged stream a status word; the kernel, which runs the scans by
levels, equals the recorded bytes and, on the damaged streams, the host program's status words and bytes.  Every
comparison is ``array_equal``.
"""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import jpeg as J
from basd_amd.jpeg import JpegBatch, JpegDecoder, collate_jpeg, decode_reference, pack_jpegs, parse_jpeg
from basd_amd.resize import RaggedBatch, ResizeCrop, draw_crop_params, pack_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_progressive.npz")
BASELINE = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
MAGIC = 0x4745504a44534142
MODES = ("gray", "444", "422", "420")
SIZES = ((1, 1), (7, 9), (8, 8), (9, 17), (17, 33), (33, 31), (40, 24), (64, 48))
HAND_SIZES = ((1, 1), (9, 17), (17, 33), (33, 31))
SCRIPTS = ("spectral", "reversed", "al3")
FLAT = "gray_1456x1448_flat"
MANY = "444_72x72_q75_81segments"
PROGRESSIVE = "not baseline: progressive (SOF2)"


@pytest.fixture(scope="module")
def corpus():
    """name -> (stream bytes, Pillow's RGB)."""
    g = np.load(GOLDEN, allow_pickle=False)
    return {str(n): (g[f"stream_{n}"].tobytes(), g[f"rgb_{o}"]) for n, o in zip(g["names"], g["origin"])}


@pytest.fixture(scope="module")
def baseline():
    g = np.load(BASELINE, allow_pickle=False)
    return {str(n): (g[f"stream_{n}"].tobytes(), g[f"rgb_{n}"]) for n in g["names"]}


def _lookup(*corpora):
    """A fallback that finds the recorded pixels of a stream (no Pillow needed)."""
    def fallback(data):
        return next(rgb for c in corpora for s, rgb in c.values() if s == data)
    return fallback


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_the_corpus_holds_what_the_issue_names(corpus):
    assert os.path.getsize(GOLDEN) < 400 * 1000
    kinds = {(m, s): set() for m in MODES for s in SIZES}
    for name in corpus:
        mode, size, *rest = name.split("_")
        if mode != "hand" and name not in (FLAT, MANY):
            kinds[mode, tuple(int(v) for v in size.split("x"))].update(rest)
    for (mode, size), seen in kinds.items():
        assert {"q75", "rst1", "rstrow"} <= seen and seen & {"q1", "q100"} and seen & {"noise", "ramp"}, (mode, size, seen)
        if size[0] * size[1] < 1000:
            assert {"q1", "q100"} <= seen, (mode, size)
    assert {"q1", "q100", "noise", "ramp"} <= set().union(*(kinds[m, (64, 48)] for m in MODES))
    for mode in MODES:
        for w, h in HAND_SIZES:
            for script in SCRIPTS:
                for restart in (0, 1, 3) if (w, h) == (17, 33) else (0,):
                    assert f"hand_{mode}_{w}x{h}_{script}_rst{restart}" in corpus
    many = parse_jpeg(corpus[MANY][0], progressive=True)
    assert many.reason is None and all(len(s.segments) == 81 for s in many.scans) and many.hs == 1
    flat = parse_jpeg(corpus[FLAT][0], progressive=True)
    assert flat.reason is None and flat.ncomp == 1 and flat.blocks > 32767 and len(corpus[FLAT][0]) < 16000
    assert (corpus[FLAT][1] == corpus[FLAT][1][0, 0]).all()
    # the hand-made scripts are what their names say
    al3 = parse_jpeg(corpus["hand_420_17x33_al3_rst3"][0], progressive=True)
    assert al3.reason is None and len(al3.scans) == 25 and al3.scans[0].al == 3 and al3.scans[0].restart == 3
    assert [s.ah for s in al3.scans if s.ss == 0] == [0, 3, 2, 1] and max(s.level for s in al3.scans) == 3
    assert len(al3.scans[1].segments) == 5 and len(al3.scans[0].segments) == 2      # 3 x 5 luma blocks, 2 x 3 MCUs
    rev = parse_jpeg(corpus["hand_444_9x17_reversed_rst0"][0], progressive=True)
    assert [s.comps for s in rev.scans] == [(2,), (1,), (0,)] * 3 and [s.ah for s in rev.scans] == [0] * 6 + [1] * 3
    spectral = parse_jpeg(corpus["hand_gray_33x31_spectral_rst0"][0], progressive=True)
    assert [(s.ss, s.se, s.ah, s.al) for s in spectral.scans] == [(0, 0, 0, 0), (1, 5, 0, 0), (6, 63, 0, 0)]


def test_goldens_equal_the_reference_and_pillow(corpus):
    for name, (stream, rgb) in corpus.items():
        assert np.array_equal(decode_reference(stream, progressive=True), rgb), name
    try:
        from PIL import Image  # noqa: F401
    except ImportError:
        return
    for name, (stream, rgb) in corpus.items():
        assert np.array_equal(J.pillow_fallback(stream), rgb), name


def test_without_the_keyword_nothing_changes(corpus, baseline):
    names = ["420_17x33_q75_rst1", "hand_gray_9x17_al3_rst0", "444_8x8_q100_" + ("noise" if "444_8x8_q100_noise" in corpus
                                                                                else "ramp")]
    fallback = _lookup(corpus)
    for name in names:
        stream = corpus[name][0]
        assert parse_jpeg(stream) == parse_jpeg(stream, False) == J.JpegHeader(PROGRESSIVE)
        with pytest.raises(ValueError, match="not in the device's scope: not baseline: progressive"):
            decode_reference(stream)
    files = [corpus[n][0] for n in names]
    batch = pack_jpegs(files, fallback=fallback)
    assert batch.records["kind"].tolist() == [1, 1, 1] and batch.fallbacks == 3 and batch.progressive == 0
    assert not batch.records["pad"].any() and batch.max_blocks == 0 and (batch.max_scans, batch.max_segments) == (0, 0)
    collated = collate_jpeg([{"image": f, "label": i} for i, f in enumerate(files)], fallback)
    assert collated["images"].records.tobytes() == batch.records.tobytes() and collated["label"].tolist() == [0, 1, 2]
    assert torch.equal(collated["images"].data, batch.data)
    saved, J._default_fallback = J._default_fallback, lambda: None
    try:
        with pytest.raises(J.UnsupportedJpeg, match="progressive"):
            pack_jpegs(files)
    finally:
        J._default_fallback = saved
    # a baseline stream parses and packs alike with and without the keyword
    for name in ("420_33x31_q75_rst1", "gray_17x9_q75_plain"):
        stream = baseline[name][0]
        assert parse_jpeg(stream, progressive=True) == parse_jpeg(stream) and parse_jpeg(stream).scans == ()
        assert np.array_equal(decode_reference(stream, progressive=True), baseline[name][1])
        a, b = pack_jpegs([stream]), pack_jpegs([stream], progressive=True)
        assert a.records.tobytes() == b.records.tobytes() and torch.equal(a.data, b.data)


def test_with_the_keyword_scans_levels_and_records(corpus, baseline):
    stream = corpus["420_17x33_q75_rst1"][0]
    h = parse_jpeg(stream, progressive=True)
    assert h.reason is None and (h.width, h.height, h.ncomp, h.hs, h.vs) == (17, 33, 3, 2, 2) and len(h.quant) == 3
    assert (h.dc, h.ac, h.segments) == ((), (), ()) and h.blocks == 36
    # libjpeg's script for three components: ten scans in three levels
    assert [(s.comps, s.ss, s.se, s.ah, s.al) for s in h.scans] == [
        ((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
        ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
    assert tuple(s.level for s in h.scans) == (0, 0, 0, 0, 0, 1, 1, 1, 1, 2)
    # a one-component scan walks the component's own grid, 3 x 5 luma blocks, not the MCU-padded 4 x 6
    assert [len(s.segments) for s in h.scans] == [6, 15, 6, 6, 15, 15, 6, 6, 6, 15] and all(s.restart == 1 for s in h.scans)
    for s in h.scans:
        assert s.segments[0] > 0 and stream[s.data_end] == 0xFF and stream[s.data_end + 1] in (0xC4, 0xDA, 0xD9)
        assert all(stream[p - 2:p] == bytes([0xFF, 0xD0 + (i & 7)]) for i, p in enumerate(s.segments[1:]))
    gray = parse_jpeg(corpus["gray_9x17_q75_rst1"][0], progressive=True)
    assert tuple(s.level for s in gray.scans) == (0, 0, 0, 1, 1, 2) and gray.blocks == 6
    # records of the three kinds in one batch
    names = [(baseline, "420_33x31_q75_rst2"), (corpus, "420_17x33_q75_rst1"), (baseline, "fallback_cmyk"),
             (corpus, "hand_gray_9x17_al3_rst0"), (baseline, "gray_17x9_q75_plain")]
    files = [c[n][0] for c, n in names]
    batch = pack_jpegs(files, fallback=_lookup(baseline), progressive=True)
    rec, data = batch.records, batch.data.numpy()
    assert rec["kind"].tolist() == [0, 2, 1, 2, 0] and (batch.fallbacks, batch.progressive) == (1, 2)
    assert batch.max_scans == 11 and batch.max_segments == 15 and batch.max_blocks == 36
    assert rec["coef_offset"].tolist() == [128, 128 + 192 * 36, 0, 128 + 192 * 72, 128 + 192 * 78]
    assert batch.workspace_bytes == 128 + 192 * 84 and rec.dtype.itemsize == 128 and J.SCAN_DTYPE.itemsize == 64
    for i, header in ((1, h), (3, parse_jpeg(files[3], progressive=True))):
        at, n = int(rec["src_offset"][i]), int(rec["src_len"][i])
        assert data[at:at + n].tobytes() == files[i] and tuple(rec["quant"][i][:header.ncomp]) == header.quant
        count, table_at, widest, zero = rec["pad"][i].tolist()
        assert count == len(header.scans) and (at + table_at) % 8 == 0 and zero == 0
        assert widest == max(len(s.segments) for s in header.scans)
        rows = data[at + table_at:at + table_at + 64 * count].view(J.SCAN_DTYPE)
        for row, scan in zip(rows, header.scans):
            assert (int(row["ss"]), int(row["se"]), int(row["ah"]), int(row["al"])) == (scan.ss, scan.se, scan.ah, scan.al)
            assert (int(row["ncomp"]), int(row["comp"]), int(row["level"])) == (len(scan.comps), scan.comps[0], scan.level)
            assert int(row["data_end"]) == scan.data_end and int(row["restart"]) == scan.restart
            assert tuple(row["dc"].tolist()) == scan.dc and int(row["ac"]) == scan.ac
            seg_at = at + int(row["seg_offset"])
            assert seg_at % 4 == 0 and tuple(data[seg_at:seg_at + 4 * int(row["n_seg"])].view(np.int32).tolist()) == scan.segments
    collated = collate_jpeg([{"image": f} for f in files], _lookup(baseline), progressive=True)
    assert collated["images"].records.tobytes() == rec.tobytes() and torch.equal(collated["images"].data, batch.data)
    assert batch.to("cpu") is batch
    # the library's table and the header agree on the new entry point
    from basd_amd import _lib
    vp, i32, i64 = _lib.vp, _lib.i32, _lib.i64
    assert _lib.SIGNATURES["basd_jpeg_decode_progressive"] == [vp, i64, vp, i64, i32, vp, vp, i64, vp, i64, i64, i32, i32,
                                                               i32, i32, vp]
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        text = f.read()
    for want in ("int basd_jpeg_decode_progressive(", f"#define BASD_JPEG_MAX_SCANS {J.MAX_SCANS}",
                 f"#define BASD_JPEG_KIND_PROGRESSIVE {J.KIND_PROGRESSIVE}", "typedef struct BasdJpegScan {"):
        assert want in text, want
    assert J.MAX_SCANS == 64 and J.KIND_PROGRESSIVE == 2 and "``progressive=True``" in pack_jpegs.__doc__


def _scan_spans(stream):
    """Per scan of a progressive stream (the offset of its SOS marker, the offset of the marker behind its data)."""
    h = parse_jpeg(stream, progressive=True)
    spans = []
    for s in h.scans:
        sos = stream.rfind(b"\xff\xda", 0, s.segments[0])
        spans.append((sos, s.data_end))
    return spans


def _set_approximation(stream, scan, ah, al):
    sos = _scan_spans(stream)[scan][0]
    first = parse_jpeg(stream, progressive=True).scans[scan].segments[0]
    assert stream[sos:sos + 2] == b"\xff\xda"
    return stream[:first - 1] + bytes([(ah << 4) | al]) + stream[first:]


def test_out_of_scope_files_take_the_fallback_with_a_named_reason(corpus, baseline):
    stream, rgb = corpus["420_17x33_q75_rst1"]
    spans = _scan_spans(stream)
    assert len(spans) == 10 and stream[spans[-1][1]:] == b"\xff\xd9"
    dqt = stream.index(b"\xff\xdb")
    dqt = stream[dqt:dqt + 2 + int.from_bytes(stream[dqt + 2:dqt + 4], "big")]
    # an AC scan ahead of its component's first DC scan: the hand-made script's per-component scans, reordered
    rev = corpus["hand_444_9x17_reversed_rst0"][0]
    rs = _scan_spans(rev)
    head, tail = rev[:rs[0][0]], rev[rs[-1][1]:]
    piece = lambda i: rev[rs[i][0]:rs[i][1]]                           # noqa: E731
    ac_first = head + piece(3) + b"".join(piece(i) for i in (0, 1, 2, 4, 5, 6, 7, 8)) + tail
    # a DC scan of two of the three components
    sos = spans[0][0]
    two = stream[:sos] + b"\xff\xda\x00\x0a\x02" + stream[sos + 5:sos + 9] + stream[sos + 11:]
    # more than 64 scans: a gray stream whose 63 AC coefficients come in 63 scans, between three DC scans (66 in all)
    many = _many_scans()
    cases = {
        "an incomplete progression (Pillow smooths it)": stream[:spans[-1][0]] + b"\xff\xd9",
        "a quantisation table between scans": stream[:spans[3][0]] + dqt + stream[spans[3][0]:],
        "an AC scan ahead of the first DC scan of its component (2)": ac_first,
        "previous Al is 2 (Ah must equal it, and Al be Ah - 1)": _set_approximation(stream, 5, 1, 0),
        "a DC scan of 2 of the 3 components": two,
        "more than 64 scans": many,
        "4 components (CMYK / YCCK)": _progressive_cmyk(baseline),
    }
    fallback_calls = []

    def fallback(data):
        fallback_calls.append(data)
        return rgb

    for reason, data in cases.items():
        found = parse_jpeg(data, progressive=True).reason
        assert found is not None and reason in found, (reason, found)
        with pytest.raises(ValueError, match="not in the device's scope"):
            decode_reference(data, progressive=True)
    batch = pack_jpegs(list(cases.values()) + [stream], fallback=fallback, progressive=True)
    assert fallback_calls == list(cases.values()) and batch.records["kind"].tolist() == [1] * len(cases) + [2]
    # further rules, each with its reason
    for reason, data in (("a first scan (Ah 0) of coefficients 1..63 of component 0", _set_approximation(stream, 5, 0, 1)),
                         ("a scan with Al 14", _set_approximation(stream, 0, 0, 14)),
                         ("an Adobe APP14 segment", stream[:spans[2][0]] + b"\xff\xee\x00\x0eAdobe\0\x64\0\0\0\0\0"
                          + stream[spans[2][0]:])):
        found = parse_jpeg(data, progressive=True).reason
        assert found is not None and reason in found, (reason, found)
    # a comment and an application segment between scans are in scope
    noted = stream[:spans[4][0]] + b"\xff\xfe\x00\x05hey" + b"\xff\xe1\x00\x04ab" + stream[spans[4][0]:]
    assert parse_jpeg(noted, progressive=True).reason is None
    assert np.array_equal(decode_reference(noted, progressive=True), rgb)


def _many_scans():
    """66 scans of a flat 1 x 1 gray picture: DC, each AC coefficient alone (one end-of-band code each), DC again."""
    g = np.load(GOLDEN, allow_pickle=False)
    name = next(str(n) for n in g["names"] if str(n).startswith("gray_1x1_q75_") and "rst" not in str(n))
    stream = g[f"stream_{name}"].tobytes()
    head = stream[:stream.index(b"\xff\xc4")]                          # SOI, APP0, DQT, SOF2: what lies ahead of the first DHT
    dht = b"\xff\xc4\x00\x14\x00" + bytes([1] + [0] * 15) + b"\x00" + b"\xff\xc4\x00\x14\x10" + bytes([1] + [0] * 15) + b"\x00"
    cid = head[head.index(b"\xff\xc2") + 10]
    sos = lambda ss, se, ah, al: b"\xff\xda\x00\x08\x01" + bytes([cid, 0, ss, se, (ah << 4) | al])       # noqa: E731
    out = head + dht + sos(0, 0, 0, 2) + b"\x7f"                       # DC category 0 (code 0), padded with ones
    for k in range(1, 64):
        out += sos(k, k, 0, 0) + b"\x7f"                               # end of band (symbol 0)
    out += sos(0, 0, 2, 1) + b"\x7f" + sos(0, 0, 1, 0) + b"\x7f"
    return out + b"\xff\xd9"


def _progressive_cmyk(baseline):
    """A progressive CMYK file: Pillow's where it is importable, else the recorded baseline CMYK file with its frame
    header marked SOF2 (the frame header is what the host decides on)."""
    try:
        from PIL import Image
    except ImportError:
        stream = baseline["fallback_cmyk"][0]
        return stream.replace(b"\xff\xc0", b"\xff\xc2", 1)
    import io
    out = io.BytesIO()
    Image.fromarray(np.arange(9 * 15 * 4, dtype=np.uint8).reshape(9, 15, 4), mode="CMYK").save(
        out, format="JPEG", quality=75, progressive=True)
    return out.getvalue()


def test_sixty_four_scans_are_in_scope_and_sixty_six_are_not():
    many = _many_scans()
    assert "more than 64 scans" in parse_jpeg(many, progressive=True).reason
    # the same file with the AC coefficients 61..63 in one scan instead of three has 64 scans and is in scope
    spans = _scan_spans_unchecked(many)
    assert len(spans) == 66
    head = many[:spans[61][0]]
    cid = many[spans[0][0] + 5]
    merged = head + b"\xff\xda\x00\x08\x01" + bytes([cid, 0, 61, 63, 0]) + b"\x7f" + many[spans[64][0]:]
    h = parse_jpeg(merged, progressive=True)
    assert h.reason is None and len(h.scans) == 64 and max(s.level for s in h.scans) == 2
    rgb = decode_reference(merged, progressive=True)
    assert rgb.shape == (1, 1, 3) and rgb[0, 0, 0] == rgb[0, 0, 1] == rgb[0, 0, 2]
    try:
        from PIL import Image  # noqa: F401
    except ImportError:
        return
    assert np.array_equal(J.pillow_fallback(merged), rgb)


def _scan_spans_unchecked(stream):
    """(offset of each SOS marker, offset of the marker behind its one byte of data) of ``_many_scans``'s layout."""
    spans, at = [], stream.index(b"\xff\xda")
    while at >= 0:
        spans.append((at, at + 11))
        at = stream.find(b"\xff\xda", at + 2)
    return spans


# ---- the host program under the sanitizers (a stand-alone program; nothing is preloaded and nothing is loaded into
# this process)
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
def program(tmp_path_factory):
    where = tmp_path_factory.mktemp("jpeg_progressive_host")
    return _sanitizer_build(os.path.join(ROOT, "tools", "jpeg_progressive_host_check.cpp"),
                            str(where / "jpeg_progressive_host_check"))


def _run(program, batch: JpegBatch, where, tag):
    """(the output bytes, per-image status, batch status) of the host program on ``batch``."""
    src, dst = str(where / f"{tag}.in"), str(where / f"{tag}.out")
    with open(src, "wb") as f:
        f.write(np.array([MAGIC, len(batch), batch.data.numel(), batch.out_bytes, batch.workspace_bytes, batch.max_scans,
                          batch.max_segments, 0], dtype="<i8").tobytes())
        f.write(batch.records.tobytes())
        f.write(batch.data.numpy().tobytes())
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint8)
    B = len(batch)
    assert raw.size == batch.out_bytes + 4 * B + 4
    status = raw[batch.out_bytes:].view("<i4")
    return raw[:batch.out_bytes], status[:B].copy(), int(status[B])


def _split(flat, batch):
    images, at = [], 0
    for h, w in batch.sizes.tolist():
        images.append(flat[at:at + 3 * h * w].reshape(h, w, 3))
        at += 3 * h * w
    return images


def _damaged(corpus):
    """Entries for ``J._pack`` from two small streams of three components, one without and one with restart markers:
    each scan cut at every byte (the bytes from there to the scan's end are taken out, what follows stays, and the host
    parses the result again: a truncated scan); every prefix of the file from its first scan on under the whole file's
    header (offsets past the end: the record check's share); and 300 seeded changes of one byte behind the first SOS
    under the whole file's header."""
    plain = next(n for n in corpus if n.startswith("420_9x17_q75_") and "rst" not in n)
    rng = np.random.default_rng(20261020)
    entries = []
    for name in (plain, "420_9x17_q75_rst1"):
        stream = corpus[name][0]
        whole = parse_jpeg(stream, progressive=True)
        for scan in whole.scans:
            for at in range(scan.segments[0], scan.data_end):
                cut = stream[:at] + stream[scan.data_end:]
                header = parse_jpeg(cut, progressive=True)
                entries.append((cut, header if header.reason is None else whole))
        entries += [(stream[:n], whole) for n in range(whole.scan_offset, len(stream))]
        for _ in range(300):
            at = int(rng.integers(whole.scan_offset - 14, len(stream)))
            value = (stream[at] ^ (1 << int(rng.integers(0, 8)))) if rng.integers(0, 2) else int(rng.integers(0, 256))
            entries.append((stream[:at] + bytes([value]) + stream[at + 1:], whole))
    return entries


@pytest.fixture(scope="module")
def host_damaged(program, corpus, tmp_path_factory):
    """(the damaged batch, the host program's output bytes, status words and batch word): kept for the GPU test."""
    batch = J._pack(_damaged(corpus))
    return (batch,) + _run(program, batch, tmp_path_factory.mktemp("jpeg_progressive_damaged"), "damaged")


def test_host_build_under_the_sanitizers(program, corpus, baseline, host_damaged, tmp_path):
    names = list(corpus)
    batch = pack_jpegs([s for s, _ in corpus.values()], fallback=lambda data: pytest.fail("no fallback here"),
                       progressive=True)
    assert batch.progressive == len(names) and batch.max_segments == 81 and batch.max_scans == 25
    flat, status, word = _run(program, batch, tmp_path, "corpus")
    assert word == 0 and not status.any()
    for got, name in zip(_split(flat, batch), names):
        assert np.array_equal(got, corpus[name][1]), name
    # baseline and raw records among them
    mixed_names = [(baseline, "420_33x31_q75_rst1"), (corpus, "420_17x33_q75_rst1"), (baseline, "fallback_cmyk"),
                   (corpus, "hand_422_33x31_al3_rst0"), (baseline, "444_72x72_q75_81segments"), (corpus, MANY)]
    mixed = pack_jpegs([c[n][0] for c, n in mixed_names], fallback=_lookup(baseline), progressive=True)
    assert mixed.records["kind"].tolist() == [0, 2, 1, 2, 0, 2]
    flat, status, word = _run(program, mixed, tmp_path, "mixed")
    assert word == 0 and not status.any()
    for got, (c, n) in zip(_split(flat, mixed), mixed_names):
        assert np.array_equal(got, c[n][1]), n
    # the damaged streams: each ends with a status word and, where that is not 0, an all-zero image
    damaged, flat, status, word = host_damaged
    assert len(damaged) > 2000 and damaged.progressive == len(damaged)
    codes = {int(c): int((status == c).sum()) for c in np.unique(status)}
    print(f"[jpeg_progressive] host program, {len(damaged)} damaged streams: status -> count {codes}")
    assert set(codes) <= set(J.STATUS_NAMES) and codes.get(3, 0) > 100 and codes.get(1, 0) > 100 and codes.get(5, 0) > 50 and codes.get(0, 0) > 10
    assert word == sum(1 << (c - 1) for c in codes if c)
    for image, code in zip(_split(flat, damaged), status):
        assert code == 0 or not image.any()
    # the host program and the kernels refuse the record elsewhere: the serial program sees a bad record
    serial = _sanitizer_build(os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), str(tmp_path / "jpeg_host_check"))
    flat, status, word = _run(serial, mixed, tmp_path, "serial")
    assert status.tolist() == [0, 1, 0, 1, 0, 1] and word == 1
    for got, (c, n), code in zip(_split(flat, mixed), mixed_names, status):
        assert np.array_equal(got, c[n][1]) if code == 0 else not got.any(), n


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
@pytest.mark.parametrize("entropy", ["serial", "parallel"])
def test_the_corpus_as_one_batch(dev, corpus, baseline, entropy):
    more = ["420_33x31_q75_rst1", "gray_17x9_q75_plain", "444_72x72_q75_81segments"]
    files = [s for s, _ in corpus.values()] + [baseline[n][0] for n in more]
    want = [rgb for _, rgb in corpus.values()] + [baseline[n][1] for n in more]
    batch = pack_jpegs(files, fallback=lambda data: pytest.fail("no fallback here"), progressive=True)
    assert batch.progressive == len(corpus)
    decoder = JpegDecoder(dev, entropy=entropy)
    got = decoder(batch.to(dev))
    assert decoder.status() == 0 and not decoder.image_status().any()
    for image, rgb, name in zip(_images(got), want, list(corpus) + more):
        assert np.array_equal(image, rgb), name


@pytest.mark.gpu
def test_one_image_and_each_position_in_a_mixed_batch(dev, corpus, baseline):
    decoder = JpegDecoder(dev)
    lookup = _lookup(baseline)
    others = [baseline["420_33x31_q75_rst1"], baseline["fallback_cmyk"], corpus["gray_9x17_q75_rst1"],
              baseline["gray_17x9_q75_plain"], corpus["hand_444_17x33_reversed_rst3"]]
    for name in (MANY, "420_17x33_q75_rst1", "hand_420_17x33_al3_rst1", "gray_1x1_q75_rstrow"):
        stream, rgb = corpus[name]
        alone = decoder(pack_jpegs([stream], progressive=True).to(dev))
        assert decoder.status() == 0 and np.array_equal(_images(alone)[0], rgb), name
        for at in range(len(others) + 1):
            mixed = others[:at] + [(stream, rgb)] + others[at:]
            batch = pack_jpegs([s for s, _ in mixed], fallback=lookup, progressive=True)
            assert sorted(batch.records["kind"].tolist()) == [0, 0, 1, 2, 2, 2]
            got = _images(decoder(batch.to(dev)))
            assert decoder.status() == 0
            for image, (_, want) in zip(got, mixed):
                assert np.array_equal(image, want), (name, at)


@pytest.mark.gpu
def test_damaged_streams_between_good_ones(dev, corpus, baseline, host_damaged):
    """The damaged streams are those the sanitizer run of the host build has been through: the kernel, which runs the
    scans by levels, gives the status words and bytes of the host program, which runs them in stream order."""
    damaged, flat, status, word = host_damaged
    good = [(corpus["420_17x33_q75_rst1"][0], parse_jpeg(corpus["420_17x33_q75_rst1"][0], progressive=True)),
            (baseline["420_33x31_q75_rst1"][0], parse_jpeg(baseline["420_33x31_q75_rst1"][0]))]
    batch = J._pack([good[0], good[1]] + _damaged(corpus) + [good[1], good[0]])
    for entropy in ("serial", "parallel"):
        decoder = JpegDecoder(dev, entropy=entropy)
        images = _images(decoder(batch.to(dev)))
        per_image = decoder.image_status().numpy()
        assert per_image[:2].tolist() == [0, 0] and per_image[-2:].tolist() == [0, 0]
        assert np.array_equal(per_image[2:-2], status) and decoder.status() == word
        got = np.concatenate([image.reshape(-1) for image in images[2:-2]])
        assert np.array_equal(got, flat)
        for at, (c, n) in ((0, (corpus, "420_17x33_q75_rst1")), (1, (baseline, "420_33x31_q75_rst1")),
                           (-2, (baseline, "420_33x31_q75_rst1")), (-1, (corpus, "420_17x33_q75_rst1"))):
            assert np.array_equal(images[at], c[n][1]), at


@pytest.mark.gpu
def test_guard_bytes_and_the_workspace_past_its_used_part(dev, corpus, baseline):
    from basd_amd import _lib
    from basd_amd._launch import raw_stream
    decoder = JpegDecoder(dev)
    decoder(pack_jpegs([s for s, _ in corpus.values() if len(s) < 20000], progressive=True).to(dev))
    large = decoder.used_bytes
    names = [(corpus, "420_17x33_q75_rst1"), (baseline, "420_33x31_q75_rst1"), (corpus, "hand_422_33x31_al3_rst0")]
    small = pack_jpegs([c[n][0] for c, n in names], progressive=True).to(dev)
    assert small.workspace_bytes < large // 4 and small.progressive == 2
    guard = 256
    out = torch.full((small.out_bytes + 2 * guard,), 0xC3, dtype=torch.uint8, device=dev)
    table = torch.from_numpy(small.records.view(np.uint8).copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    want = np.concatenate([c[n][1].reshape(-1) for c, n in names])
    for parallel in (0, 1):
        decoder.workspace.fill_(0x5A)
        out.fill_(0xC3)
        _lib.call("basd_jpeg_decode_progressive", small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard,
                  small.out_bytes, 3, table.data_ptr(), decoder.workspace.data_ptr(), decoder.workspace.numel(),
                  status.data_ptr(), small.max_blocks, small.max_pixels, 0, parallel, small.max_scans,
                  small.max_segments, raw_stream(dev.index))
        host, ws = out.cpu().numpy(), decoder.workspace.cpu().numpy()
        assert int(status.item()) == 0
        assert (host[:guard] == 0xC3).all() and (host[-guard:] == 0xC3).all()
        assert (ws[small.workspace_bytes:] == 0x5A).all() and (ws[12:128] == 0x5A).all() and not ws[:12].any()
        assert np.array_equal(host[guard:-guard], want)
    # the other entry points refuse the record, and say so in its status word alone
    for entry, extra in (("basd_jpeg_decode", ()), ("basd_jpeg_decode_parallel", (0,))):
        status.zero_()
        _lib.call(entry, small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard, small.out_bytes, 3,
                  table.data_ptr(), decoder.workspace.data_ptr(), decoder.workspace.numel(), status.data_ptr(),
                  small.max_blocks, small.max_pixels, *extra, raw_stream(dev.index))
        assert int(status.item()) == 1
        assert decoder.workspace[:12].view(torch.int32).tolist() == [1, 0, 1]
        host = out.cpu().numpy()[guard:-guard]
        first, second = 3 * 17 * 33, 3 * 17 * 33 + 3 * 33 * 31
        assert not host[:first].any() and not host[second:].any()
        assert np.array_equal(host[first:second], baseline["420_33x31_q75_rst1"][1].reshape(-1))
    # a record that claims more scans, or a scan more segments, than the call allows is a bad record
    for scans, segments, codes in ((9, small.max_segments, [1, 0, 0]), (small.max_scans, 14, [1, 0, 0])):
        status.zero_()
        _lib.call("basd_jpeg_decode_progressive", small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard,
                  small.out_bytes, 3, table.data_ptr(), decoder.workspace.data_ptr(), decoder.workspace.numel(),
                  status.data_ptr(), small.max_blocks, small.max_pixels, 0, 0, scans, segments, raw_stream(dev.index))
        assert decoder.workspace[:12].view(torch.int32).tolist()[0] == 1 and int(status.item()) == 1
    # the argument rules, ahead of every launch
    lib = _lib.load()
    for sub_bytes, parallel, scans, segments in ((0, 2, 10, 15), (16, 0, 10, 15), (12, 1, 10, 15), (0, 0, 65, 15),
                                                 (0, 0, -1, 15), (0, 0, 10, -1)):
        assert lib.basd_jpeg_decode_progressive(small.data.data_ptr(), small.data.numel(), out.data_ptr() + guard,
                                                small.out_bytes, 3, table.data_ptr(), decoder.workspace.data_ptr(),
                                                decoder.workspace.numel(), status.data_ptr(), small.max_blocks,
                                                small.max_pixels, sub_bytes, parallel, scans, segments,
                                                raw_stream(dev.index)) == _lib.EINVAL, (sub_bytes, parallel, scans)


@pytest.mark.gpu
def test_one_more_launch_with_progressive_records_and_none_without(dev, corpus, baseline):
    """A batch without progressive records: the three launches of the parent commit (the entropy kernel of the chosen
    stage, idct, pixels).  With them: four.  One copy (the record table) either way, no memset, for B = 1 and B = 9.
    Counted with ``torch.profiler`` where it sees launches made through ctypes (the output says whether)."""
    from torch.profiler import ProfilerActivity, profile
    plain = [s for n, (s, _) in baseline.items() if not n.startswith("fallback_")]
    prog = [s for s, _ in corpus.values() if len(s) < 3000]
    for entropy, first in (("serial", "jpeg_entropy_kernel"), ("parallel", "jpeg_entropy_parallel_kernel")):
        decoder = JpegDecoder(dev, entropy=entropy)
        counts = {}
        for kind, files, per_call in (("baseline", plain, 3), ("mixed", prog[:5] + plain, 4)):
            for B in (9, 1):
                batch = pack_jpegs(files[:B], progressive=True).to(dev)
                assert (batch.progressive > 0) == (kind == "mixed")
                for _ in range(3):
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
                counts[kind, B] = (len(kernels), len(ours), len(copies))
                print(f"[jpeg_progressive] profiler, {entropy}, {kind}, B = {B}: {len(kernels)} kernels ({len(ours)} of "
                      f"the decoder), {len(copies)} copies in 7 calls")
                if ours:
                    assert len(ours) == 7 * per_call and len(kernels) == 7 * per_call, sorted({e.name for e in kernels})
                    assert sum(first + "<" in e.name or first + "(" in e.name for e in ours) == 7
                    assert sum("jpeg_progressive_kernel" in e.name for e in ours) == (7 if kind == "mixed" else 0)
                    assert sum("jpeg_idct_kernel" in e.name for e in ours) == 7
                    assert sum("jpeg_pixel_kernel" in e.name for e in ours) == 7
                    assert len(copies) == 7 and not any("dtoh" in e.name.lower().replace(" ", "") for e in copies)
                else:
                    assert not kernels and len(copies) in (0, 7)
            assert counts[kind, 1] == counts[kind, 9]
        assert decoder.status() == 0


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STATS = {"clean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "augmented": (MEAN, STD)}


def _config():
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=4),
                           model=SimpleNamespace(num_classes=10, vit=SimpleNamespace(img_size=16)),
                           data=SimpleNamespace(eval_crop_ratio=0.875))


@pytest.mark.gpu
def test_trainer_and_evaluation_fed_by_the_progressive_collate(dev, corpus, baseline):
    """The same files through ``collate_jpeg(progressive=True)`` and through the fallback: bit-identical batches."""
    from basd_amd import trainer as T
    from basd_amd.evaluation import evaluate_model
    from tools import stock_models as SM
    names = [(corpus, "420_33x31_q75_rst1"), (corpus, "hand_444_33x31_al3_rst0"), (baseline, "420_33x31_q75_rst1"),
             (corpus, "422_64x48_q75_rstrow")]
    files = [c[n][0] for c, n in names]
    fallback = _lookup(corpus, baseline)
    samples = [{"image": f, "label": i + 1} for i, f in enumerate(files)]
    crops = draw_crop_params(pack_images([c[n][1] for c, n in names]).sizes, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    student = SM.StockViT(img_size=16, patch_size=4, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.make_teacher(SM.StockViT(img_size=16, patch_size=4, embed_dim=64, depth=3, num_heads=4,
                                          num_classes=0).to(dev), 16)
    kw = dict(student_info=SM.probe_model(student, 16), mixup="fused", image_stats=STATS, resize_crop=True)
    views = {}
    for progressive in (False, True):
        batch = collate_jpeg(samples, fallback, progressive=progressive)
        assert batch["images"].progressive == (3 if progressive else 0) and batch["images"].fallbacks == (0 if progressive else 3)
        tr = T.Trainer(student, _config(), teacher, jpeg_decode=True, **kw)
        views[progressive] = tr.prepare_views(dict(batch, crop_params=crops))
        assert tr._decoder.status() == 0 and tr._resizer.status() == 0
    for p, f in zip(views[True], views[False]):
        assert p.dtype == torch.uint8 and p.shape == (4, 3, 16, 16) and torch.equal(p, f)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    ekw = dict(num_classes=10, image_stats=(MEAN, STD), resize_crop=ResizeCrop(16, 0.875, device=dev))
    results = {}
    for progressive in (False, True):
        batches = [collate_jpeg(samples, fallback, progressive=progressive),
                   collate_jpeg(samples[:2], fallback, progressive=progressive)]
        decoder = JpegDecoder(dev)
        results[progressive] = evaluate_model(student, batches, criterion, jpeg_decode=decoder, **ekw)
        assert decoder.status() == 0
    assert results[True] == results[False] and np.isfinite(results[True]["loss"])
    assert "progressive" in T.Trainer.__doc__ and "progressive" in evaluate_model.__doc__
