"""Bicubic and box resampling in ``basd_resize_crop``, chosen per record / per view (``basd_amd.resize``,
``csrc/resize.hip``, ``csrc/resize_core.h``).

The same three layers as ``tests/test_resize_crop.py``, every comparison ``array_equal`` (no tolerance, no excluded
pixels): the specification of ``include/basd_hip.h`` restated in numpy (``resize_reference(..., filter=)``) is held to
Pillow -- live where Pillow is installed, and always to Pillow 12.2.0's outputs recorded in
``tests/golden/resize_filters.npz`` --, the kernel is held to the restatement, and so is the host build of the kernel's
per-axis code (``tools/resize_host_check.cpp``) under the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import resize as R
from basd_amd.resize import (CropParams, ResizeCrop, draw_crop_params, make_records, max_reduction, pack_images,
                             resize_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_filters.npz")
FILTERS = ("bilinear", "bicubic", "box")
MAGIC = 0x5a53524444534142


def structured(rng, h, w, c, two_level=False):
    """A ramp with noise (so that a shifted or transposed read shows), or a 0 / 255 image."""
    if two_level:
        return np.where(rng.rand(h, w, c) < 0.5, 0, 255).astype(np.uint8)
    ramp = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None]
    return ((ramp + rng.randint(0, 120, (h, w, c))) % 256).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against Pillow
# ---------------------------------------------------------------------------------------------------------------------
def _pillow(img, window, resized, name):
    from PIL import Image
    wx, wy, ww, wh = window
    pil = Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img)
    out = np.asarray(pil.crop((wx, wy, wx + ww, wy + wh)).resize(resized, getattr(Image, name.upper())))
    return out[:, :, None] if out.ndim == 2 else out


def test_restatement_equals_pillow_for_every_filter():
    pytest.importorskip("PIL")
    rng = np.random.RandomState(17)
    bad = []
    extremes = {name: [1 << 21, 1 << 21] for name in FILTERS}
    for i in range(240):
        h, w, c = rng.randint(1, 90), rng.randint(1, 90), (3, 1)[i % 4 == 3]
        img = structured(rng, h, w, c, two_level=i % 3 == 0)
        ww, wh = rng.randint(1, w + 1), rng.randint(1, h + 1)
        window = (rng.randint(0, w - ww + 1), rng.randint(0, h - wh + 1), ww, wh)
        resized = (rng.randint(1, 70), rng.randint(1, 70))
        for name in FILTERS:
            got = resize_reference(img, window, resized, filter=name, extremes=extremes[name])
            if not np.array_equal(got, _pillow(img, window, resized, name)):
                bad.append((i, name, img.shape, window, resized))
    assert not bad, f"{len(bad)} of {3 * 240} cases differ: {bad[:5]}"
    img = structured(rng, 375, 500, 3)
    for name in FILTERS:
        got = resize_reference(img, (0, 0, 500, 375), (341, 256), filter=name, extremes=extremes[name])
        assert np.array_equal(got, _pillow(img, (0, 0, 500, 375), (341, 256), name)), name
    # the clamp is the one thing bicubic adds to the passes: these cases reach it at both ends, the others never do
    low, high = extremes["bicubic"]
    assert low < 0 and high > (255 << 22) + (1 << 22) - 1, (low, high)       # acc >> 22 below 0 and above 255
    for name in ("bilinear", "box"):
        assert extremes[name][0] >= 0 and extremes[name][1] >> 22 <= 255, (name, extremes[name])


def test_restatement_equals_the_recorded_pillow_outputs():
    g = np.load(GOLDEN, allow_pickle=False)
    cases = g["cases"]
    assert 36 <= len(cases) <= 48 and str(g["pillow_version"]) == "12.2.0" and tuple(g["filters"].tolist()) == FILTERS
    assert os.path.getsize(GOLDEN) < 512 * 1024
    differ = 0
    for k, (i, wx, wy, ww, wh, rw, rh) in enumerate(cases.tolist()):
        for name in FILTERS:
            got = resize_reference(g[f"image_{i}"], (wx, wy, ww, wh), (rw, rh), filter=name)
            assert np.array_equal(got, g[f"out_{name}_{k}"]), (k, name, cases[k].tolist())
        differ += not np.array_equal(g[f"out_bicubic_{k}"], g[f"out_bilinear_{k}"])
        differ += not np.array_equal(g[f"out_box_{k}"], g[f"out_bilinear_{k}"])
    assert differ > len(cases)                                           # the three filters are three different answers
    # the default is bilinear, by position too
    i, wx, wy, ww, wh, rw, rh = cases[0].tolist()
    assert np.array_equal(resize_reference(g[f"image_{i}"], (wx, wy, ww, wh), (rw, rh)), g["out_bilinear_0"])


def test_identity_pass_and_rectangle_for_every_filter():
    rng = np.random.RandomState(2)
    img = structured(rng, 23, 31, 3)
    for name in FILTERS:
        whole = resize_reference(img, (2, 3, 25, 17), (13, 29), filter=name)
        assert whole.shape == (29, 13, 3)
        assert np.array_equal(resize_reference(img, (2, 3, 25, 17), (13, 29), (4, 6, 9, 20), filter=name), whole[6:26, 4:13])
        assert np.array_equal(resize_reference(img, (2, 3, 25, 17), (25, 17), filter=name), img[3:20, 2:27]), name


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the record table and the names
# ---------------------------------------------------------------------------------------------------------------------
def test_make_records_fills_the_filter_per_view():
    assert R.INTERPOLATIONS == FILTERS and (R.BAD_GEOMETRY, R.BAD_RATIO, R.BAD_FILTER) == (1, 2, 4)
    assert R.RECORD_DTYPE.itemsize == 64 and R.RECORD_DTYPE.fields["filter"][1] == 48
    assert R.RECORD_DTYPE.fields["pad"][1] == 52 and R.RECORD_DTYPE["pad"].shape == (3,)
    assert [max_reduction(n) for n in FILTERS] == [32, 16, 32]
    sizes = torch.tensor([[375, 500], [64, 48]], dtype=torch.int32)
    crops = CropParams([10, 0], [20, 8], [300, 64], [400, 40])
    default = make_records(sizes, 224, 0.875, crops)
    assert default["filter"].tolist() == [0, 0, 0, 0] and not default["pad"].any()
    assert make_records(sizes, 224, 0.875, crops, interpolation="bilinear").tobytes() == default.tobytes()
    for name, value in (("bicubic", 1), ("box", 2), ("BICUBIC", 1)):
        rec = make_records(sizes, 224, 0.875, crops, interpolation=name)
        assert rec["filter"].tolist() == [value] * 4
        rec["filter"] = 0
        assert rec.tobytes() == default.tobytes()                         # nothing else moves
    rec = make_records(sizes, 224, 0.875, crops, interpolation={"clean": "bicubic", "augmented": "box"})
    assert rec["filter"].tolist() == [1, 1, 2, 2]
    rec = make_records(sizes, 224, 0.875, crops, interpolation={"clean": "bicubic"})      # the other view: the default
    assert rec["filter"].tolist() == [1, 1, 0, 0]
    rec = make_records(sizes, 224, 0.875, crops, views=("augmented", "clean"), interpolation={"clean": "box"})
    assert rec["filter"].tolist() == [0, 0, 2, 2]
    out = np.zeros(4, dtype=R.RECORD_DTYPE)
    out["filter"] = 7
    assert make_records(sizes, 224, 0.875, crops, out=out, interpolation={"augmented": "bicubic"})["filter"].tolist() == [
        0, 0, 1, 1]


def test_the_reduction_limit_is_per_filter():
    # the augmented view: a window of exactly 16 times the image size passes for bicubic, one more source pixel does not
    one = torch.tensor([[200, 200]])
    assert make_records(one, 6, 0.875, CropParams([0], [0], [96], [10]), views=("augmented",),
                        interpolation="bicubic")["win_h"].tolist() == [96]
    with pytest.raises(ValueError, match=r"image 0 \(97 x 10\) is more than 16 times the image size 6.*bicubic"):
        make_records(one, 6, 0.875, CropParams([0], [0], [97], [10]), views=("augmented",), interpolation="bicubic")
    with pytest.raises(ValueError, match=r"image 0 \(10 x 97\) is more than 16 times"):
        make_records(one, 6, 0.875, CropParams([0], [0], [10], [97]), views=("augmented",), interpolation="bicubic")
    for name in ("bilinear", "box"):                                       # 97 is fine for them, 192 the most, 193 too much
        make_records(one, 6, 0.875, CropParams([0], [0], [192], [10]), views=("augmented",), interpolation=name)
        with pytest.raises(ValueError, match=f"image 0.*more than 32 times.*{name}"):
            make_records(one, 6, 0.875, CropParams([0], [0], [193], [10]), views=("augmented",), interpolation=name)
    # the limit is the view's own: the same window is refused only where its view is bicubic
    crops, small = CropParams([0], [0], [97], [10]), torch.tensor([[100, 100]])     # clean: 100 -> 7, inside both limits
    make_records(small, 6, 0.875, crops, interpolation={"clean": "bicubic", "augmented": "bilinear"})
    with pytest.raises(ValueError, match="more than 16 times"):
        make_records(small, 6, 0.875, crops, interpolation={"clean": "bilinear", "augmented": "bicubic"})
    # the clean view: 160 -> 10 is a reduction of exactly 16, 161 -> 10 is above it
    assert make_records(torch.tensor([[160, 160]]), 10, 1.0, views=("clean",), interpolation="bicubic")["res_w"].tolist() == [10]
    with pytest.raises(ValueError, match=r"image 0 \(161 x 161\).*outside the limits \(a bicubic reduction of at most 16"):
        make_records(torch.tensor([[161, 161]]), 10, 1.0, views=("clean",), interpolation="bicubic")
    make_records(torch.tensor([[161, 161]]), 10, 1.0, views=("clean",), interpolation="box")


def test_unknown_and_excluded_names():
    sizes = torch.tensor([[64, 48]], dtype=torch.int32)
    for call in (lambda n: make_records(sizes, 16, 0.875, views=("clean",), interpolation=n),
                 lambda n: ResizeCrop(16, 0.875, device="cpu", interpolation=n),
                 lambda n: resize_reference(np.zeros((4, 4, 3), np.uint8), (0, 0, 4, 4), (2, 2), filter=n),
                 lambda n: make_records(sizes, 16, 0.875, views=("clean",), interpolation={"clean": n})):
        with pytest.raises(ValueError, match=r"one of \('bilinear', 'bicubic', 'box'\).*'cubic'"):
            call("cubic")
        with pytest.raises(ValueError, match=r"one of \('bilinear', 'bicubic', 'box'\)"):
            call(1)
        for name, why in (("hamming", "cos"), ("lanczos", "sin"), ("LANCZOS", "sin")):
            with pytest.raises(ValueError, match=f"(?s)not offered.*{why}.*last bit differs between math libraries.*"
                                                 r"\('bilinear', 'bicubic', 'box'\)"):
                call(name)
        with pytest.raises(ValueError, match=r"(?s)'nearest' is not offered.*different code path.*'bilinear', 'bicubic', 'box'"):
            call("nearest")
    with pytest.raises(ValueError, match=r"names the views \['flipped'\]"):
        ResizeCrop(16, 0.875, device="cpu", interpolation={"flipped": "box"})


def test_resize_crop_defaults_are_unchanged():
    rc = ResizeCrop(16, 0.875, device="cpu")
    assert rc.interpolation == {"clean": "bilinear", "augmented": "bilinear"}
    assert (rc.image_size, rc.crop_ratio, rc.device) == (16, 0.875, torch.device("cpu"))
    assert ResizeCrop(16, 0.875, device="cpu", interpolation="box").interpolation == {"clean": "box", "augmented": "box"}
    mixed = ResizeCrop(16, 0.875, device="cpu", interpolation={"clean": "bicubic"})
    assert mixed.interpolation == {"clean": "bicubic", "augmented": "bilinear"}
    images = [structured(np.random.RandomState(1), 20, 27, 3)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the arguments are in order; only the device is not
        mixed(pack_images(images))
    # the limit of the instance's filter is applied by the call, ahead of the device
    tall = pack_images([np.zeros((300, 20, 3), np.uint8)])
    with pytest.raises(ValueError, match="more than 16 times"):
        ResizeCrop(16, 0.875, device="cpu", interpolation="bicubic")(tall, CropParams([0], [0], [257], [20]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ResizeCrop(16, 0.875, device="cpu")(tall, CropParams([0], [0], [257], [20]))


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


def test_trainer_takes_the_interpolation_on_cpu():
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models()
    kw = dict(student_info=SM.probe_model(student, 16), loss_cls=OracleBASD, mixup="fused", image_stats=STATS)
    per_view = {"clean": "bicubic", "augmented": "bilinear"}
    tr = T.Trainer(student, _config(), teacher, resize_crop=True, resize_interpolation=per_view, **kw)
    assert tr._resizer.interpolation == per_view
    assert T.Trainer(student, _config(), teacher, resize_crop=True, resize_interpolation="box",
                     **kw)._resizer.interpolation == {"clean": "box", "augmented": "box"}
    assert T.Trainer(student, _config(), teacher, resize_crop=True, **kw)._resizer.interpolation == {
        "clean": "bilinear", "augmented": "bilinear"}
    with pytest.raises(ValueError, match="resize_interpolation.*needs resize_crop=True"):
        T.Trainer(student, _config(), teacher, resize_interpolation="bicubic", **kw)
    with pytest.raises(ValueError, match="not offered"):
        T.Trainer(student, _config(), teacher, resize_crop=True, resize_interpolation="lanczos", **kw)
    assert T.Trainer(student, _config(), teacher, **kw)._resizer is None


# ---------------------------------------------------------------------------------------------------------------------
# records, shared by the host program's test and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _record(offset, img, window, resized, corner, name="bilinear"):
    rec = np.zeros((), dtype=R.RECORD_DTYPE)
    rec["src_offset"], rec["src_h"], rec["src_w"] = offset, img.shape[0], img.shape[1]
    rec["win_x"], rec["win_y"], rec["win_w"], rec["win_h"] = window
    rec["res_w"], rec["res_h"] = resized
    rec["out_x"], rec["out_y"] = corner
    rec["filter"] = name if isinstance(name, int) else FILTERS.index(name)
    return rec


def _want(images, index, rec, OH, OW):
    """The restatement of one record: (C, OH, OW)."""
    window = tuple(int(rec[k]) for k in ("win_x", "win_y", "win_w", "win_h"))
    got = resize_reference(images[index], window, (int(rec["res_w"]), int(rec["res_h"])),
                           (int(rec["out_x"]), int(rec["out_y"]), OW, OH), filter=FILTERS[int(rec["filter"])])
    return got.transpose(2, 0, 1)


def _assert_records(got, images, owners, records, OH, OW, what):
    bad = []
    for i, (index, rec) in enumerate(zip(owners, records)):
        want = _want(images, index, rec, OH, OW)
        if not np.array_equal(got[i], want):
            bad.append((i, rec.tolist()[:12], int((got[i] != want).sum())))
    assert not bad, f"{what}: {len(bad)} of {len(records)} records differ: (index, record, bytes) {bad[:6]}"


def _golden():
    g = np.load(GOLDEN, allow_pickle=False)
    cases = g["cases"].tolist()
    images = [g[f"image_{i}"] for i in range(1 + max(c[0] for c in cases))]
    return g, cases, images


def _bad_record_table(kind):
    """Two images, a good record before and after a bad one: (images, ragged, table, the good records, the status bit)."""
    rng = np.random.RandomState(12)
    images = [structured(rng, 21, 25, 3), structured(rng, 150, 19, 3)]
    ragged = pack_images(images)
    o = ragged.offsets
    good = [_record(o[0], images[0], (2, 3, 20, 15), (9, 11), (1, 2), "bicubic"),
            _record(o[1], images[1], (0, 0, 19, 30), (14, 12), (5, 3), "box")]
    if kind == "ratio":                                                    # 145 > 16 * 9 down; 144 would pass
        bad, bit = _record(o[1], images[1], (5, 1, 13, 145), (9, 9), (0, 0), "bicubic"), R.BAD_RATIO
    else:
        bad, bit = _record(o[1], images[1], (5, 4, 13, 20), (12, 12), (1, 1), kind), R.BAD_FILTER
    return images, ragged, [good[0], bad, good[1]], good, bit


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the host build of csrc/resize_core.h under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    source = os.path.join(ROOT, "tools", "resize_host_check.cpp")
    out = str(tmp_path_factory.mktemp("resize_host") / "resize_host_check")
    compilers = [c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)]
    if not compilers:
        pytest.skip("no host C++ compiler found")
    errors = []
    # the sanitizers' runtimes linked statically where the compiler can (the program then stands alone), else as it links
    for cxx in compilers:
        for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
            done = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-ffp-contract=off",
                                   "-fno-sanitize-recover=all", *static, "-o", out, source], capture_output=True,
                                  text=True)
            if done.returncode == 0:
                return out
            errors.append(f"{cxx} {' '.join(static)}: {done.stderr[-400:]}")
    if all("sanitize" in e or "asan" in e or "ubsan" in e for e in errors):
        pytest.skip("no host compiler with the sanitizer runtimes found")
    pytest.fail("the sanitizer build of tools/resize_host_check.cpp failed:\n" + "\n".join(errors))


def _run_host(program, ragged, records, OH, OW, tmp_path, name, src_bytes=None):
    """((n, C, OH, OW) bytes, status word) of the host program on one record table."""
    table = np.stack(records)
    n, C = len(table), ragged.channels
    data = ragged.data.numpy()[:ragged.data.numel() if src_bytes is None else src_bytes]
    src, dst = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}.out")
    with open(src, "wb") as f:
        f.write(np.array([MAGIC, n, data.size, C, OH, OW, 0, 0], dtype="<i8").tobytes())
        f.write(table.tobytes())
        f.write(data.tobytes())
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (name, done.returncode, done.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint8)
    assert raw.size == n * C * OH * OW + 4
    return raw[:-4].reshape(n, C, OH, OW), int(raw[-4:].view("<i4")[0])


def test_host_build_under_the_sanitizers(host_check, tmp_path):
    g, cases, images = _golden()
    for k, (i, wx, wy, ww, wh, rw, rh) in enumerate(cases):               # one run per case, a record per filter
        img = images[i]
        records = [_record(0, img, (wx, wy, ww, wh), (rw, rh), (0, 0), name) for name in FILTERS]
        got, status = _run_host(host_check, pack_images([img]), records, rh, rw, tmp_path, f"golden{k}")
        assert status == 0
        for j, name in enumerate(FILTERS):
            assert np.array_equal(got[j], g[f"out_{name}_{k}"].transpose(2, 0, 1)), (k, name, cases[k])
    # 65 taps (bicubic at 16, bilinear at 32), box at 32, the last byte of the buffer as the last tap, 1 x 1 enlarged
    rng = np.random.RandomState(3)
    img = structured(rng, 224, 225, 3, two_level=True)
    ragged = pack_images([img])
    records = [_record(0, img, (1, 112, 224, 112), (14, 7), (7, 0), "bicubic"),
               _record(0, img, (1, 0, 224, 224), (7, 7), (0, 0), "box"),
               _record(0, img, (1, 0, 224, 224), (7, 7), (0, 0), "bilinear"),
               _record(0, img, (224, 223, 1, 1), (9, 9), (2, 2), "bicubic"),
               _record(0, img, (224, 223, 1, 1), (9, 9), (2, 2), "box")]
    got, status = _run_host(host_check, ragged, records, 7, 7, tmp_path, "limits")
    assert status == 0
    _assert_records(got, [img], [0] * len(records), records, 7, 7, "host, limits")
    # bad records: zeros and the status bit, the neighbours exact; a source one byte short of its image is not read
    for kind in ("ratio", 3, -1):
        images2, ragged2, table, good, bit = _bad_record_table(kind)
        got, status = _run_host(host_check, ragged2, table, 9, 7, tmp_path, f"bad{kind}")
        assert status == bit and not got[1].any(), kind
        _assert_records(got[[0, 2]], images2, [0, 1], good, 9, 7, f"host, bad {kind}")
    images2, ragged2, table, good, _ = _bad_record_table(3)
    got, status = _run_host(host_check, ragged2, [good[1]], 9, 7, tmp_path, "short", src_bytes=ragged2.nbytes - 1)
    assert status == R.BAD_GEOMETRY and not got.any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the restatement, byte for byte
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _launch(dev, ragged, records, OH, OW, band_rows=0):
    """One raw launch: ``records`` a list of RECORD_DTYPE scalars.  Returns (n, C, OH, OW) on the host and the status."""
    from basd_amd import _lib
    table = np.stack(records)
    n, C = len(table), ragged.channels
    data = ragged.data.to(dev)
    dev_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.full((n, C, OH, OW), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("basd_resize_crop", data.data_ptr(), data.numel(), out.data_ptr(), n, C, OH, OW, dev_table.data_ptr(),
              status.data_ptr(), band_rows, torch._C._cuda_getCurrentRawStream(dev.index))
    return out.cpu().numpy(), int(status.item())


def _axis(rng, kind, need, most):
    """(window side, resized side) of one axis: resized >= need (the output rectangle must fit), window <= most * resized."""
    if kind == "reduce" and need <= 9:
        res = rng.randint(need, 10)
        return rng.randint(res, min(17, most * res) + 1), res            # sides 1..17 -> 1..9
    if kind == "same":
        res = rng.randint(need, 18)
        return res, res
    res = rng.randint(need, 18)
    return rng.randint(1, min(9, res) + 1), res                         # sides 1..9 -> 1..17


def _mixed_table(rng, C, OH, OW, names):
    """Twelve records on six sources of odd widths: every pair of records shares its source (with ``names[i % len]`` as
    the filter of record i); the kinds per axis cover reducing, enlarging and one axis unchanged with the other
    changed; half of the rectangles touch the far edge of the resized image at a corner > 0 where the sizes allow."""
    kinds = [("reduce", "reduce"), ("enlarge", "enlarge"), ("same", "reduce"), ("reduce", "same"), ("same", "enlarge"),
             ("enlarge", "same"), ("reduce", "enlarge"), ("enlarge", "reduce"), ("same", "same"), ("reduce", "reduce"),
             ("enlarge", "enlarge"), ("enlarge", "reduce")]
    geo = []
    for i, (kx, ky) in enumerate(kinds):
        name = names[i % len(names)]
        win_w, res_w = _axis(rng, kx, OW, max_reduction(name))
        win_h, res_h = _axis(rng, ky, OH, max_reduction(name))
        far = i % 2 == 0
        corner = (res_w - OW if far else rng.randint(0, res_w - OW + 1), res_h - OH if far else rng.randint(0, res_h - OH + 1))
        geo.append((win_w, win_h, res_w, res_h, corner, name))
    images, owners, placed = [], [], []
    for s in range(6):
        a, b = geo[2 * s], geo[2 * s + 1]
        w = max(a[0], b[0]) + rng.randint(0, 4)
        w += 1 - w % 2                                                   # odd: the next image starts at an odd offset
        h = max(a[1], b[1]) + rng.randint(0, 4)
        images.append(structured(rng, h, w, C, two_level=s in (1, 4)))
        for win_w, win_h, res_w, res_h, corner, name in (a, b):
            window = (rng.randint(0, w - win_w + 1), rng.randint(0, h - win_h + 1), win_w, win_h)
            owners.append(s)
            placed.append((window, (res_w, res_h), corner, name))
    ragged = pack_images(images)
    offsets = ragged.offsets
    records = [_record(offsets[s], images[s], *p) for s, p in zip(owners, placed)]
    return images, ragged, owners, records


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("name", ["bicubic", "box"])
def test_mixed_tables_equal_the_restatement(dev, name, C):
    """Output widths 1..17 (the heights walk through 1..17 as well), one launch each over a mixed table of one filter."""
    rng = np.random.RandomState(60 + C + 10 * FILTERS.index(name))
    starts, far_corners, one_axis = set(), 0, 0
    for OW in range(1, 18):
        OH = (OW * 7) % 17 + 1
        images, ragged, owners, records = _mixed_table(rng, C, OH, OW, (name,))
        starts |= {int(o) % 4 for o in ragged.offsets}
        far_corners += sum(int(r["out_x"]) > 0 and int(r["out_x"]) + OW == int(r["res_w"]) for r in records)
        one_axis += sum((int(r["res_w"]) == int(r["win_w"])) != (int(r["res_h"]) == int(r["win_h"])) for r in records)
        got, status = _launch(dev, ragged, records, OH, OW)
        _assert_records(got, images, owners, records, OH, OW, f"{name}, C = {C}, OW = {OW}, OH = {OH}")
        assert status == 0
    assert starts == {0, 1, 2, 3} and far_corners >= 17 and one_axis >= 34


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bicubic", "box"])
def test_clamps_at_the_window_and_at_both_ends_of_a_byte(dev, name):
    """A 1 x 1 window enlarged to 9 x 9 (every tap clamps at the window, ``ww`` renormalises what is left of the negative
    lobes); a block of 0 in an image of 255 and the reverse, with the window on the block alone (nothing outside it may
    be read: the output is flat) and with the window over the block's edges (bicubic overshoots below 0 and above 255
    there, and the clamp cuts both)."""
    H, W, OH, OW = 40, 47, 8, 8
    images, records, owners = [], [], []
    for level in (0, 255):
        img = np.full((H, W, 3), 255 - level, np.uint8)
        img[14:25, 17:30] = level
        images.append(img)
    rng = np.random.RandomState(5)
    images.append(structured(rng, 7, 9, 3))
    ragged = pack_images(images)
    flat = []
    for i in range(2):
        for resized, corner in (((8, 8), (0, 0)), ((29, 31), (21, 23)), ((8, 31), (0, 11))):
            records.append(_record(ragged.offsets[i], images[i], (17, 14, 13, 11), resized, corner, name))   # the block alone
            owners.append(i)
            flat.append(len(records) - 1)
        for window, resized, corner in (((9, 8, 29, 23), (8, 8), (0, 0)), ((14, 11, 12, 10), (31, 29), (2, 3)),
                                        ((0, 0, 47, 40), (94, 80), (30, 26)), ((15, 12, 8, 8), (8, 8), (0, 0))):
            records.append(_record(ragged.offsets[i], images[i], window, resized, corner, name))            # over its edges
            owners.append(i)
    for at in ((0, 0), (8, 6), (4, 3)):
        records.append(_record(ragged.offsets[2], images[2], (at[0], at[1], 1, 1), (9, 9), (1, 1), name))
        owners.append(2)
    got, status = _launch(dev, ragged, records, OH, OW)
    assert status == 0
    _assert_records(got, images, owners, records, OH, OW, f"{name}, clamping")
    for j in flat:
        assert (got[j] == (0 if owners[j] == 0 else 255)).all(), j
    for j, at in zip(range(len(records) - 3, len(records)), ((0, 0), (8, 6), (4, 3))):
        assert (got[j] == images[2][at[1], at[0]][:, None, None]).all(), j
    if name == "bicubic":                                                  # the restatement reaches the clamp on these records
        extremes = [1 << 21, 1 << 21]
        for i, rec in zip(owners, records):
            window = tuple(int(rec[k]) for k in ("win_x", "win_y", "win_w", "win_h"))
            resize_reference(images[i], window, (int(rec["res_w"]), int(rec["res_h"])),
                             (int(rec["out_x"]), int(rec["out_y"]), OW, OH), filter=name, extremes=extremes)
        assert extremes[0] < 0 and extremes[1] >> 22 > 255, extremes


@pytest.mark.gpu
def test_reductions_at_the_limit_chunks_and_cut_bands(dev):
    """Bicubic at a reduction of exactly 16 and box at 32, across and down (65 and 33 taps); a row cut into column
    chunks (65 bicubic taps a column: 4096 / 65 = 63 columns < 70; 33 box taps: 124 < 130); a band cut to fit the stage
    (bicubic, 16 down at 200 columns of 3 bytes: 68 source rows fit, 8 output rows need 128)."""
    rng = np.random.RandomState(6)
    cases = [(structured(rng, 9, 120, 3), (3, 1, 112, 7), (7, 7), 7, 7, "bicubic"),
             (structured(rng, 120, 9, 3, two_level=True), (1, 3, 7, 112), (7, 7), 7, 7, "bicubic"),
             (structured(rng, 9, 230, 3), (0, 0, 224, 7), (7, 7), 7, 7, "box"),
             (structured(rng, 230, 9, 1), (2, 6, 7, 224), (7, 7), 7, 7, "box"),
             (structured(rng, 5, 1121, 3, two_level=True), (1, 1, 1120, 3), (70, 3), 3, 70, "bicubic"),
             (structured(rng, 4, 1121, 1), (0, 0, 1120, 4), (70, 2), 2, 70, "bicubic"),
             (structured(rng, 3, 4161, 3), (1, 0, 4160, 3), (130, 3), 3, 130, "box"),
             (structured(rng, 130, 201, 3, two_level=True), (1, 2, 200, 128), (200, 8), 8, 200, "bicubic"),
             (structured(rng, 257, 213, 3), (0, 1, 212, 256), (212, 8), 8, 212, "box")]
    for img, window, resized, OH, OW, name in cases:
        ragged = pack_images([img])
        rec = _record(0, img, window, resized, (0, 0), name)
        got, status = _launch(dev, ragged, [rec, rec], OH, OW)
        assert status == 0
        _assert_records(got, [img], [0, 0], [rec, rec], OH, OW, f"{name} {img.shape} -> {resized}")


@pytest.mark.gpu
def test_one_table_mixes_the_three_filters(dev):
    """Records of the three filters in turn, every pair on one source with two different filters; every record equals
    its own filter's restatement, whatever the band."""
    rng = np.random.RandomState(70)
    OH, OW = 9, 6
    images, ragged, owners, records = _mixed_table(rng, 3, OH, OW, FILTERS)
    assert all(int(records[2 * s]["filter"]) != int(records[2 * s + 1]["filter"]) for s in range(6))
    assert sorted({int(r["filter"]) for r in records}) == [0, 1, 2]
    # the whole of one source under the three filters
    h, w = images[0].shape[:2]
    for name in FILTERS:
        records.append(_record(ragged.offsets[0], images[0], (0, 0, w, h), (OW + 1, OH + 2), (1, 0), name))
        owners.append(0)
    want = [_want(images, i, rec, OH, OW) for i, rec in zip(owners, records)]
    assert not np.array_equal(want[-1], want[-2]) and not np.array_equal(want[-2], want[-3])
    for band_rows in (0, 1, 4, 32):
        got, status = _launch(dev, ragged, records, OH, OW, band_rows=band_rows)
        assert status == 0
        bad = [(i, int(records[i]["filter"])) for i in range(len(records)) if not np.array_equal(got[i], want[i])]
        assert not bad, (band_rows, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ratio", 3, -1])
def test_a_bad_filter_or_ratio_is_zeroed_and_reported(dev, kind):
    """A bicubic reduction above 16 (145 rows to 9; exactly 16 is resampled in the test above) and a filter outside 0..2: the
    record's image is 0, the status word says which, the neighbours in the table are exact."""
    images, ragged, table, good, bit = _bad_record_table(kind)
    got, status = _launch(dev, ragged, table, 9, 7)
    assert status == bit
    assert not got[1].any()
    _assert_records(got[[0, 2]], images, [0, 1], good, 9, 7, f"bad {kind}")
    if kind == "ratio":                                                    # the same geometry is fine for bilinear and box
        for name in ("bilinear", "box"):
            ok = table[1].copy()
            ok["filter"] = FILTERS.index(name)
            got, status = _launch(dev, ragged, [ok], 9, 7)
            assert status == 0
            _assert_records(got, images, [1], [ok], 9, 7, name)


@pytest.mark.gpu
def test_device_equals_the_recorded_pillow_outputs(dev):
    g, cases, images = _golden()
    for k, (i, wx, wy, ww, wh, rw, rh) in enumerate(cases):               # one launch per case: the output size varies
        records = [_record(0, images[i], (wx, wy, ww, wh), (rw, rh), (0, 0), name) for name in FILTERS]
        got, status = _launch(dev, pack_images([images[i]]), records, rh, rw)
        assert status == 0
        for j, name in enumerate(FILTERS):
            assert np.array_equal(got[j], g[f"out_{name}_{k}"].transpose(2, 0, 1)), (k, name, cases[k])


@pytest.mark.gpu
def test_a_photograph_sized_image_with_a_filter_per_view(dev):
    """375 x 500 x 3 -> a bicubic clean view and a bilinear augmented one at 224 through ``ResizeCrop``: both equal
    their restatements, and a steady-state call is still one kernel launch and one host-to-device copy."""
    from torch.profiler import ProfilerActivity, profile
    rng = np.random.RandomState(9)
    img = structured(rng, 375, 500, 3)
    rc = ResizeCrop(224, 0.875, device=dev, interpolation={"clean": "bicubic", "augmented": "bilinear"})
    crops = CropParams([31], [77], [289], [333])
    ragged = pack_images([img]).to(dev)
    views = rc(ragged, crops)
    assert set(views) == {"clean", "augmented"} and all(v.shape == (1, 3, 224, 224) for v in views.values())
    clean = resize_reference(img, (0, 0, 500, 375), (341, 256), (58, 16, 224, 224), filter="bicubic").transpose(2, 0, 1)
    augmented = resize_reference(img, (77, 31, 333, 289), (224, 224)).transpose(2, 0, 1)
    assert np.array_equal(views["clean"][0].cpu().numpy(), clean)
    assert np.array_equal(views["augmented"][0].cpu().numpy(), augmented)
    assert rc.status() == 0
    bilinear_clean = resize_reference(img, (0, 0, 500, 375), (341, 256), (58, 16, 224, 224)).transpose(2, 0, 1)
    assert not np.array_equal(clean, bilinear_clean)
    for _ in range(4):
        rc(ragged, crops)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(7):
            views = rc(ragged, crops)
        torch.cuda.synchronize()
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    copies = [e for e in device_events if "memcpy" in e.name.lower()]
    memsets = [e for e in device_events if "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in copies and e not in memsets]
    ours = [e for e in kernels if "resize_crop_kernel" in e.name]
    assert not memsets, sorted({e.name for e in memsets})
    if ours:
        print(f"[resize_filters] profiler: {len(kernels)} kernels ({len(ours)} resize_crop_kernel), {len(copies)} copies "
              "in 7 calls")
        assert len(ours) == 7 and len(kernels) == 7, sorted({e.name for e in kernels})
        assert len(copies) == 7 and not any("dtoh" in e.name.lower().replace(" ", "") for e in copies), \
            sorted({e.name for e in copies})
    else:
        print("[resize_filters] the profiler does not see the ctypes launches here "
              f"({len(kernels)} device kernels, {len(copies)} copies seen by it)")
        assert not kernels and len(copies) in (0, 7)
    assert np.array_equal(views["clean"][0].cpu().numpy(), clean) and rc.status() == 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inside the trainer and the validation loop
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(shapes=((20, 27, 3), (33, 19, 3), (16, 16, 3), (40, 41, 3)), seed=1):
    rng = np.random.RandomState(seed)
    images = [structured(rng, *s, two_level=i == 2) for i, s in enumerate(shapes)]
    return images, pack_images(images)


@pytest.mark.gpu
@pytest.mark.parametrize("interpolation", [{"clean": "bicubic", "augmented": "bilinear"}, "box"])
def test_trainer_prepares_both_views_with_their_filters_and_steps(dev, interpolation):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    images, ragged = _ragged()
    crops = draw_crop_params(ragged.sizes, generator=torch.Generator().manual_seed(2))
    student, teacher = _toy_models(dev)
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 16), mixup="fused",
                   image_stats=STATS, resize_crop=True, resize_interpolation=interpolation)
    batch = {"images": ragged, "label": torch.arange(4) % 10, "crop_params": crops}
    clean, augmented = tr.prepare_views(batch)
    rec = make_records(ragged.sizes, 16, 0.875, crops, interpolation=interpolation)
    want_clean, want_augmented = (np.stack([_want(images, b, part[b], 16, 16) for b in range(4)])
                                  for part in (rec[:4], rec[4:]))
    assert clean.dtype == torch.uint8 and clean.shape == (4, 3, 16, 16) and augmented.shape == (4, 3, 16, 16)
    assert np.array_equal(clean.cpu().numpy(), want_clean) and np.array_equal(augmented.cpu().numpy(), want_augmented)
    plain = make_records(ragged.sizes, 16, 0.875, crops)
    assert not np.array_equal(want_clean, np.stack([_want(images, b, plain[b], 16, 16) for b in range(4)]))
    torch.manual_seed(77)
    assert torch.isfinite(tr.train_step(batch)["loss"])
    assert tr._resizer.status() == 0


@pytest.mark.gpu
def test_evaluate_model_resamples_with_the_clean_filter(dev):
    """The same dict as on the uint8 batches the bicubic restatement makes of the same images."""
    from basd_amd.evaluation import evaluate_model
    rng = np.random.RandomState(14)
    student, _ = _toy_models(dev)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    ragged_loader, uint8_loader, differ = [], [], 0
    for n in (5, 7, 4):
        images = [structured(rng, rng.randint(12, 40), rng.randint(12, 40), 3, two_level=j % 2 == 1) for j in range(n)]
        label = torch.from_numpy(rng.randint(0, 10, n))
        ragged = pack_images(images)
        ragged_loader.append({"images": ragged, "label": label})
        rec = make_records(ragged.sizes, 16, 0.875, views=("clean",), interpolation="bicubic")
        clean = np.ascontiguousarray(np.stack([_want(images, b, rec[b], 16, 16) for b in range(n)]))     # dense NCHW
        plain = make_records(ragged.sizes, 16, 0.875, views=("clean",))
        differ += sum(not np.array_equal(clean[b], _want(images, b, plain[b], 16, 16)) for b in range(n))
        uint8_loader.append({"pixel_values": torch.from_numpy(clean), "label": label})
    assert differ >= 12
    kw = dict(num_classes=10, image_stats=(MEAN, STD))
    # the augmented entry plays no part in validation
    for interpolation in ("bicubic", {"clean": "bicubic", "augmented": "box"}):
        rc = ResizeCrop(16, 0.875, device=dev, interpolation=interpolation)
        got = evaluate_model(student, ragged_loader, criterion, resize_crop=rc, **kw)
        want = evaluate_model(student, uint8_loader, criterion, **kw)
        assert got == want and np.isfinite(got["loss"]) and rc.status() == 0
