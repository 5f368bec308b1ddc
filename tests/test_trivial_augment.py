"""TrivialAugmentWide and the flip for uint8 batches (``basd_amd.trivial_augment`` / ``csrc/taug.hip``).

Three layers: the specification in ``include/basd_hip.h`` restated in numpy below (``restate``) is held to Pillow -- live
where Pillow is installed, and always to Pillow 12.2.0's outputs recorded in ``tests/golden/trivial_augment.npz`` --
and the kernel is held to the restatement bit for bit.  Rotation is the one operation with an exclusion rule: a pixel
counts only if its fp64 source coordinate lies farther than 1 / 256 from an integer in both axes (Pillow walks the source
coordinate in 16.16 fixed point), and the excluded share is capped at 15 %.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import trivial_augment as TA
from basd_amd.trivial_augment import AugmentParams, TrivialAugment, draw_augment_params, make_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trivial_augment.npz")
BINS = (0, 1, 15, 30)
ROTATE_EXCLUSION = 1.0 / 256.0
ROTATE_CAP = 0.15


# ---------------------------------------------------------------------------------------------------------------------
# the specification, restated
# ---------------------------------------------------------------------------------------------------------------------
def source_coordinates(a, H, W):
    """fp64, left to right, every product and sum rounded on its own."""
    xc = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    yc = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    fx = ((a[0] * xc) + (a[1] * yc)) + a[2]
    fy = ((a[3] * xc) + (a[4] * yc)) + a[5]
    return fx, fy


def _affine(src, a):
    C, H, W = src.shape
    fx, fy = source_coordinates(a, H, W)
    sx, sy = np.floor(fx), np.floor(fy)
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    ix = np.where(inside, sx, 0).astype(np.int64)
    iy = np.where(inside, sy, 0).astype(np.int64)
    return np.where(inside[None], src[:, iy, ix], 0).astype(np.uint8)


def _blend(a, b, f):
    """t = float(a) + f * float(b - a): one fp32 product, one fp32 sum."""
    f = np.float32(f)
    t = a.astype(np.float32) + f * (b.astype(np.int32) - a.astype(np.int32)).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def _grey(src):
    s = src.astype(np.int64)
    return ((19595 * s[0] + 38470 * s[1] + 7471 * s[2] + 32768) >> 16).astype(np.uint8)


def _smooth(src):
    C, H, W = src.shape
    out = src.copy()
    if H < 3 or W < 3:
        return out
    k = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)
    acc = np.full((C, H - 2, W - 2), 0.5, dtype=np.float32)
    i = 0
    for dy in range(3):
        for dx in range(3):
            acc = acc + src[:, dy:dy + H - 2, dx:dx + W - 2].astype(np.float32) * k[i]
            i += 1
    assert acc.dtype == np.float32
    out[:, 1:-1, 1:-1] = np.clip(np.floor(acc), 0, 255).astype(np.uint8)
    return out


def _autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], dtype=np.uint8)


def _equalize_lut(h):
    nz = np.nonzero(h)[0]
    if len(nz) < 2:
        return np.arange(256, dtype=np.uint8)
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def restate(img, rec):
    """``img``: (C, H, W) uint8; ``rec``: one record of ``make_records``.  op(flip(image))."""
    src = np.ascontiguousarray(img[:, :, ::-1]) if int(rec["flip"]) else img
    C, H, W = src.shape
    op = int(rec["op"])
    if op <= TA.ROTATE:
        return _affine(src, [float(v) for v in rec["a"]])
    f = np.float32(rec["farg"])
    if op == TA.BRIGHTNESS:
        return _blend(np.zeros_like(src), src, f)
    if op == TA.COLOR:
        if C == 1:
            return src.copy()
        return _blend(np.broadcast_to(_grey(src), src.shape), src, f)
    if op == TA.CONTRAST:
        g = _grey(src) if C == 3 else src[0]
        mean = int(np.floor(int(g.astype(np.int64).sum()) / (H * W) + 0.5))
        return _blend(np.full_like(src, mean), src, f)
    if op == TA.SHARPNESS:
        return _blend(_smooth(src), src, f)
    if op == TA.POSTERIZE:
        return src & np.uint8((0xFF << (8 - int(rec["iarg"]))) & 0xFF)
    if op == TA.SOLARIZE:
        return np.where(src.astype(np.float32) < f, src, 255 - src).astype(np.uint8)
    lut_of = _autocontrast_lut if op == TA.AUTOCONTRAST else _equalize_lut
    assert op in (TA.AUTOCONTRAST, TA.EQUALIZE)
    return np.stack([lut_of(np.bincount(src[c].ravel(), minlength=256))[src[c]] for c in range(C)])


def rotate_mask(rec, H, W):
    """Pixels of a Rotate that count: the source coordinate is farther than 1 / 256 from an integer in both axes."""
    fx, fy = source_coordinates([float(v) for v in rec["a"]], H, W)
    return (np.abs(fx - np.round(fx)) > ROTATE_EXCLUSION) & (np.abs(fy - np.round(fy)) > ROTATE_EXCLUSION)


# ---------------------------------------------------------------------------------------------------------------------
# Pillow's side
# ---------------------------------------------------------------------------------------------------------------------
def pillow_apply(img, rec, m):
    """The same operation by Pillow's own entry points; ``m``: the magnitude (``TA.magnitude``)."""
    from PIL import Image, ImageEnhance, ImageOps
    C = img.shape[0]
    im = Image.fromarray(img[0], "L") if C == 1 else Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB")
    if int(rec["flip"]):
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    op = int(rec["op"])
    if op == TA.IDENTITY:
        out = im.copy()
    elif op in (TA.SHEAR_X, TA.SHEAR_Y, TA.TRANSLATE_X, TA.TRANSLATE_Y):
        out = im.transform(im.size, Image.AFFINE, tuple(float(v) for v in rec["a"]), Image.NEAREST, fillcolor=0)
    elif op == TA.ROTATE:
        out = im.rotate(m, Image.NEAREST, expand=False, fillcolor=0)
    elif op == TA.BRIGHTNESS:
        out = ImageEnhance.Brightness(im).enhance(float(rec["farg"]))
    elif op == TA.COLOR:
        out = ImageEnhance.Color(im).enhance(float(rec["farg"]))
    elif op == TA.CONTRAST:
        out = ImageEnhance.Contrast(im).enhance(float(rec["farg"]))
    elif op == TA.SHARPNESS:
        out = ImageEnhance.Sharpness(im).enhance(float(rec["farg"]))
    elif op == TA.POSTERIZE:
        out = ImageOps.posterize(im, int(rec["iarg"]))
    elif op == TA.SOLARIZE:
        out = ImageOps.solarize(im, float(rec["farg"]))
    elif op == TA.AUTOCONTRAST:
        out = ImageOps.autocontrast(im)
    else:
        out = ImageOps.equalize(im)
    arr = np.asarray(out)
    return arr[None].copy() if C == 1 else np.ascontiguousarray(arr.transpose(2, 0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# inputs (shared with tests/golden/make_goldens_trivial_augment.py)
# ---------------------------------------------------------------------------------------------------------------------
def golden_images():
    """A few images of at most 40 pixels a side: random ones at odd sizes, a narrow value range, a constant image, an
    image with two grey levels, one channel, and H or W equal to 3."""
    rng = np.random.RandomState(20240607)
    images = [rng.randint(0, 256, (3, 23, 39)).astype(np.uint8),
              rng.randint(40, 200, (3, 39, 24)).astype(np.uint8),
              rng.randint(0, 256, (3, 16, 16)).astype(np.uint8),
              np.full((3, 9, 13), 77, dtype=np.uint8),
              np.where(rng.rand(3, 12, 10) < 0.3, 60, 190).astype(np.uint8),
              rng.randint(0, 256, (1, 17, 21)).astype(np.uint8),
              rng.randint(0, 256, (3, 3, 11)).astype(np.uint8),
              rng.randint(0, 256, (3, 12, 3)).astype(np.uint8),
              rng.randint(0, 256, (3, 5, 7)).astype(np.uint8)]
    images[3][1] = 200                                     # constant per channel, channels differ
    return images


def golden_entries(n_images):
    """(image, op, bin, sign, flip): every op at bins 0, 1, 15 and 30 with both signs, walking through the images; the
    degenerate images (3: constant, 4: two levels, 5: one channel, 6 / 7: a side of 3) meet every op once more."""
    entries, k = [], 0
    for op in range(len(TA.OPS)):
        for b in BINS:
            for sign in (0, 1):
                entries.append((k % n_images, op, b, sign, (k // 2) % 2))
                k += 1
        for j, image in enumerate((3, 4, 5, 6, 7)):
            entries.append((image, op, (1, 15, 30)[j % 3], j % 2, (j + op) % 2))
    return entries


def _params_of(entries):
    e = np.asarray(entries)
    return AugmentParams(torch.from_numpy(e[:, 1].copy()), torch.from_numpy(e[:, 2].copy()),
                         torch.from_numpy(e[:, 3].astype(bool)), torch.from_numpy(e[:, 4].astype(bool)))


def _record(entry, H, W):
    _, op, b, sign, flip = entry
    return make_records(AugmentParams([op], [b], [bool(sign)], [bool(flip)]), H, W)[0]


def _check_against(expected_of, what):
    """The restatement against ``expected_of(k, image, record, magnitude)`` over the golden entries."""
    images = golden_images()
    entries = golden_entries(len(images))
    counted = excluded = 0
    for k, entry in enumerate(entries):
        img = images[entry[0]]
        rec = _record(entry, img.shape[1], img.shape[2])
        m = TA.magnitude(entry[1], entry[2], bool(entry[3]))
        got, want = restate(img, rec), expected_of(k, img, rec, m)
        assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
        if entry[1] == TA.ROTATE:
            mask = rotate_mask(rec, img.shape[1], img.shape[2])
            counted += mask.size
            excluded += int((~mask).sum())
            assert np.array_equal(got[:, mask], want[:, mask]), f"{what}: entry {k} {entry}"
        else:
            assert np.array_equal(got, want), (f"{what}: entry {k} {entry} ({TA.OPS[entry[1]]}): "
                                               f"{int((got != want).sum())} bytes differ")
    share = excluded / counted
    print(f"[trivial_augment] {what}: {len(entries)} entries, Rotate excluded {excluded} of {counted} pixels "
          f"({100 * share:.1f} %)")
    assert share <= ROTATE_CAP


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against Pillow
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow():
    pytest.importorskip("PIL")
    _check_against(lambda k, img, rec, m: pillow_apply(img, rec, m), "live Pillow")


def test_restatement_equals_the_recorded_pillow_outputs():
    g = np.load(GOLDEN, allow_pickle=False)
    images = golden_images()
    entries = golden_entries(len(images))
    assert np.array_equal(g["entries"], np.asarray(entries))
    for i, img in enumerate(images):
        assert np.array_equal(g[f"image_{i}"], img)
    _check_against(lambda k, img, rec, m: g[f"out_{k}"], f"Pillow {str(g['pillow_version'])} recorded")


def test_degenerate_inputs_stay_as_the_specification_says():
    images = golden_images()
    const, two = images[3], images[4]
    for op in (TA.AUTOCONTRAST, TA.EQUALIZE):
        rec = _record((0, op, 15, 0, 0), *const.shape[1:])
        assert np.array_equal(restate(const, rec), const)
    rec = _record((0, TA.AUTOCONTRAST, 15, 0, 0), *two.shape[1:])
    assert set(np.unique(restate(two, rec))) == {0, 255}
    grey = images[5]
    rec = _record((0, TA.COLOR, 30, 1, 0), *grey.shape[1:])
    assert np.array_equal(restate(grey, rec), grey)
    thin = images[6]                                                   # H = 3: one interior row
    rec = _record((0, TA.SHARPNESS, 30, 1, 0), *thin.shape[1:])        # f = 0.01: almost the smoothed image
    out = restate(thin, rec)
    assert np.array_equal(out[:, 0], thin[:, 0]) and np.array_equal(out[:, 2], thin[:, 2])
    assert not np.array_equal(out[:, 1, 1:-1], thin[:, 1, 1:-1])


def test_rotations_pillow_transposes_are_exact_integer_maps():
    x = np.arange(3 * 6 * 6, dtype=np.uint8).reshape(3, 6, 6)
    for deg, want in ((90.0, np.rot90(x, 1, (1, 2))), (-90.0, np.rot90(x, -1, (1, 2))), (180.0, x[:, ::-1, ::-1]),
                      (270.0, np.rot90(x, -1, (1, 2))), (0.0, x), (360.0, x)):
        rec = np.zeros(1, dtype=TA.RECORD_DTYPE)[0]
        rec["op"], rec["a"] = TA.ROTATE, TA.rotation_matrix(deg, 6, 6)
        assert np.array_equal(restate(x, rec), want), deg
        assert rotate_mask(rec, 6, 6).all()                             # half-integer coordinates: nothing excluded
    y = np.arange(3 * 4 * 7, dtype=np.uint8).reshape(3, 4, 7)
    rec = np.zeros(1, dtype=TA.RECORD_DTYPE)[0]
    rec["op"], rec["a"] = TA.ROTATE, TA.rotation_matrix(180.0, 4, 7)
    assert np.array_equal(restate(y, rec), y[:, ::-1, ::-1])


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the draws and the record table
# ---------------------------------------------------------------------------------------------------------------------
def test_draws_are_reproducible_and_in_range():
    a = draw_augment_params(500, generator=torch.Generator().manual_seed(5))
    b = draw_augment_params(500, generator=torch.Generator().manual_seed(5))
    c = draw_augment_params(500, generator=torch.Generator().manual_seed(6))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a.op, c.op)
    assert a.op.dtype == torch.int64 and a.sign.dtype == torch.bool and a.flip.dtype == torch.bool
    assert set(a.op.tolist()) == set(range(14)) and set(a.bin.tolist()) == set(range(31))
    assert 0.35 < a.sign.float().mean() < 0.65 and 0.35 < a.flip.float().mean() < 0.65
    # the order of the draws: op, bin, sign, flip, each for the whole batch
    g = torch.Generator().manual_seed(5)
    assert torch.equal(a.op, torch.randint(14, (500,), generator=g))
    assert torch.equal(a.bin, torch.randint(31, (500,), generator=g))
    assert torch.equal(a.sign, torch.rand(500, generator=g) <= 0.5)
    assert torch.equal(a.flip, torch.rand(500, generator=g) < 0.5)
    torch.manual_seed(9)
    d = draw_augment_params(7)
    torch.manual_seed(9)
    assert torch.equal(d.op, draw_augment_params(7).op)                 # generator=None: the global one


def test_flip_probability_zero_and_one():
    g = torch.Generator().manual_seed(1)
    assert not draw_augment_params(300, flip_p=0.0, generator=g).flip.any()
    assert draw_augment_params(300, flip_p=1.0, generator=g).flip.all()
    with pytest.raises(ValueError, match="flip_p"):
        draw_augment_params(3, flip_p=1.5)
    with pytest.raises(ValueError, match="31 bins"):
        draw_augment_params(3, num_bins=30)
    assert draw_augment_params(0).op.numel() == 0


def test_unsigned_ops_ignore_the_sign():
    for op in (TA.IDENTITY, TA.POSTERIZE, TA.SOLARIZE, TA.AUTOCONTRAST, TA.EQUALIZE):
        assert op not in TA.SIGNED
        for b in BINS:
            p = make_records(AugmentParams([op, op], [b, b], [False, True], [False, False]), 19, 23)
            assert p[0].tobytes() == p[1].tobytes()
    for op in sorted(TA.SIGNED):
        p = make_records(AugmentParams([op, op], [15, 15], [False, True], [False, False]), 19, 23)
        assert p[0].tobytes() != p[1].tobytes()
        assert TA.magnitude(op, 15, True) == -TA.magnitude(op, 15, False)
        q = make_records(AugmentParams([op, op], [0, 0], [False, True], [False, False]), 19, 23)
        assert np.array_equal(q["a"][0], q["a"][1])                      # magnitude 0: the identity either way
        assert np.array_equal(q["a"][0], [1, 0, 0, 0, 1, 0])


def test_magnitude_tables():
    bits = (8 - (torch.arange(31) / ((31 - 1) / 6))).round().int()
    assert torch.equal(TA.posterize_bits(), bits) and int(bits[0]) == 8 and int(bits[30]) == 2
    rec = make_records(AugmentParams([TA.POSTERIZE] * 31, list(range(31)), [False] * 31, [False] * 31), 8, 8)
    assert rec["iarg"].tolist() == bits.tolist()
    shear = torch.linspace(0.0, 0.99, 31)
    translate = torch.linspace(0.0, 32.0, 31)
    rotate = torch.linspace(0.0, 135.0, 31)
    solar = torch.linspace(1.0, 0.0, 31)
    for b in range(31):
        assert TA.magnitude(TA.SHEAR_X, b, False) == float(shear[b])
        assert TA.magnitude(TA.ROTATE, b, True) == -float(rotate[b])
        assert TA.magnitude(TA.SOLARIZE, b, True) == 255.0 * float(solar[b])
        for sign in (False, True):
            m = TA.magnitude(TA.TRANSLATE_X, b, sign)
            r = make_records(AugmentParams([TA.TRANSLATE_X, TA.TRANSLATE_Y], [b, b], [sign, sign], [False, True]), 9, 9)
            assert m == (-1 if sign else 1) * float(translate[b])
            assert r["a"][0].tolist() == [1, 0, -int(m), 0, 1, 0]        # int(m): towards zero, not floor
            assert r["a"][1].tolist() == [1, 0, 0, 0, 1, -int(m)] and r["flip"].tolist() == [0, 1]
    assert int(TA.magnitude(TA.TRANSLATE_X, 1, True)) == -1 and TA.magnitude(TA.TRANSLATE_X, 1, True) < -1.06
    r = make_records(AugmentParams([TA.BRIGHTNESS, TA.SOLARIZE], [30, 2], [True, False], [False, False]), 9, 9)
    assert r["farg"][0] == np.float32(1.0 + -float(shear[30])) and r["farg"][1] == np.float32(255.0 * float(solar[2]))
    assert TA.RECORD_DTYPE.itemsize == 64


# ---------------------------------------------------------------------------------------------------------------------
# CPU: argument errors come before the device
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_on_cpu():
    aug = TrivialAugment(device="cpu")
    x = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        aug(torch.zeros(4, 3, 8, 8))
    with pytest.raises(ValueError, match="dense NCHW"):
        aug(x.to(memory_format=torch.channels_last))
    with pytest.raises(ValueError, match=r"1 or 3 channels.*\(4, 2, 8, 8\)"):
        aug(torch.zeros(4, 2, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
        aug(x[0])
    buf = torch.zeros(2 * x.numel(), dtype=torch.uint8)
    src = buf[:x.numel()].view(4, 3, 8, 8)
    with pytest.raises(ValueError, match="overlaps"):
        aug(src, out=buf[x.numel() - 1:2 * x.numel() - 1].view(4, 3, 8, 8))
    with pytest.raises(ValueError, match="overlaps"):
        aug(src, out=src)
    with pytest.raises(TypeError, match="out must be uint8"):
        aug(x, out=torch.zeros(4, 3, 8, 8))
    with pytest.raises(ValueError, match="entries for a batch of 4"):
        aug(x, draw_augment_params(3))
    with pytest.raises(ValueError, match="op must lie"):
        aug(x, AugmentParams([0, 1, 2, 14], [0] * 4, [False] * 4, [False] * 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(x, out=buf[x.numel():].view(4, 3, 8, 8))                    # everything is in order but the device


def test_exported_from_the_package():
    import basd_amd
    from basd_amd import _lib
    assert "trivial_augment" in basd_amd.__doc__
    assert "basd_trivial_augment" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    assert "int basd_trivial_augment(" in header and "BasdTaugRecord" in header


def _config(points=4, classes=10):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=points), model=SimpleNamespace(num_classes=classes))


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
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    return student, SM.make_teacher(teacher, 32)


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STATS = {"clean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "augmented": (MEAN, STD)}


def _uint8_batch(B=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {"clean": torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8),
            "augmented": torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8),
            "label": torch.arange(B) % 10}


def test_trainer_argument_errors_on_cpu():
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models()
    kw = dict(student_info=SM.probe_model(student, 32), loss_cls=OracleBASD)
    with pytest.raises(ValueError, match="trivial_augment.*image_stats"):
        T.Trainer(student, _config(), teacher, mixup="fused", trivial_augment=True, **kw)       # no image_stats
    with pytest.raises(ValueError, match="trivial_augment.*mixup='fused'"):
        T.Trainer(student, _config(), teacher, mixup=True, image_stats=STATS, trivial_augment=True, **kw)
    with pytest.raises(ValueError, match="flip_p"):
        T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, trivial_augment=True, flip_p=2.0, **kw)
    tr = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, trivial_augment=True, flip_p=0.25, **kw)
    assert isinstance(tr._augmenter, TrivialAugment) and tr._augmenter.flip_p == 0.25
    batch = _uint8_batch()
    batch["augmented"] = batch["augmented"].float()
    with pytest.raises(TypeError, match="trivial_augment.*uint8.*torch.float32"):
        tr.train_step(batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.train_step(_uint8_batch())                                   # everything is in order but the device
    assert T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, **kw)._augmenter is None


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _restate_batch(x, params):
    rec = make_records(params, x.shape[2], x.shape[3])
    return np.stack([restate(x[i], rec[i]) for i in range(x.shape[0])])


def _assert_batch(got, want, params, what):
    got = got.cpu().numpy()
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
    detail = [(i, TA.OPS[int(params.op[i])], int(params.bin[i]), bool(params.sign[i]), bool(params.flip[i]),
               int((got[i] != want[i]).sum())) for i in bad[:8]]
    assert not bad, f"{what}: {len(bad)} of {want.shape[0]} images differ: (index, op, bin, sign, flip, bytes) {detail}"


def _every_op_batch(C, H, W, seed):
    """14 x 4 images: every op at bins 1 and 30 with both signs; the first image of each histogram op (and of Contrast)
    is constant, the second has two levels, one image has a narrow range."""
    rng = np.random.RandomState(seed)
    ops, bins, signs = [], [], []
    x = rng.randint(0, 256, (56, C, H, W)).astype(np.uint8)
    for op in range(14):
        for j, (b, s) in enumerate(((1, False), (1, True), (30, False), (30, True))):
            ops.append(op), bins.append(b), signs.append(s)
        if op in (TA.CONTRAST, TA.AUTOCONTRAST, TA.EQUALIZE):
            x[4 * op] = rng.randint(0, 256, (C, 1, 1))
            x[4 * op + 1] = np.where(rng.rand(C, H, W) < 0.4, 31, 222)
            x[4 * op + 2] = rng.randint(90, 140, (C, H, W))
    return x, ops, bins, signs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rgb", "rgb_flipped", "grey"])
def test_every_op_equals_the_restatement(dev, case):
    C = 1 if case == "grey" else 3
    x, ops, bins, signs = _every_op_batch(C, 37, 29, 11 + C)
    flips = [case == "rgb_flipped" or (case == "grey" and i % 2 == 1) for i in range(56)]
    params = AugmentParams(torch.tensor(ops), torch.tensor(bins), torch.tensor(signs), torch.tensor(flips))
    aug = TrivialAugment(device=dev)
    got = aug(torch.from_numpy(x).to(dev), params)
    _assert_batch(got, _restate_batch(x, params), params, case)
    assert aug.status() == 0


_STAGING_OPS = (TA.EQUALIZE, TA.SHARPNESS, TA.ROTATE)


def _staging_params(bin_=7):
    ops = [op for op in _STAGING_OPS for _ in range(2)]
    return AugmentParams(torch.tensor(ops), torch.tensor([bin_] * 6), torch.tensor([False, True] * 3),
                         torch.tensor([False, True] * 3))


@pytest.mark.gpu
@pytest.mark.parametrize("side", [224, 240], ids=["staged_in_lds", "read_from_memory"])
def test_both_sides_of_the_staging_budget(dev, side):
    """3 x 224 x 224 = 150,528 B is the largest image staged in LDS; 3 x 240 x 240 is read from memory twice."""
    rng = np.random.RandomState(side)
    one = (rng.randint(0, 256, (3, side, side)) * rng.rand(3, side, 1) ** 2).astype(np.uint8)     # an uneven histogram
    x = np.broadcast_to(one, (6, 3, side, side)).copy()
    params = _staging_params()
    aug = TrivialAugment(device=dev)
    got = aug(torch.from_numpy(x).to(dev), params)
    _assert_batch(got, _restate_batch(x, params), params, f"side {side}")
    assert aug.status() == 0


@pytest.mark.gpu
def test_widths_1_to_17_at_odd_byte_offsets(dev):
    """The byte-wise head and tail around the 16-byte accesses: every width from 1 to 17 at H = 5, the source view at
    byte offsets 0..3 of its buffer and the destination at offsets 0..15; the bytes around the destination stay."""
    aug = TrivialAugment(device=dev)
    rng = np.random.RandomState(3)
    params = _staging_params(bin_=11)
    for W in range(1, 18):
        x = rng.randint(0, 256, (6, 3, 5, W)).astype(np.uint8)
        n, s_off, d_off = x.size, W % 4, (5 * W) % 16
        src = torch.zeros(n + 32, dtype=torch.uint8, device=dev)
        dst = torch.full((n + 48,), 0xA5, dtype=torch.uint8, device=dev)
        src[s_off:s_off + n] = torch.from_numpy(x.ravel()).to(dev)
        out = aug(src[s_off:s_off + n].view(6, 3, 5, W), params, out=dst[d_off:d_off + n].view(6, 3, 5, W))
        _assert_batch(out, _restate_batch(x, params), params, f"W = {W}")
        assert bool((dst[:d_off] == 0xA5).all()) and bool((dst[d_off + n:] == 0xA5).all()), W
    assert aug.status() == 0


@pytest.mark.gpu
def test_device_equals_the_recorded_pillow_outputs(dev):
    g = np.load(GOLDEN, allow_pickle=False)
    images = golden_images()
    entries = golden_entries(len(images))
    aug = TrivialAugment(device=dev)
    counted = excluded = 0
    for i, img in enumerate(images):                                    # one launch per image size
        mine = [k for k, e in enumerate(entries) if e[0] == i]
        params = _params_of([entries[k] for k in mine])
        x = np.broadcast_to(img, (len(mine),) + img.shape).copy()
        got = aug(torch.from_numpy(x).to(dev), params).cpu().numpy()
        rec = make_records(params, img.shape[1], img.shape[2])
        for j, k in enumerate(mine):
            want = g[f"out_{k}"]
            if entries[k][1] == TA.ROTATE:
                mask = rotate_mask(rec[j], img.shape[1], img.shape[2])
                counted += mask.size
                excluded += int((~mask).sum())
                assert np.array_equal(got[j][:, mask], want[:, mask]), entries[k]
            else:
                assert np.array_equal(got[j], want), (entries[k], TA.OPS[entries[k][1]])
    assert excluded / counted <= ROTATE_CAP
    assert aug.status() == 0


@pytest.mark.gpu
def test_one_launch_and_one_copy_per_call(dev):
    """A steady-state call is one host-to-device copy (the record table) and one kernel launch: no memset, no
    allocation on the device.  Counted with ``torch.profiler`` where it sees launches made through ctypes (the output
    says whether it does); the allocator's counter is checked either way."""
    from torch.profiler import ProfilerActivity, profile
    x = torch.randint(0, 256, (64, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(dev)
    out = torch.empty_like(x)
    aug = TrivialAugment(device=dev)
    g = torch.Generator().manual_seed(8)
    draws = [draw_augment_params(64, generator=g) for _ in range(3)]
    for i in range(6):
        aug(x, draws[i % 3], out=out)
    torch.cuda.synchronize()
    device_allocations = torch.cuda.memory_stats(dev)["num_device_alloc"]
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(21):
            aug(x, draws[i % 3], out=out)
        torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["num_device_alloc"] == device_allocations
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    copies = [e for e in device_events if "memcpy" in e.name.lower()]
    memsets = [e for e in device_events if "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in copies and e not in memsets]
    ours = [e for e in kernels if "trivial_augment_kernel" in e.name]
    assert not memsets, sorted({e.name for e in memsets})
    if ours:
        print(f"[trivial_augment] profiler: {len(kernels)} kernels ({len(ours)} trivial_augment_kernel), {len(copies)} "
              "copies in 21 calls")
        assert len(ours) == 21 and len(kernels) == 21, sorted({e.name for e in kernels})
        # the copy of the record table: one per call, never towards the host (the tracer labels a copy out of pinned
        # host memory by the pointers' attributes, "DtoD" on some runtimes, so only the direction it must not have is
        # asserted by name)
        assert len(copies) == 21 and not any("dtoh" in e.name.lower().replace(" ", "") for e in copies), \
            sorted({e.name for e in copies})
    else:
        print("[trivial_augment] the profiler does not see the ctypes launches here "
              f"({len(kernels)} device kernels, {len(copies)} copies seen by it)")
        assert not kernels and len(copies) in (0, 21)
    assert aug.status() == 0
    assert torch.equal(out.cpu(), torch.from_numpy(_restate_batch(x.cpu().numpy(), draws[20 % 3])))


@pytest.mark.gpu
def test_unknown_op_code_sets_the_status_word(dev):
    """A record with an op code outside the table (the host class never makes one): the image is copied and bit 0 of the
    status word is set; nothing is read or written out of bounds."""
    from basd_amd import _lib
    x = torch.randint(0, 256, (2, 3, 9, 11), dtype=torch.uint8).to(dev)
    out = torch.zeros_like(x)
    rec = make_records(AugmentParams([0, 0], [0, 0], [False, False], [False, True]), 9, 11)
    rec["op"][0] = 99
    table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("basd_trivial_augment", x.data_ptr(), out.data_ptr(), 2, 3, 9, 11, table.data_ptr(), status.data_ptr(),
              torch._C._cuda_getCurrentRawStream(dev.index))
    assert int(status.item()) == 1
    assert torch.equal(out[0], x[0]) and torch.equal(out[1], x[1].flip(-1))
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("basd_trivial_augment", x.data_ptr(), x.data_ptr() + 8, 2, 3, 9, 11, table.data_ptr(),
                  status.data_ptr(), torch._C._cuda_getCurrentRawStream(dev.index))
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("basd_trivial_augment", x.data_ptr(), out.data_ptr(), 2, 2, 9, 11, table.data_ptr(),
                  status.data_ptr(), torch._C._cuda_getCurrentRawStream(dev.index))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inside the trainer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_trainer_step_with_the_augmenter(dev):
    """Identity without a flip: the loss of the step without the feature, bit for bit.  Drawn params: finite, another."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    raw = _uint8_batch(4)
    losses = {}
    for name in ("off", "identity", "drawn"):
        student, teacher = _toy_models(dev)
        torch.manual_seed(42)
        tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused",
                       image_stats=STATS, trivial_augment=name != "off")
        seen = []
        student.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone()))
        batch = dict(raw)
        if name == "identity":
            batch["augment_params"] = AugmentParams([TA.IDENTITY] * 4, [0] * 4, [False] * 4, [False] * 4)
        if name == "drawn":
            batch["augment_params"] = AugmentParams([TA.SOLARIZE, TA.ROTATE, TA.EQUALIZE, TA.SHARPNESS], [20, 30, 3, 30],
                                                    [False, True, False, False], [True, False, True, True])
        torch.manual_seed(77)
        losses[name] = (tr.train_step(batch)["loss"].item(), seen[0])
        if name != "off":
            assert tr._augmenter.status() == 0
    assert losses["off"][0] == losses["identity"][0] and torch.equal(losses["off"][1], losses["identity"][1])
    assert np.isfinite(losses["drawn"][0]) and losses["drawn"][0] != losses["off"][0]
    assert not torch.equal(losses["off"][1], losses["drawn"][1])
    # without params in the batch the trainer draws its own (global CPU generator)
    student, teacher = _toy_models(dev)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused",
                   image_stats=STATS, trivial_augment=True)
    torch.manual_seed(5)
    assert torch.isfinite(tr.train_step(raw)["loss"])
