"""Pillow-exact crops and resizes of ragged uint8 batches (``basd_amd.resize`` / ``csrc/resize.hip``).

Three layers, every comparison ``array_equal`` (no tolerance, no excluded pixels): the specification in
``include/basd_hip.h`` restated in numpy (``basd_amd.resize.resize_reference``) is held to Pillow -- live where Pillow is
installed, and always to Pillow 12.2.0's outputs recorded in ``tests/golden/resize_crop.npz`` -- and the kernel is held to
the restatement.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import resize as R
from basd_amd.resize import (CropParams, RaggedBatch, ResizeCrop, collate_ragged, draw_crop_params, eval_window,
                             make_records, pack_images, resize_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_crop.npz")


def structured(rng, h, w, c, two_level=False):
    """A ramp with noise (so that a shifted or transposed read shows), or a 0 / 255 image."""
    if two_level:
        return np.where(rng.rand(h, w, c) < 0.5, 0, 255).astype(np.uint8)
    ramp = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None]
    return ((ramp + rng.randint(0, 120, (h, w, c))) % 256).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against Pillow
# ---------------------------------------------------------------------------------------------------------------------
def _pillow(img, window, resized):
    from PIL import Image
    wx, wy, ww, wh = window
    pil = Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img)
    out = np.asarray(pil.crop((wx, wy, wx + ww, wy + wh)).resize(resized, Image.BILINEAR))
    return out[:, :, None] if out.ndim == 2 else out


def test_restatement_equals_pillow():
    pytest.importorskip("PIL")
    rng = np.random.RandomState(7)
    bad = []
    for i in range(330):
        h, w, c = rng.randint(1, 90), rng.randint(1, 90), (3, 1)[i % 4 == 3]
        img = structured(rng, h, w, c, two_level=i % 3 == 0)
        ww, wh = rng.randint(1, w + 1), rng.randint(1, h + 1)
        window = (rng.randint(0, w - ww + 1), rng.randint(0, h - wh + 1), ww, wh)
        resized = (rng.randint(1, 70), rng.randint(1, 70))
        if not np.array_equal(resize_reference(img, window, resized), _pillow(img, window, resized)):
            bad.append((i, img.shape, window, resized))
    assert not bad, f"{len(bad)} of 330 cases differ: {bad[:5]}"
    img = structured(rng, 375, 500, 3)
    assert np.array_equal(resize_reference(img, (0, 0, 500, 375), (341, 256)), _pillow(img, (0, 0, 500, 375), (341, 256)))
    img = structured(rng, 1500, 2000, 3)
    window = (2, 9, 1996, 1485)
    assert np.array_equal(resize_reference(img, window, (224, 224)), _pillow(img, window, (224, 224)))


def test_restatement_equals_the_recorded_pillow_outputs():
    g = np.load(GOLDEN, allow_pickle=False)
    cases = g["cases"]
    assert 24 <= len(cases) <= 60 and str(g["pillow_version"]) == "12.2.0"
    assert os.path.getsize(GOLDEN) < 256 * 1024
    for k, (i, wx, wy, ww, wh, rw, rh) in enumerate(cases.tolist()):
        got = resize_reference(g[f"image_{i}"], (wx, wy, ww, wh), (rw, rh))
        assert np.array_equal(got, g[f"out_{k}"]), (k, cases[k].tolist())


def test_rectangle_of_the_restatement_is_a_slice():
    rng = np.random.RandomState(2)
    img = structured(rng, 23, 31, 3)
    whole = resize_reference(img, (2, 3, 25, 17), (13, 29))
    assert whole.shape == (29, 13, 3)
    assert np.array_equal(resize_reference(img, (2, 3, 25, 17), (13, 29), (4, 6, 9, 20)), whole[6:26, 4:13])
    # a pass whose size does not change is the identity
    assert np.array_equal(resize_reference(img, (2, 3, 25, 17), (25, 17)), img[3:20, 2:27])


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the two transforms
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_window_values():
    assert eval_window(375, 500, 224, 0.875) == (256, 341, 16, 58)       # (341 - 224) / 2 = 58.5 rounds to even
    assert eval_window(500, 375, 224, 0.875) == (341, 256, 58, 16)
    assert eval_window(300, 300, 224, 0.875) == (256, 256, 16, 16)
    assert eval_window(64, 64, 224, 0.875) == (256, 256, 16, 16)         # Resize enlarges a small image first
    assert eval_window(100, 333, 224, 1.0) == (224, 745, 0, 260)         # int(224 * 333 / 100) = 745; 260.5 to even
    # CenterCrop of an image smaller than the crop would pad; after Resize(round(S / ratio)) that is a ratio above 1
    with pytest.raises(ValueError, match="smaller than the crop"):
        eval_window(100, 100, 224, 2.0)
    with pytest.raises(ValueError, match="smaller than the crop"):
        eval_window(375, 500, 224, 1.01)
    with pytest.raises(ValueError, match="crop_ratio"):
        eval_window(100, 100, 224, 0.0)
    with pytest.raises(ValueError, match="positive"):
        eval_window(0, 100, 224, 0.875)


def test_draws_are_reproducible_and_inside_their_images():
    rng = np.random.RandomState(4)
    sizes = torch.from_numpy(np.stack([rng.randint(1, 600, 200), rng.randint(1, 600, 200)], 1))
    a = draw_crop_params(sizes, generator=torch.Generator().manual_seed(9))
    b = draw_crop_params(sizes, generator=torch.Generator().manual_seed(9))
    c = draw_crop_params(sizes, generator=torch.Generator().manual_seed(10))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(x, y) for x, y in zip(a, c))
    H, W = sizes[:, 0], sizes[:, 1]
    assert all(t.dtype == torch.int64 and t.shape == (200,) for t in a)
    assert bool(((a.top >= 0) & (a.left >= 0) & (a.height >= 1) & (a.width >= 1)).all())
    assert bool(((a.top + a.height <= H) & (a.left + a.width <= W)).all())
    # a window that is not the fallback has an aspect ratio inside the bounds up to the rounding of its sides: w and h
    # are each within 1/2 of their real values, whose quotient lies in [3/4, 4/3]
    checked = 0
    for i in range(200):
        h, w = int(a.height[i]), int(a.width[i])
        whole = h == int(H[i]) or w == int(W[i])                          # the fallback always keeps one full side
        if whole:
            continue
        checked += 1
        assert (w - 0.5) / (h + 0.5) <= 4.0 / 3.0 and (w + 0.5) / (h - 0.5) >= 3.0 / 4.0, (h, w)
    assert checked > 100
    # the global generator when none is given
    torch.manual_seed(3)
    d = draw_crop_params(sizes)
    torch.manual_seed(3)
    assert all(torch.equal(x, y) for x, y in zip(d, draw_crop_params(sizes)))


def test_draw_fallback_and_empty_batch():
    p = draw_crop_params(torch.tensor([[10, 1000]]), generator=torch.Generator().manual_seed(0))
    assert (int(p.height), int(p.width), int(p.top), int(p.left)) == (10, 13, 0, 493)      # 10 x 13, centred
    p = draw_crop_params(torch.tensor([[1000, 10]]), generator=torch.Generator().manual_seed(0))
    assert (int(p.height), int(p.width), int(p.top), int(p.left)) == (13, 10, 493, 0)
    e = draw_crop_params(torch.zeros(0, 2, dtype=torch.int32))
    assert all(t.shape == (0,) for t in e)
    e = draw_crop_params(pack_images([]))
    assert all(t.shape == (0,) for t in e)
    with pytest.raises(ValueError, match=r"\(B, 2\)"):
        draw_crop_params(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="scale and ratio"):
        draw_crop_params(torch.tensor([[10, 10]]), scale=(0.5, 0.1))


def test_record_table_layout_and_limits():
    sizes = torch.tensor([[375, 500], [64, 48]], dtype=torch.int32)
    crops = CropParams([10, 0], [20, 8], [300, 64], [400, 40])
    rec = make_records(sizes, 224, 0.875, crops)
    assert rec.dtype == R.RECORD_DTYPE and rec.shape == (4,) and R.RECORD_DTYPE.itemsize == 64
    assert [R.RECORD_DTYPE.fields[n][1] for n in ("src_offset", "src_h", "src_w", "win_x", "win_y", "win_w", "win_h",
                                                  "res_w", "res_h", "out_x", "out_y")] == [0, 8, 12, 16, 20, 24, 28, 32,
                                                                                          36, 40, 44]
    assert rec["src_offset"].tolist() == [0, 375 * 500 * 3] * 2
    clean, aug = rec[:2], rec[2:]
    assert (clean["win_x"].tolist(), clean["win_w"].tolist(), clean["win_h"].tolist()) == ([0, 0], [500, 48], [375, 64])
    assert (clean["res_h"].tolist(), clean["res_w"].tolist()) == ([256, 341], [341, 256])
    assert (clean["out_y"].tolist(), clean["out_x"].tolist()) == ([16, 58], [58, 16])      # 58.5 rounds to even
    assert (aug["win_y"].tolist(), aug["win_x"].tolist(), aug["win_h"].tolist(), aug["win_w"].tolist()) == (
        [10, 0], [20, 8], [300, 64], [400, 40])
    assert aug["res_w"].tolist() == [224, 224] and aug["out_x"].tolist() == [0, 0]
    only = make_records(sizes, 224, 0.875, views=("clean",), channels=1)
    assert only.shape == (2,) and only["src_offset"].tolist() == [0, 375 * 500]
    assert make_records(torch.zeros(0, 2), 224, 0.875, draw_crop_params(torch.zeros(0, 2))).shape == (0,)
    with pytest.raises(ValueError, match="does not lie inside"):
        make_records(sizes, 224, 0.875, CropParams([10, 1], [20, 8], [300, 64], [400, 40]))
    with pytest.raises(ValueError, match="does not lie inside"):
        make_records(sizes, 224, 0.875, CropParams([10, 0], [20, 8], [300, 0], [400, 40]))
    with pytest.raises(ValueError, match="more than 32 times"):
        make_records(torch.tensor([[200, 200]]), 6, 0.875, CropParams([0], [0], [193], [10]))
    with pytest.raises(ValueError, match="outside the limits"):
        make_records(torch.tensor([[200, 200]]), 2, 1.0, views=("clean",))           # 200 -> 2
    with pytest.raises(ValueError, match="needs crop_params"):
        make_records(sizes, 224, 0.875)
    with pytest.raises(ValueError, match="entries for a batch of 2"):
        make_records(sizes, 224, 0.875, CropParams([0], [0], [1], [1]))
    with pytest.raises(ValueError, match="views"):
        make_records(sizes, 224, 0.875, crops, views=("clean", "clean"))
    with pytest.raises(ValueError, match="smaller than the crop"):
        make_records(sizes, 224, 1.5, crops)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: plumbing; argument errors come before the device
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(shapes=((20, 27, 3), (33, 19, 3), (16, 16, 3), (40, 41, 3)), seed=1):
    rng = np.random.RandomState(seed)
    images = [structured(rng, *s) for s in shapes]
    return images, pack_images(images)


def test_pack_images_and_ragged_batch():
    images, ragged = _ragged()
    assert len(ragged) == 4 and ragged.channels == 3 and ragged.data.dtype == torch.uint8 and ragged.data.dim() == 1
    assert ragged.sizes.dtype == torch.int32 and ragged.sizes.tolist() == [[20, 27], [33, 19], [16, 16], [40, 41]]
    assert ragged.offsets.tolist() == [0, 1620, 1620 + 1881, 1620 + 1881 + 768]
    for i, img in enumerate(images):
        assert np.array_equal(ragged.image(i).numpy(), img)
    mixed = pack_images([images[0], torch.from_numpy(images[1]), images[2][:, :, 0:1].repeat(3, axis=2)])
    assert len(mixed) == 3 and np.array_equal(mixed.image(1).numpy(), images[1])
    grey = pack_images([images[0][:, :, 0], images[1][:, :, :1]])
    assert grey.channels == 1 and grey.nbytes == 20 * 27 + 33 * 19
    assert len(pack_images([])) == 0 and pack_images([], channels=1).channels == 1
    assert ragged.to("cpu") is ragged and ragged.to(torch.device("cpu"), non_blocking=True) is ragged
    with pytest.raises(TypeError, match="uint8"):
        pack_images([images[0].astype(np.float32)])
    with pytest.raises(TypeError, match="uint8"):
        pack_images([torch.zeros(4, 4, 3)])
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        pack_images([np.zeros((4, 4, 2), np.uint8)])
    with pytest.raises(ValueError, match="one channel count"):
        pack_images([images[0], images[1][:, :, 0]])
    with pytest.raises(ValueError, match="not be empty"):
        pack_images([np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match="sizes describe"):
        RaggedBatch(torch.zeros(10, dtype=torch.uint8), torch.tensor([[2, 2]]), 3)
    with pytest.raises(TypeError, match="1-D uint8"):
        RaggedBatch(torch.zeros(12), torch.tensor([[2, 2]]), 3)


def test_pack_images_takes_pil_images():
    Image = pytest.importorskip("PIL.Image")
    images, _ = _ragged()
    ragged = pack_images([Image.fromarray(im) for im in images])
    assert all(np.array_equal(ragged.image(i).numpy(), im) for i, im in enumerate(images))
    assert pack_images([Image.fromarray(images[0][:, :, 0])]).channels == 1


class _Decoded(torch.utils.data.Dataset):
    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return {"image": self.images[i], "label": i % 10}


def test_collate_ragged_round_trip_through_a_loader():
    rng = np.random.RandomState(5)
    images = [structured(rng, rng.randint(3, 30), rng.randint(3, 30), 3) for _ in range(10)]
    loader = torch.utils.data.DataLoader(_Decoded(images), batch_size=4, collate_fn=collate_ragged, pin_memory=False)
    seen = 0
    for batch in loader:
        ragged = batch["images"]
        assert isinstance(ragged, RaggedBatch) and set(batch) == {"images", "label"}
        assert batch["label"].tolist() == [i % 10 for i in range(seen, seen + len(ragged))]
        for j in range(len(ragged)):
            assert np.array_equal(ragged.image(j).numpy(), images[seen + j])
        seen += len(ragged)
    assert seen == 10
    pairs = collate_ragged([(images[0], 3), (images[1], 4)])
    assert pairs["label"].tolist() == [3, 4] and len(pairs["images"]) == 2
    with pytest.raises(KeyError, match="image"):
        collate_ragged([{"pixels": images[0], "label": 0}])


def test_argument_errors_on_cpu():
    with pytest.raises(ValueError, match="image_size"):
        ResizeCrop(0, 0.875, device="cpu")
    with pytest.raises(ValueError, match="crop_ratio"):
        ResizeCrop(16, 0.0, device="cpu")
    rc = ResizeCrop(16, 0.875, device="cpu")
    images, ragged = _ragged()
    with pytest.raises(TypeError, match="RaggedBatch"):
        rc(torch.zeros(4, 3, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="views"):
        rc(ragged, views=())
    with pytest.raises(ValueError, match="views"):
        rc(ragged, views=("clean", "flipped"))
    with pytest.raises(ValueError, match="entries for a batch of 4"):
        rc(ragged, draw_crop_params(ragged.sizes[:3]))
    with pytest.raises(ValueError, match="does not lie inside"):
        rc(ragged, CropParams([0, 0, 0, 0], [0, 0, 1, 0], [16] * 4, [16] * 4))          # image 2 is 16 wide
    with pytest.raises(ValueError, match="smaller than the crop"):
        ResizeCrop(16, 1.5, device="cpu")(ragged)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rc(ragged)                                                       # everything is in order but the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rc(ragged, draw_crop_params(ragged), views=("augmented",))
    assert rc.status() == 0


def test_exported_from_the_package():
    import basd_amd
    from basd_amd import _lib
    assert "``resize``" in basd_amd.__doc__
    for name in ("RaggedBatch", "ResizeCrop", "pack_images", "collate_ragged", "draw_crop_params", "eval_window",
                 "CropParams"):
        assert name in basd_amd.__all__ and getattr(basd_amd, name) is getattr(R, name)
    vp, i32, i64 = _lib.vp, _lib.i32, _lib.i64
    assert _lib.SIGNATURES["basd_resize_crop"] == [vp, i64, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    assert "int basd_resize_crop(" in header and "BasdResizeRecord" in header
    for text in ("#define BASD_RESIZE_STAGE_BYTES", "#define BASD_RESIZE_MAX_RATIO 32", "k_x = int(0.5 + w_x * 2^22)",
                 "taps clamp at the window"):
        assert text in header, text
    assert R.MAX_RATIO == 32 and R.MAX_SIDE == 1048576 and (R.BAD_GEOMETRY, R.BAD_RATIO) == (1, 2)


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


def test_trainer_and_evaluation_argument_errors_on_cpu():
    from basd_amd import trainer as T
    from basd_amd.evaluation import evaluate_model
    from tools import stock_models as SM
    student, teacher = _toy_models()
    kw = dict(student_info=SM.probe_model(student, 16), loss_cls=OracleBASD)
    with pytest.raises(ValueError, match="resize_crop.*image_stats"):
        T.Trainer(student, _config(), teacher, mixup="fused", resize_crop=True, **kw)           # no image_stats
    with pytest.raises(ValueError, match="resize_crop.*mixup='fused'"):
        T.Trainer(student, _config(), teacher, mixup=True, image_stats=STATS, resize_crop=True, **kw)
    tr = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, resize_crop=True, **kw)
    assert isinstance(tr._resizer, ResizeCrop) and (tr._resizer.image_size, tr._resizer.crop_ratio) == (16, 0.875)
    _, ragged = _ragged()
    with pytest.raises(TypeError, match="resize_crop.*RaggedBatch"):
        tr.prepare_views({"clean": torch.zeros(4, 3, 16, 16), "augmented": torch.zeros(4, 3, 16, 16),
                          "label": torch.arange(4)})
    with pytest.raises(ValueError, match="entries for a batch of 4"):
        tr.train_step({"images": ragged, "label": torch.arange(4), "crop_params": draw_crop_params(ragged.sizes[:2])})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.train_step({"images": ragged, "label": torch.arange(4)})      # everything is in order but the device
    # defaults are unchanged: no resizer, and prepare_views hands the batch's own entries over
    plain = T.Trainer(student, _config(), teacher, mixup="fused", image_stats=STATS, **kw)
    assert plain._resizer is None
    c, a = torch.zeros(2, 3, 16, 16), torch.ones(2, 3, 16, 16)
    got = plain.prepare_views({"clean": c, "augmented": a})
    assert got[0] is c and got[1] is a
    # evaluate_model: the resizer hands uint8 batches on, so it needs image_stats; decoded images need the resizer
    rc = ResizeCrop(16, 0.875, device="cpu")
    criterion = nn.CrossEntropyLoss()
    with pytest.raises(ValueError, match="resize_crop needs image_stats"):
        evaluate_model(student, [], criterion, num_classes=10, resize_crop=rc)
    with pytest.raises(TypeError, match="needs resize_crop"):
        evaluate_model(student, [{"images": ragged, "label": torch.arange(4)}], criterion, num_classes=10,
                       image_stats=(MEAN, STD))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_model(student, [{"images": ragged, "label": torch.arange(4)}], criterion, num_classes=10,
                       image_stats=(MEAN, STD), resize_crop=rc)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the restatement, byte for byte
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _record(offset, img, window, resized, corner):
    rec = np.zeros((), dtype=R.RECORD_DTYPE)
    rec["src_offset"], rec["src_h"], rec["src_w"] = offset, img.shape[0], img.shape[1]
    rec["win_x"], rec["win_y"], rec["win_w"], rec["win_h"] = window
    rec["res_w"], rec["res_h"] = resized
    rec["out_x"], rec["out_y"] = corner
    return rec


def _launch(dev, ragged, records, OH, OW, band_rows=0, src_bytes=None):
    """One raw launch: ``records`` a list of RECORD_DTYPE scalars.  Returns (n, C, OH, OW) on the host and the status."""
    from basd_amd import _lib
    table = np.stack(records) if records else np.zeros(0, dtype=R.RECORD_DTYPE)
    n, C = len(table), ragged.channels
    data = ragged.data.to(dev)
    dev_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.full((n, C, OH, OW), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("basd_resize_crop", data.data_ptr(), data.numel() if src_bytes is None else src_bytes, out.data_ptr(), n,
              C, OH, OW, dev_table.data_ptr(), status.data_ptr(), band_rows,
              torch._C._cuda_getCurrentRawStream(dev.index))
    return out.cpu().numpy(), int(status.item())


def _want(images, index, rec, OH, OW):
    """The restatement of one record: (C, OH, OW)."""
    window = tuple(int(rec[k]) for k in ("win_x", "win_y", "win_w", "win_h"))
    got = resize_reference(images[index], window, (int(rec["res_w"]), int(rec["res_h"])),
                           (int(rec["out_x"]), int(rec["out_y"]), OW, OH))
    return got.transpose(2, 0, 1)


def _assert_records(got, images, owners, records, OH, OW, what):
    bad = []
    for i, (index, rec) in enumerate(zip(owners, records)):
        want = _want(images, index, rec, OH, OW)
        if not np.array_equal(got[i], want):
            bad.append((i, rec.tolist()[:11], int((got[i] != want).sum())))
    assert not bad, f"{what}: {len(bad)} of {len(records)} records differ: (index, record, bytes) {bad[:6]}"


def _axis(rng, kind, need):
    """(window side, resized side) of one axis: resized >= need (the output rectangle must fit)."""
    if kind == "reduce" and need <= 9:
        res = rng.randint(need, 10)
        return rng.randint(res, 18), res                                # sides 1..17 -> 1..9
    if kind == "same":
        res = rng.randint(need, 18)
        return res, res
    res = rng.randint(need, 18)
    return rng.randint(1, min(9, res) + 1), res                         # sides 1..9 -> 1..17


def _mixed_table(rng, C, OH, OW):
    """Twelve records on six sources of odd widths: every pair of records shares its source; the kinds per axis cover
    reducing, enlarging and one axis unchanged with the other changed; half of the rectangles touch the far edge of
    the resized image at a corner > 0 where the sizes allow one."""
    kinds = [("reduce", "reduce"), ("enlarge", "enlarge"), ("same", "reduce"), ("reduce", "same"), ("same", "enlarge"),
             ("enlarge", "same"), ("reduce", "enlarge"), ("enlarge", "reduce"), ("same", "same"), ("reduce", "reduce"),
             ("enlarge", "enlarge"), ("enlarge", "reduce")]
    geo = []
    for i, (kx, ky) in enumerate(kinds):
        win_w, res_w = _axis(rng, kx, OW)
        win_h, res_h = _axis(rng, ky, OH)
        far = i % 2 == 0
        corner = (res_w - OW if far else rng.randint(0, res_w - OW + 1), res_h - OH if far else rng.randint(0, res_h - OH + 1))
        geo.append((win_w, win_h, res_w, res_h, corner))
    images, owners, placed = [], [], []
    for s in range(6):
        a, b = geo[2 * s], geo[2 * s + 1]
        w = max(a[0], b[0]) + rng.randint(0, 4)
        w += 1 - w % 2                                                   # odd: the next image starts at an odd offset
        h = max(a[1], b[1]) + rng.randint(0, 4)
        images.append(structured(rng, h, w, C, two_level=s == 4))
        for win_w, win_h, res_w, res_h, corner in (a, b):
            window = (rng.randint(0, w - win_w + 1), rng.randint(0, h - win_h + 1), win_w, win_h)
            owners.append(s)
            placed.append((window, (res_w, res_h), corner))
    ragged = pack_images(images)
    offsets = ragged.offsets
    records = [_record(offsets[s], images[s], *p) for s, p in zip(owners, placed)]
    return images, ragged, owners, records


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 1])
def test_mixed_tables_equal_the_restatement(dev, C):
    """Output widths 1..17 (the heights walk through 1..17 as well), one launch each over a mixed table."""
    rng = np.random.RandomState(40 + C)
    starts, far_corners, one_axis = set(), 0, 0
    for OW in range(1, 18):
        OH = (OW * 7) % 17 + 1
        images, ragged, owners, records = _mixed_table(rng, C, OH, OW)
        starts |= {int(o) % 4 for o in ragged.offsets}
        far_corners += sum(int(r["out_x"]) > 0 and int(r["out_x"]) + OW == int(r["res_w"]) for r in records)
        one_axis += sum((int(r["res_w"]) == int(r["win_w"])) != (int(r["res_h"]) == int(r["win_h"])) for r in records)
        got, status = _launch(dev, ragged, records, OH, OW)
        _assert_records(got, images, owners, records, OH, OW, f"C = {C}, OW = {OW}, OH = {OH}")
        assert status == 0
    assert starts == {0, 1, 2, 3} and far_corners >= 17 and one_axis >= 34


@pytest.mark.gpu
def test_taps_clamp_at_the_window_not_at_the_source(dev):
    """The window is 0 and everything around it 255: windows at the four corners and in the interior, reduced and
    enlarged.  Any tap outside the window would lift a byte above 0."""
    H, W, OH, OW = 40, 47, 8, 8
    images, records, owners = [], [], []
    places = [(0, 0), (W - 13, 0), (0, H - 11), (W - 13, H - 11), (17, 14)]
    for i, (wx, wy) in enumerate(places):
        img = np.full((H, W, 3), 255, np.uint8)
        img[wy:wy + 11, wx:wx + 13] = 0
        images.append(img)
    ragged = pack_images(images)
    for i, (wx, wy) in enumerate(places):
        for resized, corner in (((8, 8), (0, 0)), ((29, 31), (21, 23)), ((29, 31), (0, 0)), ((8, 31), (0, 11))):
            records.append(_record(ragged.offsets[i], images[i], (wx, wy, 13, 11), resized, corner))
            owners.append(i)
    got, status = _launch(dev, ragged, records, OH, OW)
    assert status == 0 and got.shape == (20, 3, 8, 8)
    assert not got.any(), np.argwhere(got.reshape(20, -1).any(1)).ravel().tolist()
    _assert_records(got, images, owners, records, OH, OW, "window clamping")


@pytest.mark.gpu
def test_ratios_up_to_the_limit_and_one_record_above_it(dev):
    rng = np.random.RandomState(6)
    wide, tall, dot = structured(rng, 9, 230, 3), structured(rng, 230, 9, 3), structured(rng, 3, 3, 3)
    images = [wide, tall, dot]
    ragged = pack_images(images)
    o = ragged.offsets
    good = [(0, (3, 1, 200, 7), (8, 7), (1, 0)),          # 200 x 7 -> 8 x 7: ratio 25 across
            (1, (1, 3, 7, 200), (7, 8), (0, 1)),          # ratio 25 down
            (0, (0, 0, 224, 7), (7, 7), (0, 0)),          # the documented maximum, 32, across
            (1, (2, 6, 7, 224), (7, 7), (0, 0)),          # and down
            (2, (1, 1, 1, 1), (9, 9), (2, 2)),            # 1 -> 9
            (2, (0, 2, 3, 1), (7, 9), (0, 1))]
    over = (0, (0, 0, 225, 7), (7, 7), (0, 0))            # 225 > 32 * 7
    rows = good[:3] + [over] + good[3:]
    records = [_record(o[s], images[s], w, r, c) for s, w, r, c in rows]
    got, status = _launch(dev, ragged, records, 7, 7)
    assert status == R.BAD_RATIO
    assert not got[3].any()
    keep = [i for i in range(len(rows)) if i != 3]
    _assert_records(got[keep], images, [rows[i][0] for i in keep], [records[i] for i in keep], 7, 7, "ratios")
    # the same the other way up, alone with good neighbours
    rows = [good[1], (1, (0, 0, 7, 225), (7, 7), (0, 0)), good[4]]
    records = [_record(o[s], images[s], w, r, c) for s, w, r, c in rows]
    got, status = _launch(dev, ragged, records, 7, 7)
    assert status == R.BAD_RATIO and not got[1].any()
    _assert_records(got[[0, 2]], images, [1, 2], [records[0], records[2]], 7, 7, "ratios, vertical")


@pytest.mark.gpu
def test_rows_cut_into_column_chunks(dev):
    """A row whose coefficients do not fit the table in one piece (ratio 32 across at 70 columns: 65 taps a column), and
    one whose 65 source rows a pixel do not fit the stage at its full width (ratio 32 down at 212 columns)."""
    rng = np.random.RandomState(8)
    wide, deep = structured(rng, 5, 2241, 3), structured(rng, 66, 213, 3)
    for img, window, resized, OH, OW in ((wide, (1, 1, 2240, 3), (70, 3), 3, 70), (deep, (0, 1, 212, 64), (212, 2), 2, 212),
                                         (wide[:, :, :1], (0, 0, 2240, 5), (70, 2), 2, 70)):
        ragged = pack_images([img])
        rec = _record(0, img, window, resized, (0, 0))
        got, status = _launch(dev, ragged, [rec, rec], OH, OW)
        assert status == 0
        _assert_records(got, [img], [0, 0], [rec, rec], OH, OW, f"{img.shape} -> {resized}")


@pytest.mark.gpu
def test_one_photograph_sized_image_gives_both_views(dev):
    """375 x 500 x 3 -> both views at 224: several bands and workgroups per image, through ``ResizeCrop``."""
    rng = np.random.RandomState(9)
    img = structured(rng, 375, 500, 3)
    rc = ResizeCrop(224, 0.875, device=dev)
    crops = CropParams([31], [77], [289], [333])
    views = rc(pack_images([img]).to(dev), crops)
    assert set(views) == {"clean", "augmented"} and all(v.shape == (1, 3, 224, 224) for v in views.values())
    clean = resize_reference(img, (0, 0, 500, 375), (341, 256), (58, 16, 224, 224)).transpose(2, 0, 1)
    augmented = resize_reference(img, (77, 31, 333, 289), (224, 224)).transpose(2, 0, 1)
    assert np.array_equal(views["clean"][0].cpu().numpy(), clean)
    assert np.array_equal(views["augmented"][0].cpu().numpy(), augmented)
    assert rc.status() == 0
    only = rc(pack_images([img]).to(dev), views=("clean",))
    assert set(only) == {"clean"} and np.array_equal(only["clean"][0].cpu().numpy(), clean)
    empty = rc(pack_images([]).to(dev))
    assert empty["clean"].shape == (0, 3, 224, 224) and empty["augmented"].shape == (0, 3, 224, 224)


@pytest.mark.gpu
def test_a_large_image_shrinks_the_band_to_fit_lds(dev):
    """1500 x 2000 x 3 -> 224 through a window of 0.9 of the area: 32 output rows need about 200 source rows of 672
    bytes, five times the stage, so a workgroup cuts its band; with the band the entry point chooses as well."""
    rng = np.random.RandomState(10)
    img = structured(rng, 1500, 2000, 3)
    window = (51, 38, 1897, 1423)                                        # 1897 * 1423 / 3e6 = 0.8998
    ragged = pack_images([img])
    rec = _record(0, img, window, (224, 224), (0, 0))
    want = resize_reference(img, window, (224, 224)).transpose(2, 0, 1)
    for band_rows in (32, 0):
        got, status = _launch(dev, ragged, [rec], 224, 224, band_rows=band_rows)
        assert status == 0 and np.array_equal(got[0], want), band_rows


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["window_past_the_source", "rectangle_past_the_resized_image", "offset_past_the_buffer",
                                   "source_past_the_buffer"])
def test_a_bad_record_is_zeroed_and_reported(dev, fault):
    """The record is rejected by the kernel's validation: nothing of it is read; its image is 0, the status word says
    so, and its neighbours in the table are correct."""
    rng = np.random.RandomState(12)
    images = [structured(rng, 21, 25, 3), structured(rng, 30, 19, 3)]
    ragged = pack_images(images)
    o = ragged.offsets
    good = [(0, (2, 3, 20, 15), (9, 11), (1, 2)), (1, (0, 0, 19, 30), (14, 12), (5, 3))]
    records = [_record(o[s], images[s], w, r, c) for s, w, r, c in good]
    bad = _record(o[1], images[1], (5, 4, 15, 20), (12, 12), (1, 1))
    if fault == "window_past_the_source":
        bad["win_y"], bad["win_h"] = 11, 20                              # 11 + 20 > 30
    elif fault == "rectangle_past_the_resized_image":
        bad["out_x"] = 6                                                 # 6 + 7 > 12
    elif fault == "offset_past_the_buffer":
        bad["src_offset"] = ragged.nbytes + 1
    else:
        bad["src_offset"] = o[1] + 1                                     # the last image would end one byte too late
    table = [records[0], bad, records[1]]
    got, status = _launch(dev, ragged, table, 9, 7)
    assert status == R.BAD_GEOMETRY
    assert not got[1].any()
    _assert_records(got[[0, 2]], images, [0, 1], records, 9, 7, fault)


@pytest.mark.gpu
def test_bad_scalar_arguments_and_an_empty_table(dev):
    from basd_amd import _lib
    images, ragged = _ragged()
    data = ragged.data.to(dev)
    out = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=dev)
    table = torch.zeros(64, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    for n, C, OH, OW, band in ((1, 2, 8, 8, 0), (1, 3, 0, 8, 0), (-1, 3, 8, 8, 0), (1, 3, 8, 8, 33), (1, 3, 8, 8, -1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            _lib.call("basd_resize_crop", data.data_ptr(), data.numel(), out.data_ptr(), n, C, OH, OW, table.data_ptr(),
                      status.data_ptr(), band, stream)
    with pytest.raises(RuntimeError, match="invalid argument"):           # the output inside the source buffer
        _lib.call("basd_resize_crop", data.data_ptr(), data.numel(), data.data_ptr() + 64, 1, 3, 8, 8, table.data_ptr(),
                  status.data_ptr(), 0, stream)
    _lib.call("basd_resize_crop", data.data_ptr(), data.numel(), out.data_ptr(), 0, 3, 8, 8, table.data_ptr(),
              status.data_ptr(), 0, stream)                               # n == 0: nothing is launched
    assert int(status.item()) == 0 and not out.any()


@pytest.mark.gpu
def test_device_equals_the_recorded_pillow_outputs(dev):
    g = np.load(GOLDEN, allow_pickle=False)
    cases = g["cases"].tolist()
    n_images = 1 + max(c[0] for c in cases)
    images = [g[f"image_{i}"] for i in range(n_images)]
    for k, (i, wx, wy, ww, wh, rw, rh) in enumerate(cases):               # one launch per case: the output size varies
        ragged = pack_images([images[i]])
        rec = _record(0, images[i], (wx, wy, ww, wh), (rw, rh), (0, 0))
        got, status = _launch(dev, ragged, [rec], rh, rw)
        assert status == 0 and np.array_equal(got[0], g[f"out_{k}"].transpose(2, 0, 1)), (k, cases[k])


@pytest.mark.gpu
def test_one_launch_and_one_copy_per_call(dev):
    """A steady-state call is one host-to-device copy (the record table) and one kernel launch: no memset, no
    workspace.  Counted with ``torch.profiler`` where it sees launches made through ctypes (the output says whether it
    does)."""
    from torch.profiler import ProfilerActivity, profile
    rng = np.random.RandomState(13)
    images = [structured(rng, rng.randint(40, 70), rng.randint(40, 70), 3) for _ in range(32)]
    ragged = pack_images(images).to(dev)
    rc = ResizeCrop(32, 0.875, device=dev)
    g = torch.Generator().manual_seed(8)
    draws = [draw_crop_params(ragged.sizes, generator=g) for _ in range(3)]
    for i in range(6):
        rc(ragged, draws[i % 3])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(21):
            views = rc(ragged, draws[i % 3])
        torch.cuda.synchronize()
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    copies = [e for e in device_events if "memcpy" in e.name.lower()]
    memsets = [e for e in device_events if "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in copies and e not in memsets]
    ours = [e for e in kernels if "resize_crop_kernel" in e.name]
    assert not memsets, sorted({e.name for e in memsets})
    if ours:
        print(f"[resize_crop] profiler: {len(kernels)} kernels ({len(ours)} resize_crop_kernel), {len(copies)} copies in "
              "21 calls")
        assert len(ours) == 21 and len(kernels) == 21, sorted({e.name for e in kernels})
        assert len(copies) == 21 and not any("dtoh" in e.name.lower().replace(" ", "") for e in copies), \
            sorted({e.name for e in copies})
    else:
        print("[resize_crop] the profiler does not see the ctypes launches here "
              f"({len(kernels)} device kernels, {len(copies)} copies seen by it)")
        assert not kernels and len(copies) in (0, 21)
    assert rc.status() == 0
    rec = make_records(ragged.sizes, 32, 0.875, draws[20 % 3])
    for view, part in (("clean", rec[:32]), ("augmented", rec[32:])):
        _assert_records(views[view].cpu().numpy(), images, list(range(32)), list(part), 32, 32, view)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inside the trainer and the validation loop
# ---------------------------------------------------------------------------------------------------------------------
def _reference_views(images, sizes, crops, S, ratio):
    rec = make_records(sizes, S, ratio, crops)
    B = len(images)
    both = [np.stack([_want(images, b, part[b], S, S) for b in range(B)]) for part in (rec[:B], rec[B:])]
    return both[0], both[1]


@pytest.mark.gpu
def test_trainer_prepares_both_views_and_steps(dev):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    images, ragged = _ragged()
    crops = draw_crop_params(ragged.sizes, generator=torch.Generator().manual_seed(2))
    student, teacher = _toy_models(dev)
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 16), mixup="fused",
                   image_stats=STATS, resize_crop=True)
    batch = {"images": ragged, "label": torch.arange(4) % 10, "crop_params": crops}
    clean, augmented = tr.prepare_views(batch)
    want_clean, want_augmented = _reference_views(images, ragged.sizes, crops, 16, 0.875)
    assert clean.dtype == torch.uint8 and clean.shape == (4, 3, 16, 16) and augmented.shape == (4, 3, 16, 16)
    assert np.array_equal(clean.cpu().numpy(), want_clean) and np.array_equal(augmented.cpu().numpy(), want_augmented)
    torch.manual_seed(77)
    assert torch.isfinite(tr.train_step(batch)["loss"])
    assert tr._resizer.status() == 0
    # without crops in the batch the trainer draws its own (global CPU generator); with the augmenter behind it
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 16), mixup="fused",
                   image_stats=STATS, resize_crop=True, trivial_augment=True)
    torch.manual_seed(5)
    assert torch.isfinite(tr.train_step({"images": ragged, "label": torch.arange(4) % 10})["loss"])
    assert tr._resizer.status() == 0 and tr._augmenter.status() == 0


@pytest.mark.gpu
def test_evaluate_model_on_ragged_batches(dev):
    """The same dict as on the uint8 batches the restatement makes of the same images."""
    from basd_amd.evaluation import evaluate_model
    rng = np.random.RandomState(14)
    student, _ = _toy_models(dev)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    ragged_loader, uint8_loader = [], []
    for n in (5, 7, 4):
        images = [structured(rng, rng.randint(12, 40), rng.randint(12, 40), 3) for _ in range(n)]
        label = torch.from_numpy(rng.randint(0, 10, n))
        ragged = pack_images(images)
        ragged_loader.append({"images": ragged, "label": label})
        rec = make_records(ragged.sizes, 16, 0.875, views=("clean",))
        clean = np.ascontiguousarray(np.stack([_want(images, b, rec[b], 16, 16) for b in range(n)]))     # dense NCHW
        uint8_loader.append({"pixel_values": torch.from_numpy(clean), "label": label})
    rc = ResizeCrop(16, 0.875, device=dev)
    kw = dict(num_classes=10, image_stats=(MEAN, STD))
    got = evaluate_model(student, ragged_loader, criterion, resize_crop=rc, **kw)
    want = evaluate_model(student, uint8_loader, criterion, **kw)
    assert got == want and np.isfinite(got["loss"]) and rc.status() == 0
    # a loader may mix both kinds of batches
    assert evaluate_model(student, ragged_loader[:2] + uint8_loader[2:], criterion, resize_crop=rc, **kw) == want
