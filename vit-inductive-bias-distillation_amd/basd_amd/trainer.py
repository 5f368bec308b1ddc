"""A real distillation step around the loss path: the reference's ``Trainer`` inner loop
(``src/training/trainer.py:40-169``) on ROCm with stock torch models, so that the synthetic benchmark's loss call can
be seen inside an actual DeiT <- ResNet / ViT step.

What is mirrored: constructor arguments and attribute names of the reference ``Trainer`` (``basd_loss``, ``optimizer``,
``model``, ``criterion``, ``metrics_history``), ``_train_epoch`` / ``train`` and the per-batch order of operations
(student forward with token hooks, frozen teacher forward, loss, backward, optimizer step) and the checkpoint contents.
The models and the probing that produce ``teacher`` / ``student_info`` are the caller's (the reference's
``src/models/teacher.py``; ``tools/stock_models.py`` for the tests here).  What is fixed:

* the loss runs OUTSIDE autocast on fp32-accumulating kernels (the reference feeds bf16 into ``matrix_norm`` / ``eigvalsh``);
* ``BASDLoss.parameters()`` (the selector's temperatures) are reduced across ranks together with the student gradients
  in ONE flat RCCL all-reduce (``ddp.FlatGradBucket``): the reference leaves them out of ``accelerator.prepare``;
* loaders are sharded with ``DistributedSampler`` (``shard_loader``).

What is absent from the image and therefore replaced: ``accelerate`` (plain ``torch.distributed``),
``torchvision.transforms.v2.MixUp / CutMix`` (``mixup_cutmix`` with torch ops, or ``mixup="fused"``: ``basd_amd.augment``, one
HIP launch per batch that also converts and normalises uint8 batches).  The reference's optimizer, ``schedulefree.AdamWScheduleFree``,
is provided by ``basd_amd.optim`` (one HIP launch per step) and selected with ``optimizer="schedulefree"``; the default stays
``torch.optim.AdamW``.  Validation (``Trainer.evaluate``) is ``basd_amd.evaluation.evaluate_model``.  No kernels here: torch
module plumbing only.
"""
from __future__ import annotations

import math
from collections import defaultdict

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from . import capture
from .ddp import FlatGradBucket

__all__ = ["mixup_cutmix", "shard_loader", "Trainer"]


# ----------------------------------------------------------------------------------------------------------------
# data side
# ----------------------------------------------------------------------------------------------------------------
def mixup_cutmix(images: torch.Tensor, targets: torch.Tensor, num_classes: int, *, alpha: float = 1.0):
    """``RandomChoice([MixUp(alpha), CutMix(alpha)])`` of the reference (trainer.py:90-93) on device tensors:
    one Beta(alpha, alpha) draw per batch (global torch RNG), partner = the batch rolled by one, soft
    (B, num_classes) targets out."""
    u = torch.rand(3)
    lam = float(torch.distributions.Beta(alpha, alpha).sample())
    onehot = F.one_hot(targets, num_classes).to(torch.float32)
    if float(u[0]) < 0.5:                                           # MixUp
        mixed = lam * images + (1.0 - lam) * images.roll(1, 0)
    else:                                                           # CutMix: a box of area (1 - lam)
        H, W = images.shape[-2:]
        rh, rw = int(H * math.sqrt(1.0 - lam)), int(W * math.sqrt(1.0 - lam))
        cy, cx = int(float(u[1]) * H), int(float(u[2]) * W)
        y0, y1, x0, x1 = max(cy - rh // 2, 0), min(cy + rh // 2, H), max(cx - rw // 2, 0), min(cx + rw // 2, W)
        mixed = images.clone()
        mixed[..., y0:y1, x0:x1] = images.roll(1, 0)[..., y0:y1, x0:x1]
        lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
    return mixed, lam * onehot + (1.0 - lam) * onehot.roll(1, 0)


def shard_loader(dataset, batch_size: int, *, shuffle: bool = True, seed: int = 0, **kw):
    """A ``DataLoader`` over this rank's shard (the reference iterates the full loader on every rank)."""
    sampler = None
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, shuffle=shuffle, seed=seed, drop_last=True)
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, sampler=sampler,
                                       shuffle=shuffle and sampler is None, drop_last=True, **kw)


_TOKEN_FORMAT_WHY = ("a token-format teacher hands over every block, and with more than one teacher layer the mixing "
                     "weights depend on the student, so the mixed teacher's Gram is not a property of the image")


def _teacher_rows(filled, k: int):
    """Which batch positions the teacher sees in a step with ``teacher_partial=k``.  ``filled``: per batch position,
    whether the image's cache row has been stored (anything ``torch.as_tensor`` takes as bools).  The positions that are
    not filled, in batch order, then -- padding to the next multiple of ``k`` -- the first filled positions in batch
    order: the teacher then meets at most ``B / k`` batch shapes instead of ``B``.  An empty tensor: nothing is missing
    (a cached step).  ``None``: everything is missing or the padded count reaches ``B`` -- the ordinary uncached step."""
    filled = torch.as_tensor(filled, dtype=torch.bool).reshape(-1)
    B = filled.numel()
    missing = torch.nonzero(~filled).reshape(-1)
    if missing.numel() == 0:
        return missing
    padded = -(-missing.numel() // k) * k
    if padded >= B:
        return None
    return torch.cat([missing, torch.nonzero(filled).reshape(-1)[:padded - missing.numel()]])


# ----------------------------------------------------------------------------------------------------------------
# the trainer
# ----------------------------------------------------------------------------------------------------------------
class Trainer:
    """``Trainer(student_model, config, teacher, student_info=probe_model(student, img_size))`` -- ``teacher`` is the
    reference's ``TeacherModel`` record (``model``, ``embed_dim``, ``layer_paths``, ``attn_subpath``, ``has_cls_token``,
    ``feature_format``, ``heads_per_layer``), ``student_info`` what its ``probe_model`` returns.

    ``config`` needs ``.training.{label_smoothing, learning_rate, weight_decay}``, ``.basd.num_extraction_points`` and
    ``.model.num_classes`` (the fields the reference constructor reads, trainer.py:52-93).  ``loss_cls`` defaults to
    the HIP-backed ``basd_amd.losses.BASDLoss``; tests on CPU hand in the oracle's class.
    ``autocast_dtype``: dtype of the model forward passes (``torch.bfloat16`` as ``Accelerator(mixed_precision="bf16")``,
    or ``None``); the loss always sees fp32 logits and computes in fp32.
    ``optimizer``: ``"adamw"`` (``torch.optim.AdamW``) or ``"schedulefree"`` (``basd_amd.optim.AdamWScheduleFree``, the
    reference's choice, trainer.py:54-58; GPU only).  The schedule-free optimizer is kept in train mode except during
    validation and while a checkpoint is taken, which see the averaged (eval-mode) weights.
    ``mixup``: ``True`` (``mixup_cutmix``, torch ops), ``False``, or ``"fused"`` (``basd_amd.augment.BatchMixer``: mixing, soft
    targets and the uint8 conversion in one HIP launch; GPU only).  ``image_stats``: ``{"clean": (mean, std), "augmented":
    (mean, std)}`` per channel; with it (and ``mixup="fused"``) the loader may hand over uint8 batches: ``augmented`` is
    normalised inside the mixing launch, ``clean`` by a convert-only launch with the teacher's statistics.  A uint8 batch
    without it, or with another ``mixup``, raises ``TypeError``.  ``mix_dtype``: dtype the fused launches write
    (``torch.bfloat16``: what autocast would cast the images to anyway; default: fp32 for uint8, else the batch's own).
    ``attn_capture``: ``"torch"`` (the capture hooks of ``basd_amd.capture`` with torch ops) or ``"fused"`` (the teacher's
    attention importance from the output of each hooked block's own ``qkv`` Linear, one HIP launch per layer,
    ``basd_amd.attention``; GPU only).
    ``trivial_augment``: ``True`` runs the reference's ``RandomHorizontalFlip(flip_p) -> TrivialAugmentWide`` on the uint8
    ``augmented`` batch in one HIP launch (``basd_amd.trivial_augment``; GPU only) ahead of the mixing launch, so the loader
    only decodes and crops; it needs ``mixup="fused"`` and ``image_stats``.  The draws are made per step on the global CPU
    generator, or taken from the batch's optional ``"augment_params"`` entry (an ``AugmentParams``).
    ``resize_crop``: ``True`` makes both views on the device (``basd_amd.resize``; GPU only): the batch carries ``"images"``
    (a ``RaggedBatch`` of decoded images: the loader only decodes, ``collate_fn=collate_ragged``) and ``"label"`` instead of
    ``"clean"`` / ``"augmented"``, and one HIP launch resizes and crops the clean view (``Resize -> CenterCrop``) and the
    augmented one (``RandomResizedCrop``) to ``config.model.vit.img_size`` with ``config.data.eval_crop_ratio``; it needs
    ``mixup="fused"`` and ``image_stats``.  The crops are drawn per step on the global CPU generator, or taken from the
    batch's optional ``"crop_params"`` entry (a ``CropParams``).  ``prepare_views(batch)`` returns the two batches.
    ``resize_interpolation`` (it needs ``resize_crop``): ``"bilinear"`` (the default, the reference's), ``"bicubic"`` or
    ``"box"``, or a dict per view such as ``{"clean": "bicubic", "augmented": "bilinear"}`` (the teacher's view resampled
    the way a timm teacher was trained); still one launch.  ``evaluate`` resamples with the ``"clean"`` entry.
    ``jpeg_decode``: ``True`` (it needs ``resize_crop``) lets the batch's ``"images"`` be a ``JpegBatch`` of the files' bytes
    (the loader does not decode, ``collate_fn=collate_jpeg``): three launches of ``basd_amd.jpeg.JpegDecoder`` decode it
    into the ``RaggedBatch`` the resize launch takes; a ``RaggedBatch`` is taken as before.  ``"parallel"`` is ``True`` with
    ``JpegDecoder(entropy="parallel")``: the entropy stage decodes inside a segment with a workgroup's lanes instead of
    one lane per segment (the same bytes; what it gains is in DESIGN.md section 8).  ``False``: no decoder.  Whether
    progressive files are decoded on the device too is no option here: it is chosen where the batch is packed
    (``collate_fn=functools.partial(collate_jpeg, progressive=True)``), and the decoder follows the batch with one more
    launch.
    ``png_decode``: ``True`` (it needs ``resize_crop`` too) lets ``"images"`` be a ``PngBatch`` (``collate_fn=collate_png``),
    decoded by the two launches of ``basd_amd.png.PngDecoder`` ahead of the resize launch; ``False``: no decoder.
    ``max_grad_norm`` (``None`` or a finite number > 0) and ``skip_nonfinite``: global-norm clipping and the guard against
    inf / NaN gradients of ``AdamWScheduleFree``, decided on the device inside the optimizer's two launches (they need
    ``optimizer="schedulefree"``).  The norm is taken over the student's and the loss's gradients together, after the
    all-reduce and with the ``grad_scale`` the update gets, so every rank forms the same coefficient and the same verdict.
    With either, ``train_step`` also returns ``"grad_norm"`` and ``_train_epoch`` ``"grad_norm"`` (the mean over the steps
    that were not skipped, accumulated on the device) and ``"skipped_steps"`` (this epoch's count, one read at its end).
    A skipped step still advances the optimizer's ``k`` (see ``AdamWScheduleFree``).
    ``prefetch``: an int >= 0.  ``_train_epoch`` and ``evaluate`` run ``prepare_batch`` (the validation loop: its input
    half) for up to ``prefetch`` batches ahead of the one whose step runs, on one side stream
    (``basd_amd.prefetch.DevicePrefetcher``); 0, the default, is the serial loop.  It costs the memory of ``prefetch``
    prepared batches.  The draws stay inside ``prepare_batch``, in their order and the batches in theirs, so a seeded run
    prepares bit-identical batches with and without it; the one exception is a model that itself draws from the CPU
    generator in its forward (dropout in a CPU model): its draws fall between other batches' draws.  A model on the GPU
    draws from the device generator and is unaffected.  While an epoch or a validation runs, the stage objects of this
    trainer belong to its prefetcher: nothing else may call them.
    ``teacher_cache``: ``None``, a ``basd_amd.teacher_cache.TeacherCache`` or an int (a capacity in images -- the dataset's
    length; the cache is then built from the first batch's shapes).  GPU only, and only for a teacher whose
    ``extract_intermediates`` returns ONE layer (``feature_format != "token"``: every CNN teacher); any other raises
    ``ValueError`` here.  Batches must carry ``"index"``: the ``(B,)`` int64 dataset indices of their images (the dataset's
    transform returns ``{..., "index": i}``; ``default_collate``, ``collate_ragged``, ``collate_jpeg`` and ``collate_png``
    pass the key through); a batch without it raises ``KeyError``.  ``prepare_batch`` asks the cache on the host whether
    every image of the batch has been seen (``"teacher_cached"`` in what it returns); if so it makes no clean view and the
    step runs neither the teacher nor the teacher side of the loss (``BASDLoss.forward_cached``, which see for what such
    a step leaves out: the selector, hence ``subspace_ranks`` and ``d_grass_sq``); if not, the step is the usual one and
    its teacher side is stored behind the loss's forward.  Loss and gradients have the same bits either way; the draws
    and their order do not change (the clean view draws nothing).  The cache is valid for one teacher, one clean
    transform, one set of clean statistics and one autocast dtype, and never invalidates itself (``TeacherCache``);
    ``evaluate`` does not use it and checkpoints do not contain it.  With more than one rank each rank fills what its
    sampler shows it -- unless every rank runs ``fill_teacher_cache`` over the whole dataset once before ``train``: then
    every step of every rank is cached from the first epoch on, and nothing is exchanged between ranks.
    ``teacher_partial``: an int >= 0 (it needs ``teacher_cache``).  0, the default: a batch with any unseen image takes the
    uncached step.  ``k > 0``: ``prepare_batch`` finds the positions whose rows are not filled (on the host, from the
    bitmap) and pads them to the next multiple of ``k`` with the first filled positions (``_teacher_rows``; the padding
    keeps the teacher to ``B / k`` batch shapes, each new convolution shape costing a search in the vendor library).  If
    that reaches ``B`` the step is the uncached one.  Otherwise the teacher runs on those rows of the clean view only,
    ``BASDLoss.teacher_side(..., as_batch=B)`` makes their rows, the genuinely missing ones are stored (a stored row is
    never written again), and the step is the cached one (``load`` -> ``forward_cached``; like it, it does not run the
    selector).  The draws and their order do not change.  ``prepared`` then also carries ``teacher_rows``: the positions
    the teacher will see (empty for a cached step), or ``None`` for an uncached step.
    One caveat for both: a vendor convolution may pick another algorithm at another batch size, so a row made at batch
    ``m`` (a fill pass, a partly cached step) can differ in its last bits from the row an uncached step at batch ``B``
    would have stored.  That is the teacher's property, not the loss's: given equal teacher tokens the rows are equal
    bit for bit."""

    def __init__(self, student_model: nn.Module, config, teacher, *, student_info: dict, loss_cls=None,
                 autocast_dtype=None, mixup=True, optimizer: str = "adamw", image_stats=None, mix_dtype=None,
                 attn_capture: str = "torch", trivial_augment: bool = False, flip_p: float = 0.5,
                 resize_crop: bool = False, jpeg_decode=False, png_decode: bool = False, max_grad_norm=None,
                 skip_nonfinite: bool = False, prefetch: int = 0, resize_interpolation="bilinear",
                 check_factorisations: bool = False, teacher_cache=None, teacher_partial: int = 0) -> None:
        if isinstance(prefetch, bool) or not isinstance(prefetch, int) or prefetch < 0:
            raise ValueError(f"prefetch must be an int >= 0 (got {prefetch!r})")
        self._guarded = max_grad_norm is not None or bool(skip_nonfinite)
        self._skipped_seen = 0
        if teacher_cache is not None:
            from .teacher_cache import TeacherCache
            if not isinstance(teacher_cache, TeacherCache) and (
                    isinstance(teacher_cache, bool) or not isinstance(teacher_cache, int) or teacher_cache <= 0):
                raise ValueError(f"teacher_cache must be None, a TeacherCache or a capacity > 0 (got {teacher_cache!r})")
            if teacher.feature_format == "token":
                raise ValueError("teacher_cache needs a teacher with ONE extracted layer (feature_format != 'token'): "
                                 f"{_TOKEN_FORMAT_WHY}; got feature_format={teacher.feature_format!r}")
        self.teacher_cache = teacher_cache
        if isinstance(teacher_partial, bool) or not isinstance(teacher_partial, int) or teacher_partial < 0:
            raise ValueError(f"teacher_partial must be an int >= 0 (got {teacher_partial!r})")
        if teacher_partial and teacher_cache is None:
            raise ValueError("teacher_partial runs the teacher on the images a teacher_cache lacks: it needs "
                             f"teacher_cache; got teacher_cache=None and teacher_partial={teacher_partial!r}")
        self.teacher_partial = teacher_partial
        if self._guarded and optimizer != "schedulefree":
            raise ValueError("max_grad_norm and skip_nonfinite are part of AdamWScheduleFree's update: they need "
                             f"optimizer='schedulefree'; got optimizer={optimizer!r}")
        self.config = config
        self.device = next(student_model.parameters()).device
        self.criterion = nn.CrossEntropyLoss(label_smoothing=config.training.label_smoothing)
        self.model = student_model
        self._teacher = teacher
        self._student_layer_paths = student_info["layer_paths"]
        self._student_has_cls = student_info["has_cls_token"]
        if loss_cls is None:
            from .losses import BASDLoss as loss_cls
        self.basd_loss = loss_cls(
            base_criterion=self.criterion, student_dim=student_info["embed_dim"], teacher_dim=teacher.embed_dim,
            student_depth=student_info["depth"], num_student_tokens=student_info["num_tokens"], config=config.basd,
            teacher_has_cls_token=teacher.has_cls_token,
        ).to(self.device)
        if check_factorisations:
            # residual check of every tridiagonal factorisation of the selector (``TridiagCheckFailed``; the environment
            # switch BASD_TRIDIAG_CHECK=1 sets the same attribute when the loss is built)
            self.basd_loss.layer_selector.check_factorisations = True
        if optimizer == "adamw":
            self.optimizer = torch.optim.AdamW(student_model.parameters(), lr=config.training.learning_rate,
                                               weight_decay=config.training.weight_decay)
        elif optimizer == "schedulefree":
            from .optim import AdamWScheduleFree
            self.optimizer = AdamWScheduleFree(student_model.parameters(), lr=config.training.learning_rate,
                                               weight_decay=config.training.weight_decay,
                                               max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        else:
            raise ValueError(f"optimizer must be 'adamw' or 'schedulefree', not {optimizer!r}")
        self.optimizer.add_param_group({"params": list(self.basd_loss.parameters())})
        self._optimizer_mode(True)
        self.autocast_dtype = autocast_dtype
        if mixup not in (True, False, "fused"):
            raise ValueError(f"mixup must be True, False or 'fused', not {mixup!r}")
        self.mixup = mixup
        if attn_capture not in ("torch", "fused"):
            raise ValueError(f"attn_capture must be 'torch' or 'fused', not {attn_capture!r}")
        self.attn_capture = attn_capture
        self.image_stats = image_stats
        self.mix_dtype = mix_dtype
        self._mixer = self._clean_mixer = None
        if image_stats is not None and set(image_stats) != {"clean", "augmented"}:
            raise ValueError(f"image_stats needs the keys 'clean' and 'augmented' (got {sorted(image_stats)})")
        if mixup == "fused":
            from .augment import BatchMixer
            stats = image_stats or {"clean": (None, None), "augmented": (None, None)}
            classes = config.model.num_classes
            self._mixer = BatchMixer(classes, mean=stats["augmented"][0], std=stats["augmented"][1],
                                     out_dtype=mix_dtype, device=self.device)
            self._clean_mixer = BatchMixer(classes, mean=stats["clean"][0], std=stats["clean"][1],
                                           out_dtype=mix_dtype, device=self.device)
        elif mix_dtype is not None:
            raise ValueError("mix_dtype needs mixup='fused'")
        self._augmenter = None
        if trivial_augment:
            self._require_fused("trivial_augment needs", "it hands its uint8 batch to the fused launch")
            from .trivial_augment import TrivialAugment
            self._augmenter = TrivialAugment(device=self.device, flip_p=flip_p)
        self._resizer = None
        if resize_crop:
            self._require_fused("resize_crop needs", "it hands its uint8 batches to the fused launches")
            from .resize import ResizeCrop
            self._resizer = ResizeCrop(config.model.vit.img_size, config.data.eval_crop_ratio, device=self.device,
                                       interpolation=resize_interpolation)
        elif resize_interpolation != "bilinear":
            raise ValueError("resize_interpolation names the filter of the resize launch: it needs resize_crop=True; "
                             f"got resize_crop=False and resize_interpolation={resize_interpolation!r}")
        self._decoder = None
        if not (isinstance(jpeg_decode, bool) or jpeg_decode == "parallel"):
            raise ValueError(f"jpeg_decode must be True, False or 'parallel', not {jpeg_decode!r}")
        if jpeg_decode:
            if not resize_crop:
                raise ValueError("jpeg_decode needs resize_crop=True (the decoded images are a ragged batch, which the "
                                 "resize launch takes); got resize_crop=False")
            from .jpeg import JpegDecoder
            self._decoder = JpegDecoder(self.device, entropy="parallel" if jpeg_decode == "parallel" else "serial")
        self._png_decoder = None
        if not isinstance(png_decode, bool):
            raise ValueError(f"png_decode must be True or False, not {png_decode!r}")
        if png_decode:
            if not resize_crop:
                raise ValueError("png_decode needs resize_crop=True (the decoded images are a ragged batch, which the "
                                 "resize launch takes); got resize_crop=False")
            from .png import PngDecoder
            self._png_decoder = PngDecoder(self.device)
        from .prefetch import DevicePrefetcher
        self.prefetch = prefetch
        self._prefetcher = DevicePrefetcher(self.prepare_batch, device=self.device, depth=prefetch)
        self.best_val_acc = 0.0
        self.metrics_history = defaultdict(list)
        self._params = [p for p in student_model.parameters() if p.requires_grad]
        self._bucket = None
        self.reattached = 0
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # replicas start from rank 0's values
            for p in list(self.model.parameters()) + list(self.basd_loss.parameters()):
                dist.broadcast(p.data, src=0)
            for b in list(self.model.buffers()) + list(self.basd_loss.buffers()):
                dist.broadcast(b.data, src=0)
            # ONE flat buffer [student gradients | selector temperatures]; every parameter's ``.grad`` is a VIEW into it
            # (autograd accumulates in place, ``zero_grad(set_to_none=False)`` keeps the views), so the all-reduce needs
            # no per-parameter copy kernels (~300 small launches a step for DeiT-S when it packed and unpacked)
            self._bucket = FlatGradBucket(sum(p.numel() for p in self._params), list(self.basd_loss.parameters()),
                                          self.device)
            self._bucket.attach_grads(self._params)
            if optimizer == "schedulefree":
                # the gradients stay where they are: the update zeroes them in its own pass (no separate zero_grad)
                self.optimizer.zero_grad_in_step = True

    def _require_fused(self, what: str, why: str, error=ValueError, **batches) -> None:
        """Whatever hands uint8 batches on needs the fused launch (``mixup="fused"``) and ``image_stats`` to convert them."""
        if self.mixup != "fused" or self.image_stats is None:
            got = "".join(f", {name} {t.dtype} {tuple(t.shape)}" for name, t in batches.items())
            raise error(f"{what} mixup='fused' and image_stats ({why}); got mixup={self.mixup!r}, image_stats="
                        f"{'given' if self.image_stats is not None else None}{got}")

    # -- one batch: the body of the reference's _train_epoch loop (trainer.py:133-164)
    def prepare_views(self, batch: dict, *, want_clean: bool = True, clean_rows=None):
        """``(clean, augmented)`` of a batch on the device.  With ``resize_crop`` both are made from the batch's
        ``"images"`` by one launch (uint8, ``(B, C, S, S)``); without, they are the batch's own entries.
        ``want_clean=False`` (the teacher side of every image is cached): ``clean`` is ``None``, not uploaded or made.
        ``clean_rows`` (a host int64 vector, ``teacher_partial``): ``clean`` holds those batch positions only -- a host
        tensor is selected on the host, ahead of the upload."""
        dev = self.device
        if self._resizer is None:
            clean = self._select_rows(batch["clean"], clean_rows).to(dev, non_blocking=True) if want_clean else None
            return clean, batch["augmented"].to(dev, non_blocking=True)
        images = self._decoded_images(batch)
        if not want_clean:
            views = self._resizer(images.to(dev, non_blocking=True), batch.get("crop_params"), views=("augmented",))
            return None, views["augmented"]
        views = self._resizer(images.to(dev, non_blocking=True), batch.get("crop_params"))
        return self._select_rows(views["clean"], clean_rows), views["augmented"]

    @staticmethod
    def _select_rows(images: torch.Tensor, rows) -> torch.Tensor:
        if rows is None:
            return images
        return images[rows.to(images.device, non_blocking=True) if images.is_cuda else rows]

    def _decoded_images(self, batch: dict):
        """The batch's ``"images"`` as the ``RaggedBatch`` the resize launch takes, decoded on the device where the
        trainer has the decoder for what the loader handed over."""
        dev = self.device
        from .resize import RaggedBatch
        images = batch.get("images")
        if self._decoder is not None:
            from .jpeg import JpegBatch
            if isinstance(images, JpegBatch):
                images = self._decoder(images.to(dev, non_blocking=True))
        if self._png_decoder is not None:
            from .png import PngBatch
            if isinstance(images, PngBatch):
                images = self._png_decoder(images.to(dev, non_blocking=True))
        if not isinstance(images, RaggedBatch):
            raise TypeError("resize_crop works on decoded images (the loader decodes, nothing else): the batch needs "
                            f"'images', a RaggedBatch (collate_fn=collate_ragged); got {sorted(batch)}")
        return images

    def _batch_index(self, batch: dict) -> torch.Tensor:
        """The batch's ``"index"`` as a host int64 vector (``teacher_cache``)."""
        if "index" not in batch:
            raise KeyError("'index': teacher_cache needs the dataset indices of the batch's images, a (B,) int64 tensor "
                           f"under 'index' (the dataset's transform returns {{..., 'index': i}}); got {sorted(batch)}")
        return torch.as_tensor(batch["index"]).to("cpu", torch.int64).reshape(-1)

    def prepare_batch(self, batch: dict) -> dict:
        """The input half of a step, everything ahead of the model forwards: the transfer, the views, the augmentation
        and the mixing, with the checks that raise ``TypeError``.  Returns ``clean``, ``augmented``, ``targets`` and
        ``mixed_targets`` on the device.  It draws crop, augment and mix, in that order, on the global CPU generator and
        touches neither model, so it may run ahead of the step before it (``prefetch``).  With ``teacher_cache`` also
        ``index`` (on the device), ``index_host`` and ``teacher_cached``, decided here on the host from the rows whose
        store has been queued; when it is true there is no ``clean``.  With ``teacher_partial`` also ``teacher_rows``
        (see the class): where it names rows, ``clean`` holds those batch positions only."""
        dev = self.device
        index = None
        cached = False
        rows = None
        if self.teacher_cache is not None:
            index = self._batch_index(batch)
            cached = not isinstance(self.teacher_cache, int) and self.teacher_cache.has(index)
            if self.teacher_partial and not isinstance(self.teacher_cache, int):
                rows = _teacher_rows(self.teacher_cache.filled(index), self.teacher_partial)
        partial = rows is not None and rows.numel() > 0
        clean, student_imgs = self.prepare_views(batch, want_clean=not cached, clean_rows=rows if partial else None)
        targets = batch["label"].to(dev, non_blocking=True)
        mixed_targets = targets
        if (clean is not None and clean.dtype == torch.uint8) or student_imgs.dtype == torch.uint8:
            self._require_fused("uint8 batches need", "the conversion and the normalisation are part of the fused launch",
                                TypeError, clean=clean, augmented=student_imgs)
        if self._augmenter is not None:
            if student_imgs.dtype != torch.uint8:
                raise TypeError("trivial_augment works on uint8 batches (the loader decodes and crops, nothing else); got "
                                f"augmented {student_imgs.dtype} {tuple(student_imgs.shape)}")
            student_imgs = self._augmenter(student_imgs, batch.get("augment_params"))
        if self.mixup == "fused":
            from .augment import MixParams
            if clean is not None and clean.dtype == torch.uint8:
                clean, _ = self._clean_mixer(clean, None, MixParams("none"))
            student_imgs, mixed_targets = self._mixer(student_imgs, targets)
        elif self.mixup:
            student_imgs, mixed_targets = mixup_cutmix(student_imgs, targets, self.config.model.num_classes)
        prepared = {"augmented": student_imgs, "targets": targets, "mixed_targets": mixed_targets}
        if clean is not None:
            prepared["clean"] = clean
        if index is not None:
            if index.numel() != targets.shape[0]:
                raise ValueError(f"'index' has {index.numel()} entries for a batch of {targets.shape[0]}")
            prepared.update(index=index.to(dev, non_blocking=True), index_host=index, teacher_cached=cached)
            if self.teacher_partial:
                prepared["teacher_rows"] = rows
        return prepared

    def step_prepared(self, prepared: dict) -> dict:
        """The rest of the step on what ``prepare_batch`` returned: both forwards, the loss, the backward, the update."""
        dev = self.device
        student_imgs = prepared["augmented"]
        targets, mixed_targets = prepared["targets"], prepared["mixed_targets"]
        cached = prepared.get("teacher_cached", False)
        rows = prepared.get("teacher_rows")
        partial = not cached and rows is not None and rows.numel() > 0
        ac = torch.autocast(dev.type, dtype=self.autocast_dtype, enabled=self.autocast_dtype is not None)
        with ac:
            logits, s_tokens = capture._extract_student(self.model, student_imgs, self.basd_loss.token_layers,
                                                        layer_paths=self._student_layer_paths,
                                                        has_cls_token=self._student_has_cls)
            if not cached:
                teacher_tokens, teacher_attns = capture.extract_intermediates(self._teacher, prepared["clean"],
                                                                              attn=self.attn_capture)
        # the loss is computed outside autocast: fp32 logits, tokens consumed in their own dtype (fp32 internal)
        if partial:
            # the teacher saw ``rows`` only: their teacher side as the uncached step at this batch size would make it,
            # the missing ones of them stored, and the step goes on as the cached one
            self._store_missing_rows(prepared, self.basd_loss.teacher_side(teacher_tokens, teacher_attns,
                                                                           as_batch=targets.shape[0]))
        if cached or partial:
            # the gather is queued HERE, on the step's stream, not where the batch was prepared: it reads rows that
            # stores on this stream wrote
            side = self.teacher_cache.load(prepared["index_host"], device_index=prepared["index"])
            loss = self.basd_loss.forward_cached(logits.float(), mixed_targets, s_tokens, side)
        else:
            loss = self.basd_loss(logits.float(), mixed_targets, s_tokens, teacher_tokens, teacher_attns)
            if self.teacher_cache is not None:
                # right behind the forward, ahead of the backward: the teacher side is a view of the call's scratch
                self._store_teacher_side(prepared)
        loss.backward()
        if getattr(self.optimizer, "zero_grad_in_step", False):
            # schedule-free AdamW over the flat bucket: 1 / world (where the backend only sums) and the zeroing of the
            # gradients are part of the one update launch
            self.optimizer.step(grad_scale=self._all_reduce_gradients(divide=False))
        else:
            self._all_reduce_gradients()
            self.optimizer.step()
            self.optimizer.zero_grad(set_to_none=False)
        out = {"loss": loss.detach(), "correct": logits.detach().argmax(1).eq(targets).sum(), "n": targets.size(0)}
        if self._guarded:
            out["grad_norm"] = self.optimizer.last_grad_norm()
        return out

    def _store_teacher_side(self, prepared: dict) -> None:
        side = self.basd_loss.last_teacher_side()
        if isinstance(self.teacher_cache, int):
            from .teacher_cache import TeacherCache
            self.teacher_cache = TeacherCache(self.teacher_cache, side.g.shape[-1], side.omega.shape[-1], self.device)
        self.teacher_cache.store(prepared["index_host"], side, device_index=prepared["index"])

    def _store_missing_rows(self, prepared: dict, side) -> None:
        """Of the rows ``side`` holds (batch positions ``teacher_rows``) those whose cache row is still not filled NOW:
        the padding is dropped, and so is a row that a step between this batch's preparation and now has stored
        (``prefetch``), so a stored row never changes after its first store."""
        index = prepared["index_host"][prepared["teacher_rows"]]
        need = ~self.teacher_cache.filled(index)
        count = int(need.sum())
        if count == 0:
            return
        if bool(need[:count].all()):            # the missing rows come first (``_teacher_rows``): views, no launch
            side = tuple(t[:count] for t in side)
        else:
            keep = torch.nonzero(need).reshape(-1).to(self.device, non_blocking=True)
            side = tuple(t.index_select(0, keep) for t in side)
        self.teacher_cache.store(index[need], side)

    def fill_teacher_cache(self, loader, *, as_batch: int) -> int:
        """Run the frozen teacher over ``loader`` once, without the student, and store every image's teacher side in
        ``teacher_cache``; returns the number of images stored.  Afterwards every step whose images the loader showed is
        a cached one, from the first epoch on and on every rank that filled: call it once per rank over the whole dataset
        before ``train``.

        The loader's batches carry ``"index"`` (``KeyError`` without) and the source of the clean view: ``"clean"``, or
        ``"images"`` with ``resize_crop`` / ``jpeg_decode`` / ``png_decode``; labels and ``"augmented"`` are not touched.
        Per batch: the clean view alone (``views=("clean",)`` of the resize launch), the teacher under the step's
        autocast, ``BASDLoss.teacher_side(..., as_batch=as_batch)``, ``TeacherCache.store``.  No generator is drawn from;
        no student forward, no selector, no optimizer.  ``as_batch``: the batch size of the TRAINING steps (it fixes the
        fold order of the split teacher Gram); the loader's own batch size may differ, and the last batch may be short.
        An int ``teacher_cache`` is built from the first batch's shapes, as in the step.  ``ValueError`` for a
        token-format teacher or without ``teacher_cache``; on a CPU device the package's "no CPU fallback"
        ``RuntimeError``.  It runs serially on the current stream and uses the trainer's stage objects: it must not be
        called while an epoch or a validation runs.  The caveat of ``teacher_partial`` (see the class) holds: a vendor
        convolution may choose by batch size, so fill at the training batch size where the last bits matter."""
        if self._teacher.feature_format == "token":
            raise ValueError("fill_teacher_cache needs a teacher with ONE extracted layer (feature_format != 'token'): "
                             f"{_TOKEN_FORMAT_WHY}; got feature_format={self._teacher.feature_format!r}")
        if self.teacher_cache is None:
            raise ValueError("fill_teacher_cache fills the trainer's teacher_cache; got teacher_cache=None")
        if isinstance(as_batch, bool) or not isinstance(as_batch, int) or as_batch <= 0:
            raise ValueError(f"as_batch must be an int > 0, the batch size of the training steps (got {as_batch!r})")
        from ._launch import require_gpu
        dev = self.device
        ac = torch.autocast(dev.type, dtype=self.autocast_dtype, enabled=self.autocast_dtype is not None)
        stored = 0
        for batch in loader:
            index = self._batch_index(batch)
            require_gpu(dev, "the teacher cache's rows")
            if self._resizer is None:
                clean = batch["clean"].to(dev, non_blocking=True)
            else:
                images = self._decoded_images(batch).to(dev, non_blocking=True)
                clean = self._resizer(images, None, views=("clean",))["clean"]
            if index.numel() != clean.shape[0]:
                raise ValueError(f"'index' has {index.numel()} entries for a batch of {clean.shape[0]}")
            if clean.dtype == torch.uint8:
                self._require_fused("uint8 batches need", "the conversion and the normalisation are part of the fused "
                                    "launch", TypeError, clean=clean)
                from .augment import MixParams
                clean, _ = self._clean_mixer(clean, None, MixParams("none"))
            with ac, torch.no_grad():
                teacher_tokens, teacher_attns = capture.extract_intermediates(self._teacher, clean,
                                                                              attn=self.attn_capture)
            side = self.basd_loss.teacher_side(teacher_tokens, teacher_attns, as_batch=as_batch)
            if isinstance(self.teacher_cache, int):
                from .teacher_cache import TeacherCache
                self.teacher_cache = TeacherCache(self.teacher_cache, side.g.shape[-1], side.omega.shape[-1], dev)
            self.teacher_cache.store(index, side)
            stored += index.numel()
        return stored

    def train_step(self, batch: dict) -> dict:
        return self.step_prepared(self.prepare_batch(batch))

    def _optimizer_mode(self, train: bool) -> bool:
        """``optimizer.train()`` / ``optimizer.eval()`` where the optimizer has them (reference trainer.py:180,184);
        returns whether it has."""
        switch = getattr(self.optimizer, "train" if train else "eval", None)
        if switch is None:
            return False
        switch()
        return True

    def _all_reduce_gradients(self, divide: bool = True) -> float:
        """The step's one exchange (reference trainer.py:157 leaves it to ``accelerator.backward``): mean over ranks of
        the flat gradient buffer, queued on the communicator's stream and joined by the current stream before the
        optimizer reads the gradients -- which ARE the buffer (``attach_grads``), so nothing is packed or unpacked.
        Returns the factor the caller still has to apply to the gradients: 1, or ``1 / world`` with ``divide=False``
        on a backend that only sums."""
        if self._bucket is None:
            return 1.0
        # a gradient autograd replaced (or never produced) goes back into the buffer; 0 in the steady state
        self.reattached += self._bucket.reattach_missing()
        self._bucket.all_reduce_mean(async_op=True)
        owed = self._bucket.wait(divide=divide)
        return 1.0 / dist.get_world_size() if owed else 1.0

    def _train_epoch(self, train_loader, epoch: int = 0) -> dict:
        # a sharded loader draws a different permutation every epoch only if it is told the epoch (every rank the same one)
        sampler = getattr(train_loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        total_loss = torch.zeros((), device=self.device)
        correct = torch.zeros((), device=self.device, dtype=torch.long)
        total = 0
        if self._guarded:
            norm_sum = torch.zeros((), device=self.device)
            norm_steps = torch.zeros((), device=self.device)
        self.model.train()
        self._optimizer_mode(True)
        for prepared in self._prefetcher.iterate(train_loader):
            out = self.step_prepared(prepared)
            total_loss += out["loss"] * out["n"]
            correct += out["correct"]
            total += out["n"]
            if self._guarded:
                kept = self.optimizer.last_step_skipped() == 0
                norm_sum += torch.where(kept, out["grad_norm"], 0.0)
                norm_steps += kept
        self._finish_loss()
        metrics = {"train_loss": (total_loss / total).item(), "train_acc": 100.0 * (correct / total).item()}
        if self._guarded:
            skipped = self.optimizer.skipped_steps()                # the epoch's one read of the verdict
            metrics["grad_norm"] = (norm_sum / norm_steps).item()  # NaN when every step was skipped
            metrics["skipped_steps"], self._skipped_seen = skipped - self._skipped_seen, skipped
        return metrics

    def _finish_loss(self) -> None:
        """Complete what the loss may have deferred past its last call (a rank read-back in ``sync_ranks = False`` mode,
        with the error it carries): nothing of a step may be left pending at an epoch end or in a checkpoint."""
        sel = getattr(self.basd_loss, "layer_selector", None)
        if sel is not None and hasattr(sel, "finish_pending"):
            sel.finish_pending()

    def evaluate(self, model: nn.Module, val_loader) -> dict:
        """The reference's validation call (trainer.py:185-189): ``evaluate_model`` with the trainer's smoothed
        criterion -- one HIP launch per batch, one read-back per epoch; over the ranks' shards when a process group
        with more than one rank exists.  With ``image_stats`` the validation loader may hand over uint8
        ``pixel_values``: they are normalised on the device with the ``augmented`` statistics -- the dataset's own, which
        the reference's validation loader uses too (datasets.py:168-175) -- and written as ``mix_dtype``.  With
        ``resize_crop`` it may hand over ``images`` (a ``RaggedBatch``) instead: they are resized and cropped first (with
        ``jpeg_decode`` a ``JpegBatch``, with ``png_decode`` a ``PngBatch``: decoded, then resized and cropped).  Has the
        signature ``train(..., evaluate=)`` expects: ``trainer.train(train_loader, val_loader,
        evaluate=trainer.evaluate)``."""
        from .evaluation import evaluate_model
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        stats = None if self.image_stats is None else self.image_stats["augmented"]
        return evaluate_model(model, val_loader, self.criterion, num_classes=self.config.model.num_classes,
                              distributed=distributed, image_stats=stats, input_dtype=self.mix_dtype,
                              resize_crop=self._resizer, jpeg_decode=self._decoder, png_decode=self._png_decoder,
                              prefetch=self.prefetch,
                              prefetch_stream=self._prefetcher.stream)

    def train(self, train_loader, val_loader=None, start_epoch: int = 0, *, evaluate=None, on_epoch_end=None) -> dict:
        """The reference's epoch loop (trainer.py:171-216): ``_train_epoch``, validation, ``metrics_history``,
        ``best_val_acc``.  Validation is the caller's (``evaluate(model, val_loader) -> {"val_acc": ...}``): pass
        ``evaluate=trainer.evaluate`` for the reference's ``evaluate_model``; ``on_epoch_end(trainer, epoch, improved)``
        is where a caller saves checkpoints."""
        for epoch in range(start_epoch, self.config.training.num_epochs):
            metrics = self._train_epoch(train_loader, epoch)
            if evaluate is not None and val_loader is not None:
                self.model.eval()
                switched = self._optimizer_mode(False)          # validation sees the averaged weights
                metrics.update(evaluate(self.model, val_loader))
                if switched:
                    self._optimizer_mode(True)
            for key, value in metrics.items():
                self.metrics_history[key].append(value)
            improved = metrics.get("val_acc", float("-inf")) > self.best_val_acc
            if improved:
                self.best_val_acc = metrics["val_acc"]
            if on_epoch_end is not None:
                on_epoch_end(self, epoch, improved)
        return self.metrics_history

    # -- checkpoints: what accelerator.save_state + custom_state.pth hold in the reference (trainer.py:94-123)
    def state_dict(self, epoch: int) -> dict:
        self._finish_loss()
        # a schedule-free optimizer is saved in eval mode (the reference saves after ``optimizer.eval()``): the weights
        # are copied out, because they move back to the train-mode sequence before this returns
        switched = self._optimizer_mode(False)
        model, loss = self.model.state_dict(), self.basd_loss.state_dict()
        if switched:
            model = {k: v.clone() for k, v in model.items()}
            loss = {k: v.clone() for k, v in loss.items()}
        state = {"model": model, "optimizer": self.optimizer.state_dict(), "basd_loss": loss, "epoch": epoch,
                 "best_val_acc": self.best_val_acc, "metrics_history": dict(self.metrics_history)}
        if switched:
            self._optimizer_mode(True)
        return state

    def save_checkpoint(self, path: str, epoch: int) -> None:
        torch.save(self.state_dict(epoch), path)

    def load_checkpoint(self, path: str) -> int:
        state = torch.load(path, map_location=self.device, weights_only=True)
        self.model.load_state_dict(state["model"])
        self.optimizer.load_state_dict(state["optimizer"])
        self.basd_loss.load_state_dict(state["basd_loss"])
        self._optimizer_mode(True)
        self.best_val_acc = state["best_val_acc"]
        self.metrics_history = defaultdict(list, state.get("metrics_history", {}))
        return state["epoch"] + 1
