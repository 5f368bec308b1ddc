"""MI355X-native BASD loss path (Grassmannian layer selector + attention-weighted
Procrustes loss) behind the reference's ``src.losses`` API.

Sub-modules:
  ``_lib``     ctypes binding of the C-ABI in ``include/basd_hip.h`` (raises if the
               HIP library is missing -- there is no CPU fallback)
  ``ops``      torch.autograd Functions / host orchestration over the C-ABI
  ``losses``   ``BASDLoss`` / ``GrassmannianLayerSelector`` / free functions
  ``optim``    ``AdamWScheduleFree``: the reference trainer's optimizer, one launch per step
  ``evaluation``  ``evaluate_model`` / ``EvalAccumulator``: top-1 / top-5 and loss, one launch per validation batch
  ``augment``  ``BatchMixer`` / ``draw_mix_params``: MixUp / CutMix, soft targets and the uint8 conversion, one launch
               per batch
  ``attention``  ``attn_importance``: a teacher's attention importance (CLS row / mean over queries) from the output of
               its own ``qkv`` projection, one launch per layer
  ``stats``    ``channel_stats`` / ``ChannelStats``: exact per-channel mean and std of uint8 images, one launch per chunk
  ``trivial_augment``  ``TrivialAugment`` / ``draw_augment_params``: the flip and TrivialAugmentWide of uint8 batches, one
               launch per batch
  ``resize``   ``ResizeCrop`` / ``pack_images`` / ``collate_ragged`` / ``draw_crop_params``: Pillow-exact crops and resizes
               of ragged batches of decoded uint8 images, both views in one launch
  ``jpeg``     ``JpegDecoder`` / ``pack_jpegs`` / ``collate_jpeg`` / ``parse_jpeg``: Pillow-exact baseline JPEG decoding of a
               batch of files' bytes into a ragged batch, three launches per batch (progressive files too, opt-in
               with ``progressive=True`` where the batch is packed: one more launch)
  ``png``      ``PngDecoder`` / ``pack_pngs`` / ``collate_png`` / ``parse_png``: Pillow-exact 8-bit PNG decoding of a batch of
               files' bytes into a ragged batch, two launches per batch
  ``prefetch``  ``DevicePrefetcher``: the input work of the next batch on a side stream while the step runs
  ``teacher_cache``  ``TeacherCache``: the teacher side of a single-layer teacher per dataset image on the device, one
               scatter and one gather launch (``BASDLoss.forward_cached``, ``Trainer(teacher_cache=...)``)
  ``_launch``  what those one-launch stages share on the host: argument checks, dtype codes, the record-table uploader
  ``synth``    seeded synthetic feature stacks (benchmark + tests)
"""
__version__ = "0.1.0"

from .attention import attn_importance  # noqa: E402
from .trivial_augment import AugmentParams, TrivialAugment, draw_augment_params  # noqa: E402
from .resize import (CropParams, RaggedBatch, ResizeCrop, collate_ragged, draw_crop_params,  # noqa: E402
                     eval_window, pack_images)
from .jpeg import (JpegBatch, JpegDecoder, UnsupportedJpeg, collate_jpeg, decode_reference,  # noqa: E402
                   pack_jpegs, parse_jpeg)
from .png import PngBatch, PngDecoder, UnsupportedPng, collate_png, pack_pngs, parse_png  # noqa: E402
from .prefetch import DevicePrefetcher  # noqa: E402

__all__ = ["attn_importance", "AugmentParams", "TrivialAugment", "draw_augment_params", "CropParams", "RaggedBatch",
           "ResizeCrop", "collate_ragged", "draw_crop_params", "eval_window", "pack_images", "JpegBatch", "JpegDecoder",
           "UnsupportedJpeg", "collate_jpeg", "decode_reference", "pack_jpegs", "parse_jpeg", "PngBatch",
           "PngDecoder", "UnsupportedPng", "collate_png", "pack_pngs", "parse_png", "DevicePrefetcher"]
