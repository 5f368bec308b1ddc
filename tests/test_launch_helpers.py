"""The host plumbing the one-launch stages share (``basd_amd._launch``): the order in which the checks of an image batch
and of its ``out=`` fire, the byte-range overlap test, the per-sample columns, the one "no CPU fallback" error, the
device-ownership predicate, and -- on the GPU -- the record-table uploader's ring of pinned buffers."""
import numpy as np
import pytest
import torch

from basd_amd import _launch as L
from basd_amd.resize import CropParams
from basd_amd.trivial_augment import RECORD_DTYPE, AugmentParams

FLOATS = (torch.float32, torch.bfloat16)


def test_check_image_batch_reports_the_first_violation():
    """Rank, then density, then dtype, then channels: every tensor below also violates all the later conditions."""
    base = torch.zeros(4, 2, 8, 16, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"\(B, C, H, W\).*\(2, 8, 8\)"):
        L.check_image_batch(base[0, :, :, ::2], (torch.uint8,), channels=(1, 3))
    with pytest.raises(ValueError, match=r"dense NCHW.*\(4, 2, 8, 8\).*strides \(256, 128, 16, 2\)"):
        L.check_image_batch(base[:, :, :, ::2], (torch.uint8,), channels=(1, 3))
    with pytest.raises(ValueError, match="dense NCHW"):
        L.check_image_batch(base.to(memory_format=torch.channels_last), (torch.uint8,), channels=(1, 3))
    with pytest.raises(TypeError, match=r"images must be uint8 \(got torch.float16, shape \(4, 2, 8, 16\)\)"):
        L.check_image_batch(base, (torch.uint8,), channels=(1, 3))
    with pytest.raises(TypeError, match=r"images must be fp32 / bf16 / uint8 \(got torch.float16"):
        L.check_image_batch(base, L.DTYPE_CODES)
    with pytest.raises(ValueError, match=r"1 or 3 channels.*\(4, 2, 8, 16\)"):
        L.check_image_batch(base.to(torch.uint8), (torch.uint8,), channels=(1, 3))
    assert L.check_image_batch(base.to(torch.uint8), (torch.uint8,)) == (4, 2, 8, 16)
    assert L.check_image_batch(base[:, :1].to(torch.uint8), (torch.uint8,), channels=(1, 3)) == (4, 1, 8, 16)
    assert L.check_image_batch(torch.zeros(0, 3, 8, 8), L.DTYPE_CODES) == (0, 3, 8, 8)


def test_dense_ignores_the_strides_of_axes_of_size_one():
    x = torch.zeros(4, 1, 8, 8)
    assert L.dense(x) and L.dense(x.to(memory_format=torch.channels_last)) and L.dense(x.as_strided(x.shape, (64, 7, 8, 1)))
    assert not L.dense(torch.zeros(4, 3, 8, 8).to(memory_format=torch.channels_last))
    assert not L.dense(torch.zeros(4, 3, 8, 8)[::2]) and not L.dense(torch.zeros(8, 8).t())
    assert L.dense(torch.zeros(5)) and L.dense(torch.zeros(())) and L.dense(torch.zeros(0, 3))


def test_check_out_reports_the_first_violation():
    """Shape and density, then dtype, then device, then overlap.  The meta tensors have no address, so they also show
    that the device is looked at before any address is."""
    images = torch.zeros(2, 3, 4, 4)
    why = "row i needs the original row i - 1"
    with pytest.raises(ValueError, match=r"out must be a dense NCHW tensor of shape \(2, 3, 4, 4\) \(shape \(2, 3, 4, 5\)"):
        L.check_out(torch.zeros(2, 3, 4, 5, dtype=torch.float16, device="meta"), images, FLOATS, why)
    with pytest.raises(ValueError, match=r"out must be a dense NCHW.*strides \(96, 32, 8, 2\)"):
        L.check_out(torch.zeros(2, 3, 4, 8, dtype=torch.float16, device="meta")[..., ::2], images, FLOATS, why)
    with pytest.raises(TypeError, match=r"out must be fp32 / bf16 \(got torch.float16\)"):
        L.check_out(torch.zeros(2, 3, 4, 4, dtype=torch.float16, device="meta"), images, FLOATS, why)
    with pytest.raises(TypeError, match="out must be uint8"):
        L.check_out(torch.zeros(2, 3, 4, 4, device="meta"), images.to(torch.uint8), (torch.uint8,), why)
    with pytest.raises(ValueError, match="out lives on meta, images on cpu"):
        L.check_out(torch.zeros(2, 3, 4, 4, device="meta"), images, FLOATS, why)
    with pytest.raises(ValueError, match=r"out overlaps images \(shape \(2, 3, 4, 4\)\): row i needs the original row i - 1"):
        L.check_out(images, images, FLOATS, why)
    L.check_out(torch.zeros(2, 3, 4, 4, dtype=torch.bfloat16), images, FLOATS, why)


def _views(buffer, *specs):
    """``(byte offset, dtype)`` -> a (1, 1, 2, 2) view of the uint8 ``buffer`` starting at that byte."""
    return [buffer[at:at + 4 * dtype.itemsize].view(dtype).view(1, 1, 2, 2) for at, dtype in specs]


def test_check_out_catches_partial_overlaps_in_both_directions():
    buffer = torch.zeros(64, dtype=torch.uint8)
    why = "w"
    # uint8: 4-byte tensors; one shared byte on either side, none when they touch
    for src_at, out_at, overlaps in ((8, 11, True), (8, 5, True), (8, 12, False), (8, 4, False), (8, 8, True)):
        images, out = _views(buffer, (src_at, torch.uint8), (out_at, torch.uint8))
        if overlaps:
            with pytest.raises(ValueError, match="out overlaps images"):
                L.check_out(out, images, (torch.uint8,), why)
        else:
            L.check_out(out, images, (torch.uint8,), why)
    # fp32 source of 16 bytes at 16..32, bf16 out of 8 bytes.  Counted in elements the source would end at byte 20 and
    # the out at its start + 4: each overlapping case below overlaps only when element_size() is counted
    for out_at, overlaps in ((30, True), (32, False), (10, True), (8, False), (20, True)):
        images, out = _views(buffer, (16, torch.float32), (out_at, torch.bfloat16))
        if overlaps:
            with pytest.raises(ValueError, match="out overlaps images"):
                L.check_out(out, images, FLOATS, why)
        else:
            L.check_out(out, images, FLOATS, why)


def test_batch_columns_takes_lists_arrays_and_tensors_and_names_a_wrong_length():
    kinds = {"op": torch.int64, "bin": torch.int64, "sign": torch.bool, "flip": torch.bool}
    params = AugmentParams([1, 2, 3], np.array([4, 5, 6], dtype=np.int32), torch.tensor([1, 0, 1]), (True, False, False))
    cols = L.batch_columns(params, 3, kinds)
    assert cols == {"op": [1, 2, 3], "bin": [4, 5, 6], "sign": [True, False, True], "flip": [True, False, False]}
    assert list(cols) == list(kinds) and all(type(v) is bool for v in cols["sign"])
    assert L.batch_columns(params, 3, {"bin": torch.int64}) == {"bin": [4, 5, 6]}
    assert L.batch_columns(AugmentParams(torch.zeros(2, 0), [], [], []), 0, kinds) == dict.fromkeys(kinds, [])
    with pytest.raises(ValueError, match=r"AugmentParams\.op has 3 entries for a batch of 4"):
        L.batch_columns(params, 4, kinds)
    with pytest.raises(ValueError, match=r"AugmentParams\.sign has 2 entries for a batch of 3"):
        L.batch_columns(params._replace(sign=np.array([True, False])), 3, kinds)
    crops = CropParams(torch.tensor([0, 1]), [2, 3], np.array([[4], [5]]), torch.tensor([6]))
    with pytest.raises(ValueError, match=r"CropParams\.width has 1 entries for a batch of 2"):
        L.batch_columns(crops, 2, dict.fromkeys(CropParams._fields, torch.int64))
    assert L.batch_columns(crops, 2, {"height": torch.int64}) == {"height": [4, 5]}


def test_require_gpu_is_one_message_for_tensors_and_devices():
    plain = r"basd_amd kernels need CUDA/HIP tensors \(there is no CPU fallback\)"
    for thing in (torch.zeros(3), torch.device("cpu"), torch.zeros(3, device="meta")):
        with pytest.raises(RuntimeError, match=plain + "$"):
            L.require_gpu(thing)
    for thing in (torch.zeros(3), torch.device("cpu")):
        with pytest.raises(RuntimeError, match=plain + "; the 4 images live on cpu$"):
            L.require_gpu(thing, "the 4 images")
    L.require_gpu(torch.device("cuda"))
    L.require_gpu(torch.device("cuda:1"), "images of shape (4, 3, 8, 8)")


def test_lives_on_lets_an_owner_without_an_index_take_every_device_of_its_type():
    cuda, cuda0, cuda1, cpu = (torch.device(d) for d in ("cuda", "cuda:0", "cuda:1", "cpu"))
    assert L.lives_on(cuda, cuda0) and L.lives_on(cuda, cuda1) and L.lives_on(cuda0, cuda0) and L.lives_on(cpu, cpu)
    assert not L.lives_on(cuda0, cuda1) and not L.lives_on(cuda1, cuda0)
    assert not L.lives_on(cpu, cuda0) and not L.lives_on(cuda, cpu) and not L.lives_on(cuda0, cpu)


def test_dtype_codes_are_those_of_the_header():
    assert L.DTYPE_CODES == {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}


@pytest.mark.gpu
def test_record_table_keeps_every_staged_batch_until_its_copy_has_left():
    """Counts 3, 1, 5, 5, 2 through a ring of two: the table grows at the third call, the ring wraps twice and a
    smaller batch follows the growth.  Nothing waits between the calls, so a pinned buffer rewritten before its copy
    has left it, staged records dropped by the growth, or a slot index out of step with its event shows up as a clone
    of the device table that differs from what was staged for that call."""
    device = torch.device("cuda:0")
    table = L.RecordTable(RECORD_DTYPE, ring=2)
    assert table.status() == 0 and table.table is None
    staged, clones, capacity = [], [], []
    for call, count in enumerate((3, 1, 5, 5, 2)):
        records = table.stage(count, device)
        assert records.shape == (count,) and records.dtype == RECORD_DTYPE and records.flags.writeable
        records.view(np.uint8)[...] = (np.arange(count * 64) * 7 + 37 * (call + 1)) % 251
        staged.append(records.copy())
        assert table.upload() == table.table.data_ptr()
        clones.append(table.table[:count * 64].clone())
        capacity.append(table.table.numel() // 64)
    torch.cuda.synchronize()
    assert capacity == [3, 3, 5, 5, 5]
    for call, (want, got) in enumerate(zip(staged, clones)):
        assert np.array_equal(got.cpu().numpy().view(RECORD_DTYPE), want), f"call {call}"
    assert table.status() == 0 and table.status_ptr
