"""The input work of batch k+1 on a side stream while batch k's step runs on the caller's.

Nothing of the input side of a step (the upload, ``JpegDecoder``, ``ResizeCrop``, ``TrivialAugment``, ``BatchMixer``, the
convert-only launch) depends on the step before it: the draws are made on the host, the record tables go up with
non-blocking copies, every launch takes the current stream and none of them waits for the device.  ``DevicePrefetcher``
is the orchestration: software pipelining in the caller's thread (no Python thread, no process), one private stream,
one event per prepared batch.  No kernels here.
"""
from __future__ import annotations

import ctypes
from collections import deque
from typing import Callable, Iterable, Iterator

import torch

__all__ = ["DevicePrefetcher"]

PRIORITIES = ("default", "lowest")


def _lowest_priority_stream(device: torch.device):
    """A non-blocking stream of the lowest priority the device has.  ``torch.cuda.Stream(priority=)`` only reaches from
    the default upwards, so the stream is made by the runtime and wrapped."""
    hip = ctypes.CDLL("libamdhip64.so")
    least, greatest = ctypes.c_int(0), ctypes.c_int(0)
    handle = ctypes.c_void_p()
    with torch.cuda.device(device):
        if hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) != 0:
            raise RuntimeError("hipDeviceGetStreamPriorityRange failed")
        if hip.hipStreamCreateWithPriority(ctypes.byref(handle), ctypes.c_uint(1), least) != 0:   # hipStreamNonBlocking
            raise RuntimeError("hipStreamCreateWithPriority failed")
    return torch.cuda.ExternalStream(handle.value, device=device)


def _record_stream(result, stream) -> None:
    """``record_stream(stream)`` on every device tensor of ``result`` (dicts, lists and tuples are walked)."""
    if isinstance(result, torch.Tensor):
        if result.is_cuda:
            result.record_stream(stream)
    elif isinstance(result, dict):
        for value in result.values():
            _record_stream(value, stream)
    elif isinstance(result, (list, tuple)):
        for value in result:
            _record_stream(value, stream)


class DevicePrefetcher:
    """``DevicePrefetcher(prepare, device=..., depth=1).iterate(loader)`` yields ``prepare(batch)`` for every batch of
    ``loader``, in order; before item k is yielded, ``prepare`` has been called for every item up to k + ``depth`` that
    the loader has, and the loader has been advanced no further than that.  ``prepare`` returns plain tensors and Python
    scalars, in dicts, lists and tuples.

    On a GPU ``device`` the object owns one stream (``.stream``), made once and used for every ``iterate``.  ``prepare``
    runs under ``torch.cuda.stream(self.stream)`` with an event recorded behind it; when the item is yielded the stream
    that is current then (the consumer's) waits for that event -- the host never does -- and every tensor of the item
    gets ``record_stream(consumer)``, so the caching allocator hands its memory out again only after the consumer's work
    that was queued while the tensor was alive, a backward that reads the images again included.  What ``prepare``
    allocates and drops itself lives and dies on the side stream and needs nothing.  ``depth=0`` is ``prepare(batch)`` on
    the current stream: no side stream is used, no event, no wait.  On a CPU ``device`` the scheduling is the same and
    there are no streams.

    The stages ``prepare`` calls keep device state that is safe only in stream order (``RecordTable.table``,
    ``JpegDecoder.workspace``).  When an ``iterate`` starts, the side stream waits for what the consumer's stream holds
    at that moment; when it ends -- the loader is exhausted, an exception leaves it, ``close()`` is called or the
    generator is dropped after a ``break`` -- the consumer's stream waits for the side stream.  So serial calls and
    prefetched iterations over the same stage objects are ordered against each other.  Between those two points the
    stage objects belong to this prefetcher alone: ONE SET OF STAGE OBJECTS BELONGS TO ONE PREFETCHER AT A TIME, and
    nothing else may call them while an iteration is open.

    An exception arrives where the serial loop would deliver it: one raised by ``prepare`` for item j, or by the loader
    when it is asked for item j, is raised (the same object) when item j is due, after items 0 .. j-1 have been yielded.
    The loader is not advanced past j, nothing stays pending, and the streams are joined as above.

    Memory: ``depth`` prepared batches more than the serial loop holds, plus the intermediates of the one being
    prepared.  ``priority``: ``"default"``, or ``"lowest"`` for a side stream of the lowest priority the device has.
    ``stream``: another prefetcher's ``.stream`` to work on instead of a new one (``Trainer.evaluate`` hands the
    training prefetcher's to the validation loop, which never runs at the same time).  ``depth=0`` makes no stream:
    ``.stream`` is ``None`` then, as on a CPU."""

    def __init__(self, prepare: Callable, *, device, depth: int = 1, priority: str = "default", stream=None) -> None:
        if isinstance(depth, bool) or not isinstance(depth, int) or depth < 0:
            raise ValueError(f"depth must be an int >= 0 (got {depth!r})")
        if priority not in PRIORITIES:
            raise ValueError(f"priority must be one of {', '.join(repr(p) for p in PRIORITIES)} (got {priority!r})")
        self.prepare = prepare
        self.device = torch.device(device)
        self.depth = depth
        self.priority = priority
        self.stream = stream
        if stream is None and depth > 0 and self.device.type == "cuda":
            self.stream = (_lowest_priority_stream(self.device) if priority == "lowest"
                           else torch.cuda.Stream(device=self.device))
        self._events: list = []

    def iterate(self, loader: Iterable) -> Iterator:
        if self.depth == 0:
            return self._serial(loader)
        return self._pipelined(loader)

    def _serial(self, loader: Iterable) -> Iterator:
        for batch in loader:
            yield self.prepare(batch)

    def _pipelined(self, loader: Iterable) -> Iterator:
        side = self.stream
        pending = deque()                # (result, event, None) or (None, None, exception), oldest first
        source = iter(loader)
        open_ = True                     # the loader may still have items, and nothing has raised
        slot = 0
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(self.device))
            while len(self._events) < self.depth + 1:
                self._events.append(torch.cuda.Event())
        try:
            while True:
                while open_ and len(pending) <= self.depth:
                    try:
                        batch = next(source)
                    except StopIteration:
                        open_ = False
                        break
                    except Exception as error:                  # delivered when this item is due
                        pending.append((None, None, error))
                        open_ = False
                        break
                    try:
                        if side is None:
                            pending.append((self.prepare(batch), None, None))
                        else:
                            with torch.cuda.stream(side):
                                result = self.prepare(batch)
                                event = self._events[slot]
                                event.record(side)
                            slot = (slot + 1) % len(self._events)
                            pending.append((result, event, None))
                    except Exception as error:
                        pending.append((None, None, error))
                        open_ = False
                    del batch
                if not pending:
                    return
                result, event, error = pending.popleft()
                if error is not None:
                    raise error
                if event is not None:
                    consumer = torch.cuda.current_stream(self.device)
                    consumer.wait_event(event)
                    _record_stream(result, consumer)
                yield result
                del result
        finally:
            pending.clear()
            if side is not None:
                torch.cuda.current_stream(self.device).wait_stream(side)
