"""The per-stream device buffers of the reasoners and the stream pools: packed weight images and workspaces.

Forwards of one module may be in flight on several HIP streams at once (serving.py keeps two passes in flight, the stream
pools run on the caller's stream).  So every stream gets its own packed image and its own workspaces: a re-pack after a
weight update must not rewrite an image that another stream's earlier launches are still reading, and two streams must not
share a history.  A pack and the launches that read its image are always ordered by their own stream.

Both caches drop the least recently used entry past `limit` at once, although launches on its stream may still be reading
it: the key holds the stream the buffer was allocated on, and the caching allocator only hands a block back to that stream,
so whatever reuses it runs behind them.  (A hipGraph is different: it must be destroyed by hand, behind a sync.)

Sizes are given as (size query of the library, its arguments) and asked only when a buffer is made; a size of 0 is the
library refusing the shape, raised with its message.  Host code only: any torch device works.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib


def device_index(device: torch.device):
    """the device's index; the current device's for a ROCm device without one (None for the CPU)"""
    if device.index is None and device.type == "cuda":
        return torch.cuda.current_device()
    return device.index


def weights_key(ws, device: torch.device) -> tuple:
    """what an image is packed from: (data_ptr, _version) of every weight, and the device"""
    return tuple((w.data_ptr(), w._version) for w in ws) + (device_index(device),)


def check_weights(ws, device: torch.device, who: str) -> None:
    for w in ws:
        if w.device != device or w.dtype != torch.float32 or not w.is_contiguous():
            raise RuntimeError(f"{who} parameters must be contiguous fp32 on the input's device "
                               "(call model.to(device) first)")


def _size(nbytes) -> int:
    query, *args = nbytes
    n = int(query(*args))
    if n == 0:
        _lib.check(-2, query.__name__)
    return n


def _new(size: int, dtype, device: torch.device, zero: bool = False) -> torch.Tensor:
    return (torch.zeros if zero else torch.empty)(size, dtype=dtype, device=device)


class PackedImages:
    """One packed weight image per stream, for at most `limit` streams."""

    def __init__(self, limit: int, who: str):
        self.limit, self.who = limit, who
        self._images: OrderedDict = OrderedDict()      # stream -> (weights key, image), least recently used first

    def get(self, stream: int, ws, device: torch.device, nbytes, pack, zero: bool = False) -> torch.Tensor:
        """the fp32 image of the weights `ws` for launches on `stream`.  pack(image, nbytes) runs only when a weight changed
        since this stream's last pack, into the same buffer while the device is the same; zero: a new buffer starts zeroed"""
        key = weights_key(ws, device)
        entry = self._images.get(stream)
        if entry is not None and entry[0] == key:
            self._images.move_to_end(stream)
            return entry[1]
        check_weights(ws, device, self.who)
        size = _size(nbytes)
        if entry is not None and entry[1].device == device:
            buf = entry[1]
        else:
            self._images.pop(stream, None)
            while len(self._images) >= self.limit:
                self._images.popitem(last=False)
            buf = _new(size // 4, torch.float32, device, zero)
        pack(buf, size)
        self._images[stream] = (key, buf)
        self._images.move_to_end(stream)
        return buf


class Workspaces:
    """uint8 workspaces by (shape, device, stream), at most `limit`.  grow_only: the shape is left out of the key (pass ()),
    and a stream's buffer is only replaced by a larger one.  one_per_stream: a new shape on a stream drops its other ones."""

    def __init__(self, limit: int, grow_only: bool = False, one_per_stream: bool = False):
        self.limit, self.grow_only, self.one_per_stream = limit, grow_only, one_per_stream
        self._ws: OrderedDict = OrderedDict()          # (*shape, device index, stream) -> buffer, least recently used first

    def get(self, stream: int, shape: tuple, device: torch.device, nbytes) -> torch.Tensor:
        key = (*shape, device_index(device), stream)
        ws = self._ws.get(key)
        if ws is not None and not self.grow_only:
            self._ws.move_to_end(key)
            return ws
        size = _size(nbytes)
        if ws is not None and ws.numel() >= size:
            self._ws.move_to_end(key)
            return ws
        self._ws.pop(key, None)
        if self.one_per_stream:
            for k in [k for k in self._ws if k[-1] == stream]:
                del self._ws[k]
        while len(self._ws) >= self.limit:
            self._ws.popitem(last=False)
        ws = self._ws[key] = _new(size, torch.uint8, device)
        return ws

    def values(self):
        return self._ws.values()

    def items(self):
        return self._ws.items()


class TrainingBuffers:
    """A training forward's packed image and its history workspace, one of each per owner: the backward reads the history of
    the owner's latest forward.  The image is re-packed by every forward."""

    def __init__(self):
        self.image = self.history = self.extra = None
        self.key = None          # (B, T, device index) of the history
        self.extra_key = None    # ... of the second workspace of a backward with extras (made on first use)

    def packed(self, device: torch.device, nbytes, pack, zero: bool = False) -> torch.Tensor:
        size = _size(nbytes)
        if self.image is None or self.image.device != device:
            self.image = _new(size // 4, torch.float32, device, zero)
        pack(self.image, size)
        return self.image

    def history_for(self, B: int, T: int, device: torch.device, nbytes) -> torch.Tensor:
        key = (B, T, device_index(device))
        if self.key != key:
            size = _size(nbytes)
            self.history = None          # release the old history before the new one is allocated
            self.history = _new(size, torch.uint8, device)
            self.key = key
        return self.history

    def extra_for(self, B: int, T: int, device: torch.device, nbytes) -> torch.Tensor:
        key = (B, T, device_index(device))
        if self.extra_key != key:
            size = _size(nbytes)
            self.extra = None
            self.extra = _new(size, torch.uint8, device)
            self.extra_key = key
        return self.extra
