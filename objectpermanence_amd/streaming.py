"""Stateful OPNet streams: frames that arrive over time, with the LSTM state carried across calls.

`OPNet.forward` is whole-clip: every call starts from h0 = c0 = 0 (reference learned_models.py:39,46).  OPNet and
OPNetLstmMlp are causal, so a clip cut into chunks whose state is carried from one chunk to the next computes the same
function.  `OPNetStreams` keeps that state in a pool on the device, one row per open stream, and advances any set of
streams by k frames in one call (opnet_stream_step_f32, include/opnet_hip.h): k + 5 launches of the launch chain's own
kernels, so any chunking of a clip gives the bits of the whole-clip launch-chain forward of the same number of clips.

    streams = OPNetStreams(model, capacity=1024)
    ids = streams.open(3)                          # zero state
    y, logits = streams.step(ids, boxes)           # boxes [n, k, 15, 6] -> y [n, k, 4], logits [n, 15, k]
    h1, c1, h2, c2 = streams.get_state(ids)        # [1, n, H] each (nn.LSTM's h_n / c_n); OPNetLstmMlp: h2 = c2 = None
    streams.set_state(ids, h1, c1, h2, c2)
    streams.close(ids)

`LstmStackStreams` does the same for the stacked-LSTM reasoners BaselineLstm and NonLinearLstm (and their `_no_labels`
variants), through opseq_stream_step_f32 and the stacked launch chain's own step kernel:

    streams = LstmStackStreams(model, capacity=1024)
    ids = streams.open(3)
    y = streams.step(ids, x)                       # x [n, k, 15, 5] -> y [n, k, 4]
    h_n, c_n = streams.get_state(ids)              # [L, n, H] each (nn.LSTM's h_n / c_n)
    streams.set_state(ids, h_n, c_n)

Both pools take per-stream frame counts (`step(ids, boxes, lengths)`, lengths [n] in 0..k): stream i consumes
boxes[i, :lengths[i]], the rest of its row is padding that never reaches the state, and its outputs there are +0.0
(opnet_stream_step_ragged_f32 / opseq_stream_step_ragged_f32).  One call then serves a tick in which the streams have
different numbers of new frames, with the bits of the uniform call over the same streams on every valid frame.

TransformerLstm is not streamed: its encoder attends over the whole sequence, so a frame's output depends on later frames.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._device_cache import Workspaces
from .learned_models import BaselineLstm, NonLinearLstm, OPNet, OPNetLstmMlp, _stream_ptr


class StreamSlots:
    """Host bookkeeping of a pool's slot ids: which are open, and the checks every call makes before it launches
    anything (ids in range, distinct within the call, open)."""

    def __init__(self, capacity: int):
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError(f"capacity must be positive, got {capacity}")
        self.capacity = capacity
        self._is_open = np.zeros(capacity, dtype=bool)

    @property
    def free(self) -> int:
        return int(self.capacity - self._is_open.sum())

    def open(self, count: int) -> np.ndarray:
        """the `count` lowest free ids, now open"""
        count = int(count)
        if count <= 0:
            raise ValueError(f"count must be positive, got {count}")
        free = np.flatnonzero(~self._is_open)
        if count > len(free):
            raise RuntimeError(f"stream pool is full: {count} requested, {len(free)} of {self.capacity} free")
        ids = free[:count]
        self._is_open[ids] = True
        return ids

    def close(self, ids) -> None:
        self._is_open[self.check(ids)] = False

    def check(self, ids) -> np.ndarray:
        """ids as an int64 array, or an exception: out of range, repeated, or not open"""
        idx = np.asarray([ids] if isinstance(ids, (int, np.integer)) else ids)
        if idx.ndim != 1 or idx.size == 0:
            raise ValueError("ids must be a non-empty list of slot ids")
        if idx.dtype.kind not in "iu":
            raise TypeError(f"slot ids must be integers, got {idx.dtype}")
        idx = idx.astype(np.int64)
        bad = idx[(idx < 0) | (idx >= self.capacity)]
        if bad.size:
            raise IndexError(f"slot id {int(bad[0])} out of range [0, {self.capacity})")
        if np.unique(idx).size != idx.size:
            raise ValueError("slot ids must be distinct within one call")
        closed = idx[~self._is_open[idx]]
        if closed.size:
            raise KeyError(f"stream {int(closed[0])} is not open")
        return idx


def check_lengths(lengths, n: int, k: int) -> np.ndarray:
    """host per-stream frame counts as int32 [n], or an exception: wrong shape, not integers, or outside [0, k]"""
    a = np.asarray(lengths)
    if a.shape != (n,):
        raise ValueError(f"lengths must be [n={n}], got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise TypeError(f"lengths must be integers, got {a.dtype}")
    if n and (int(a.min()) < 0 or int(a.max()) > k):
        raise ValueError(f"lengths must lie in [0, k={k}], got [{int(a.min())}, {int(a.max())}]")
    return a.astype(np.int32)


def upload_async(a: np.ndarray, device) -> torch.Tensor:
    """a host array on the device without a host sync: a fresh pinned copy, then an asynchronous copy on the current
    stream (the caching host allocator keeps the pinned block until that copy has run)"""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


def call_entry(entry: str, args: list, lengths: Optional[torch.Tensor], at: int) -> None:
    """the C entry `entry` (a `..._f32` of include/opnet_hip.h) on args, or for a ragged call (lengths given) its
    `..._ragged_f32` twin, which takes the lengths pointer at position `at` of the same argument list"""
    if lengths is not None:
        entry = entry[:-len("_f32")] + "_ragged_f32"
        args = args[:at] + [lengths.data_ptr()] + args[at:]
    _lib.check(getattr(_lib.load(), entry)(*args), entry)


class _StreamPool:
    """What every stream pool shares: the model's ROCm device, the slot bookkeeping, the state pool (one row of `row`
    floats per slot, zero at open), the per-(n, k, stream) workspaces and the checks of `step`.  A subclass names its frame
    argument (`_frames`, `_frames_are`: for error texts), sets its frame shape `_frame_shape` (S, F) and implements
    `_step_slots`."""

    def __init__(self, model, capacity: int):
        slots = StreamSlots(capacity)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on MI355X only: move the model to a ROCm device first; there is "
                               "no CPU fallback")
        self.model = model
        self.device = dev
        self.slots = slots
        self.capacity = slots.capacity
        self._ws = Workspaces(8)

    def _alloc_state(self, row: int, what: str) -> None:
        if row == 0:
            _lib.check(-2, what)
        self._row = int(row)
        self.state = torch.zeros((self.capacity, self._row), dtype=torch.float32, device=self.device)

    # -- slots --------------------------------------------------------------------------------
    @property
    def free(self) -> int:
        return self.slots.free

    def open(self, count: int = 1) -> List[int]:
        """`count` new streams with a zero state (the reference's h0 = c0 = 0); returns their slot ids"""
        ids = self.slots.open(count)
        with torch.cuda.device(self.device):
            self.state.index_fill_(0, torch.from_numpy(ids).to(self.device), 0.0)
        return [int(i) for i in ids]

    def close(self, ids: Sequence[int]) -> None:
        self.slots.close(ids)

    # -- frames -------------------------------------------------------------------------------
    def step(self, ids: Sequence[int], x: torch.Tensor, lengths=None):
        """advance the streams `ids` by k frames: x [n, k, S, F] (row i belongs to ids[i]) -> the outputs of those frames
        (OPNetStreams: boxes [n, k, 15, 6] -> (y [n, k, 4], logits [n, 15, k]); LstmStackStreams: x [n, k, 15, 5] ->
        y [n, k, 4]).  lengths ([n] ints in 0..k, on the host or an int32 device tensor): stream i advances by its first
        lengths[i] frames only; the outputs are +0.0 on the others."""
        name = self._frames
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.step runs on MI355X only: `{name}` must be a tensor on a ROCm device")
        if x.device != self.device:
            raise ValueError(f"{self._frames_are} on {x.device}, the stream pool on {self.device}")
        idx = self.slots.check(ids)
        n = idx.size
        S, F = self._frame_shape
        if x.dim() != 4 or x.shape[0] != n or x.shape[2] != S or x.shape[3] != F or x.shape[1] < 1:
            raise ValueError(f"{name} must be [n={n}, k>=1, {S}, {F}], got {tuple(x.shape)}")
        slots, lens = self._device_ids(idx, lengths, int(x.shape[1]))
        return self._step_slots(slots, x, lens)

    def _device_ids(self, idx: np.ndarray, lengths, k: int):
        """(slots, lengths) on the device for a call of k frames: the uniform call (lengths None) uploads the slot ids as
        it always has; host lengths are checked and go up with the ids in one pinned copy; an int32 device tensor [n] is
        taken as is (its values are clamped to [0, k] by the kernels).  No host sync on the ragged routes."""
        n = idx.size
        with torch.cuda.device(self.device):
            if lengths is None:
                return torch.from_numpy(idx.astype(np.int32)).to(self.device), None   # one small H2D copy on this stream
            if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
                if lengths.device != self.device:
                    raise ValueError(f"lengths are on {lengths.device}, the stream pool on {self.device}")
                if lengths.dtype != torch.int32 or tuple(lengths.shape) != (n,):
                    raise ValueError(f"device lengths must be int32 [n={n}], got {lengths.dtype} {tuple(lengths.shape)}")
                return upload_async(idx.astype(np.int32), self.device), lengths.contiguous()
            both = upload_async(np.concatenate([idx.astype(np.int32), check_lengths(lengths, n, k)]), self.device)
            return both[:n], both[n:]


class OPNetStreams(_StreamPool):
    """A pool of `capacity` OPNet (or OPNetLstmMlp) streams on the model's ROCm device.  Calls are enqueued on the
    current torch stream and are inference only (no autograd graph).  The model's own packed weight image is used, so an
    in-place parameter update takes effect on the next call."""
    _frames, _frames_are, _frame_shape = "boxes", "boxes are", (15, 6)

    def __init__(self, model, capacity: int = 1024):
        if isinstance(model, OPNet):
            self._mlp = 0
        elif isinstance(model, OPNetLstmMlp):
            self._mlp = 1
        else:
            raise TypeError(f"OPNetStreams serves OPNet and OPNetLstmMlp, not {type(model).__name__} (BaselineLstm and "
                            "NonLinearLstm are streamed by LstmStackStreams; transformer_lstm is not streamed: its encoder "
                            "attends over the whole sequence)")
        super().__init__(model, capacity)
        self.H1, self.H2 = model._h1, model._h2
        self._alloc_state(_lib.load().opnet_stream_state_floats(self.H1, self.H2), "opnet_stream_state_floats")

    # -- state --------------------------------------------------------------------------------
    def get_state(self, ids: Sequence[int]):
        """(h1, c1, h2, c2) of the streams, [1, n, H] each in nn.LSTM's (num_layers, batch, hidden) layout; copies"""
        idx = self.slots.check(ids)
        H1, H2 = self.H1, self.H2
        with torch.cuda.device(self.device):
            rows = self.state.index_select(0, torch.from_numpy(idx).to(self.device))
        h1 = rows[:, :H1].unsqueeze(0).contiguous()
        c1 = rows[:, H1:2 * H1].unsqueeze(0).contiguous()
        if self._mlp:
            return h1, c1, None, None
        h2 = rows[:, 2 * H1:2 * H1 + H2].unsqueeze(0).contiguous()
        c2 = rows[:, 2 * H1 + H2:].unsqueeze(0).contiguous()
        return h1, c1, h2, c2

    def set_state(self, ids: Sequence[int], h1: torch.Tensor, c1: torch.Tensor,
                  h2: Optional[torch.Tensor] = None, c2: Optional[torch.Tensor] = None) -> None:
        """overwrite the state of open streams with [1, n, H] tensors (h2 / c2 are required for OPNet and must be None
        for OPNetLstmMlp, which has no video LSTM)"""
        idx = self.slots.check(ids)
        n = idx.size
        parts = [(h1, self.H1, "h1"), (c1, self.H1, "c1")]
        if self._mlp:
            if h2 is not None or c2 is not None:
                raise ValueError("OPNetLstmMlp has no video LSTM: h2 and c2 must be None")
        else:
            if h2 is None or c2 is None:
                raise ValueError("OPNet needs h2 and c2")
            parts += [(h2, self.H2, "h2"), (c2, self.H2, "c2")]
        cols = []
        for t, H, name in parts:
            if tuple(t.shape) != (1, n, H):
                raise ValueError(f"{name} must be [1, {n}, {H}], got {tuple(t.shape)}")
            cols.append(t[0].to(device=self.device, dtype=torch.float32))
        with torch.cuda.device(self.device):
            dst = torch.from_numpy(idx).to(self.device)
            if self._mlp:      # leave the h2 / c2 columns as they are
                self.state[:, :2 * self.H1].index_copy_(0, dst, torch.cat(cols, dim=1))
            else:
                self.state.index_copy_(0, dst, torch.cat(cols, dim=1))

    # -- frames -------------------------------------------------------------------------------
    def _step_slots(self, slots: torch.Tensor, boxes: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """boxes [n, k, 15, 6] -> (y [n, k, 4], logits [n, 15, k]), with the slot ids (and the lengths of a ragged call)
        already on the device (int32 [n], checked by the caller) and boxes checked: no host synchronisation"""
        n, k = int(boxes.shape[0]), int(boxes.shape[1])
        lib = _lib.load()
        with torch.no_grad(), torch.cuda.device(self.device):
            boxes = boxes.contiguous().float()
            packed = self.model._packed_weights(self.device)
            stream = _stream_ptr(self.device)
            ws = self._ws.get(stream, (n, k), self.device, (lib.opnet_stream_workspace_bytes, n, k, self.H1, self.H2))
            y = torch.empty((n, k, 4), dtype=torch.float32, device=self.device)
            logits = torch.empty((n, 15, k), dtype=torch.float32, device=self.device)
            call_entry("opnet_stream_step_f32",
                            [boxes.data_ptr(), slots.data_ptr(), self.state.data_ptr(), packed.data_ptr(), y.data_ptr(),
                             logits.data_ptr(), ws.data_ptr(), ws.numel(), n, k, self.capacity, self.H1, self.H2, self._mlp,
                             stream], lengths, 2)
        return y, logits


class LstmStackStreams(_StreamPool):
    """A pool of `capacity` BaselineLstm (or NonLinearLstm) streams on the model's ROCm device.  Calls are enqueued on the
    current torch stream and are inference only (no autograd graph).  The model's own packed weight image (the launch
    chain's, _LstmStackRunner._packed_weights) is used, so an in-place parameter update takes effect on the next call.
    A stream's state row is [h_0 | c_0 | h_1 | c_1 ...] over the model's L layers."""
    _frames, _frames_are = "x", "x is"

    def __init__(self, model, capacity: int = 1024):
        if isinstance(model, NonLinearLstm):
            self._embed = True
        elif isinstance(model, BaselineLstm):
            self._embed = False
        else:
            raise TypeError(f"LstmStackStreams serves BaselineLstm and NonLinearLstm, not {type(model).__name__} (OPNet and "
                            "OPNetLstmMlp are streamed by OPNetStreams; transformer_lstm is not streamed: its encoder "
                            "attends over the whole sequence, so it is not causal)")
        super().__init__(model, capacity)
        r = model._runner
        self.L, self.KX, self.H = r.L, r.KX, r.H
        self.slots_per_frame, self.features = model.max_objects_in_frame, model.bb_in_dim
        self._frame_shape = (self.slots_per_frame, self.features)
        self._alloc_state(_lib.load().opseq_stream_state_floats(self.L, self.H), "opseq_stream_state_floats")

    # -- state --------------------------------------------------------------------------------
    def get_state(self, ids: Sequence[int]):
        """(h_n, c_n) of the streams, [L, n, H] each in nn.LSTM's (num_layers, batch, hidden) layout; copies"""
        idx = self.slots.check(ids)
        with torch.cuda.device(self.device):
            rows = self.state.index_select(0, torch.from_numpy(idx).to(self.device))
        rows = rows.view(idx.size, self.L, 2, self.H)
        return rows[:, :, 0].transpose(0, 1).contiguous(), rows[:, :, 1].transpose(0, 1).contiguous()

    def set_state(self, ids: Sequence[int], h_n: torch.Tensor, c_n: torch.Tensor) -> None:
        """overwrite the state of open streams with nn.LSTM-shaped [L, n, H] tensors"""
        idx = self.slots.check(ids)
        n = idx.size
        for t, name in ((h_n, "h_n"), (c_n, "c_n")):
            if tuple(t.shape) != (self.L, n, self.H):
                raise ValueError(f"{name} must be [{self.L}, {n}, {self.H}], got {tuple(t.shape)}")
        with torch.cuda.device(self.device):
            h = h_n.to(device=self.device, dtype=torch.float32).transpose(0, 1)
            c = c_n.to(device=self.device, dtype=torch.float32).transpose(0, 1)
            rows = torch.stack([h, c], dim=2).reshape(n, self._row)
            self.state.index_copy_(0, torch.from_numpy(idx).to(self.device), rows)

    # -- frames -------------------------------------------------------------------------------
    def _step_slots(self, slots: torch.Tensor, x: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [n, k, 15, 5] -> y [n, k, 4], with the slot ids (and the lengths of a ragged call) already on the device
        (int32 [n], checked by the caller) and x checked: no host synchronisation"""
        n, k = int(x.shape[0]), int(x.shape[1])
        S = self.slots_per_frame
        m = self.model
        lib = _lib.load()
        with torch.no_grad(), torch.cuda.device(self.device):
            x = x.contiguous().float()
            stream = _stream_ptr(self.device)
            if self._embed:      # relu(Linear 5 -> F) per slot, as NonLinearLstm.forward
                feats = torch.empty((n, k, self.KX), dtype=torch.float32, device=self.device)
                rc = lib.opseq_slot_embed_relu_f32(x.data_ptr(), m.boxes_linear.weight.data_ptr(), feats.data_ptr(), n * k, S,
                                                   self.KX // S, stream)
                _lib.check(rc, "opseq_slot_embed_relu_f32")
            else:
                feats = x
            packed = m._runner._packed_weights(m._runner.weights(m.video_LSTM, m.predictions_layer), self.device, stream)
            ws = self._ws.get(stream, (n, k), self.device, (lib.opseq_stream_workspace_bytes, n, k, self.L, self.KX, self.H))
            y = torch.empty((n, k, 4), dtype=torch.float32, device=self.device)
            call_entry("opseq_stream_step_f32",
                            [feats.data_ptr(), slots.data_ptr(), self.state.data_ptr(), packed.data_ptr(), y.data_ptr(),
                             ws.data_ptr(), ws.numel(), n, k, self.capacity, self.L, self.KX, self.H, stream], lengths, 2)
        return y
