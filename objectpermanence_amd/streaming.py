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

A call that carries many frames (a backlog, a video decoded in pieces, a restored checkpoint fast-forwarded) is better served
by ONE persistent launch than by k + 5 dependent ones: `OPNetStreams(model, capacity, engine="persistent")`, or
`step(ids, boxes, engine="persistent")` for one call (opnet_stream_step_x4_f32: the 4-clip persistent forward, reading each
stream's state from the pool and writing it back; OPNet at the reference hidden sizes on a whole MI355X, uniform calls only).
Both engines work on the same pool rows, so a stream can be warmed up on one and ticked on the other.  Each engine is
chunk-invariant on its own; the two round differently in the last places, which is why the engine is always the caller's
choice and never a function of k.  Persistent steps are watched by the model's LaunchMonitor: call `verify_launches()` at a
sync point before trusting outputs on the host, as after `model(boxes)`.

`LstmStackStreams(model, capacity, engine="persistent")` / `step(ids, x, engine="persistent")` is the same choice for the
stacked reasoners (opseq_stream_step_x_f32: the 4-clip persistent stacked LSTM, seqx_forward, with the state handed in and
out; H = 512 shapes that opseq_xcd_supported accepts, on a whole MI355X, uniform calls only), with the same rules: no
automatic choice, a checked precondition and not a fallback, watched by the runner's LaunchMonitor and healed on the chain.

TransformerLstm is not streamed: its encoder attends over the whole sequence, so a frame's output depends on later frames.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._device_cache import Workspaces
from .launch_monitor import verify_launches
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


ENGINES = ("chain", "persistent")


def check_engine(engine, default: Optional[str] = None) -> str:
    """`engine` as one of ENGINES (None: `default`, where a default exists), or an exception"""
    if engine is None and default is not None:
        return default
    if not isinstance(engine, str):
        raise TypeError(f"engine must be one of {ENGINES}, got {type(engine).__name__}")
    if engine not in ENGINES:
        raise ValueError(f"engine must be one of {ENGINES}, got {engine!r} (there is no automatic choice: the two engines "
                         "round differently, so which one runs is never decided behind the caller's back)")
    return engine


class ReplayEntry:
    """one logged call: the pool rows it names (`slots`), their contents before it (`before`), what is needed to run it
    again (`payload`), and - for a watched persistent launch - the `redo` its monitor holds"""
    __slots__ = ("slots", "before", "payload", "redo", "healed")

    def __init__(self, slots, before, payload):
        self.slots, self.before, self.payload = slots, before, payload
        self.redo: Optional[Callable[[], None]] = None
        self.healed = False


class StreamReplayLog:
    """The undo / redo log of a stream pool, kept while a persistent step of the pool is unverified.

    A whole-clip forward that gave up is healed by running it again; a stream step has a past: by the time the host learns
    that call i gave up, calls i+1 .. m have already advanced the pool from the state call i left behind.  A step that gave
    up leaves its own rows as they were (opnet_stream_x4_writeback), so undoing calls m .. i+1 - newest first, each putting
    back the rows it named as they were before it - gives exactly the pool before call i; calls i .. m are then run again in
    order through the launch chain, into the output tensors the caller already holds.

    `restore(slots, before)` puts rows back; `rerun(payload)` runs a logged call again (on the chain).  Both are the
    pool's; the log itself only keeps order, so it is tested on the host with numpy."""

    def __init__(self, restore: Callable, rerun: Callable):
        self._restore, self._rerun = restore, rerun
        self.entries: List[ReplayEntry] = []

    def __len__(self) -> int:
        return len(self.entries)

    def record(self, slots, before, payload) -> ReplayEntry:
        entry = ReplayEntry(slots, before, payload)
        self.entries.append(entry)
        return entry

    def prune(self, unverified: Callable[[ReplayEntry], bool]) -> None:
        """drop every entry in front of the oldest one whose launch is still `unverified` (all of them when none is): an
        abort found later can only rewind to that entry"""
        for i, entry in enumerate(self.entries):
            if entry.redo is not None and not entry.healed and unverified(entry):
                del self.entries[:i]
                return
        self.entries.clear()

    def replay(self, entry: ReplayEntry) -> int:
        """rewind the pool to the state before `entry` and run it and every later logged call again; returns how many
        calls were run.  An entry that an earlier replay has already run again (or that was pruned) is left alone."""
        if entry.healed or not any(e is entry for e in self.entries):
            return 0
        i = next(j for j, e in enumerate(self.entries) if e is entry)
        todo = self.entries[i:]
        for e in reversed(todo):
            self._restore(e.slots, e.before)
        for e in todo:
            self._rerun(e.payload)
            e.healed = True
        return len(todo)

    def clear(self) -> None:
        self.entries.clear()


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
        self._gave_up = False
        self._log = StreamReplayLog(self._restore_rows, self._rerun)
        self.healed_calls = 0            # calls run again on the chain after a persistent step gave up
        self.engine = "chain"

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
            dst = torch.from_numpy(ids).to(self.device)
            self.state.index_fill_(0, dst, 0.0)
            if len(self._log):       # a replay must zero the rows again
                self._log.record(dst, torch.zeros((len(ids), self._row), dtype=torch.float32, device=self.device),
                                 ("rows", dst, None))
        return [int(i) for i in ids]

    def close(self, ids: Sequence[int]) -> None:
        self.slots.close(ids)

    # -- frames -------------------------------------------------------------------------------
    def step(self, ids: Sequence[int], x: torch.Tensor, lengths=None, engine: Optional[str] = None):
        """advance the streams `ids` by k frames: x [n, k, S, F] (row i belongs to ids[i]) -> the outputs of those frames
        (OPNetStreams: boxes [n, k, 15, 6] -> (y [n, k, 4], logits [n, 15, k]); LstmStackStreams: x [n, k, 15, 5] ->
        y [n, k, 4]).  lengths ([n] ints in 0..k, on the host or an int32 device tensor): stream i advances by its first
        lengths[i] frames only; the outputs are +0.0 on the others.  engine: "chain" or "persistent" for this call,
        None = the pool's default."""
        self._check_engine(engine, lengths)
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
        return self._step_slots(slots, x, lens, engine=engine)

    # -- engines ------------------------------------------------------------------------------
    def _launch_monitor(self):
        """the LaunchMonitor that watches the model's persistent launches"""
        return self.model._monitor

    def _check_persistent(self) -> None:
        """the preconditions of the pool's persistent engine, or an exception (the subclass's)"""
        raise NotImplementedError

    def _check_not_given_up(self) -> None:
        if self._gave_up:
            raise RuntimeError("a persistent step of this pool gave up earlier and was healed on the launch chain; the pool "
                               "stays on engine='chain'")

    def _check_engine(self, engine, lengths) -> None:
        if check_engine(engine, self.engine) != "persistent":
            return
        self._check_persistent()
        if lengths is not None:
            raise ValueError("engine='persistent' takes uniform calls only: ragged persistent steps are not built "
                             "(pass lengths with engine='chain')")

    def verify_launches(self) -> int:
        """wait for the persistent steps (and forwards) of the model issued so far; a step that gave up is healed: the pool
        is rewound to the state before it, that call and every later one run again on the launch chain into the tensors they
        returned, and the pool stays on the chain.  Returns the number of launches that gave up.  Call it at the sync point
        you already have, before anything reads a persistent step's outputs on the host."""
        n = verify_launches(self.model)
        self._prune_log()
        return n

    # -- the replay log (StreamReplayLog) -----------------------------------------------------------
    def _prune_log(self) -> None:
        if len(self._log):
            mon = self._launch_monitor()
            mon.reap()
            self._log.prune(lambda e: mon.watching(e.redo))

    def _log_write(self, dst: torch.Tensor, rows: torch.Tensor) -> None:
        """a set_state while the log is kept: a replay has to repeat it"""
        self._prune_log()
        if len(self._log):
            self._log.record(dst, self.state.index_select(0, dst), ("rows", dst, rows.clone()))

    def log_followup(self, fn: Callable[[], None]) -> None:
        """device work a caller derived from the outputs of the step it has just made (DetectorStreams: the pixel boxes of
        y): while the log is kept it is recorded behind that step, so that a replay which rewrites the step's outputs runs
        `fn()` again - into the same tensors, which is `fn`'s business.  Names no pool rows."""
        if len(self._log):
            self._log.record(self.state.new_empty(0, dtype=torch.int64), self.state[:0], ("call", fn))

    def _restore_rows(self, slots: torch.Tensor, before: torch.Tensor) -> None:
        self.state.index_copy_(0, slots.long(), before)

    def _rerun(self, payload) -> None:
        if payload[0] == "call":         # work derived from a step's outputs (log_followup)
            payload[1]()
            return
        if payload[0] == "rows":
            _, dst, rows = payload
            if rows is None:
                self.state.index_fill_(0, dst, 0.0)
            else:
                self.state.index_copy_(0, dst, rows)
            return
        _, slots, x, lengths, *out = payload
        self._step_chain(slots, x, lengths, tuple(out))
        self.healed_calls += 1

    def _heal(self, entry: ReplayEntry) -> None:
        """the monitor's redo of a persistent step that gave up"""
        if entry.healed:
            return               # run again already, behind an earlier step that gave up
        with torch.no_grad(), torch.cuda.device(self.device):
            self.engine, self._gave_up = "chain", True     # for good: a later engine="persistent" is refused
            # the later calls of the log may still be running, on other streams too: the rows are put back behind all of them
            torch.cuda.synchronize(self.device)
            self._log.replay(entry)
            self._log.clear()

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

    def __init__(self, model, capacity: int = 1024, engine: str = "chain"):
        if isinstance(model, OPNet):
            self._mlp = 0
        elif isinstance(model, OPNetLstmMlp):
            self._mlp = 1
        else:
            raise TypeError(f"OPNetStreams serves OPNet and OPNetLstmMlp, not {type(model).__name__} (BaselineLstm and "
                            "NonLinearLstm are streamed by LstmStackStreams; transformer_lstm is not streamed: its encoder "
                            "attends over the whole sequence)")
        engine = check_engine(engine)
        if engine == "persistent" and self._mlp:
            raise TypeError(self._NO_MLP)
        super().__init__(model, capacity)
        self.H1, self.H2 = model._h1, model._h2
        self._alloc_state(_lib.load().opnet_stream_state_floats(self.H1, self.H2), "opnet_stream_state_floats")
        self._x4ws = Workspaces(8)
        self._x4_ok: Optional[bool] = None
        if engine == "persistent":
            self._check_persistent()
            self.engine = engine

    _NO_MLP = ("engine='persistent' serves OPNet only: OPNetLstmMlp has no persistent kernel (its streams run on the "
               "launch chain)")

    # -- engines ------------------------------------------------------------------------------
    def _check_persistent(self) -> None:
        """the preconditions of the persistent engine, or an exception"""
        if self._mlp:
            raise TypeError(self._NO_MLP)
        self._check_not_given_up()
        if self._x4_ok is None:
            with torch.cuda.device(self.device):
                self._x4_ok = bool(_lib.load().opnet_xcd_supported(self.H1, self.H2))
        if not self._x4_ok:
            raise ValueError(f"engine='persistent' needs the reference hidden sizes (256, 512) on a whole MI355X (8 XCDs x 32 "
                             f"CUs visible); this pool has H1={self.H1}, H2={self.H2} on {self.device}: use engine='chain'")

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
                rows = torch.cat(cols, dim=1)
                self._log_write(dst, rows)
                self.state.index_copy_(0, dst, rows)

    # -- frames -------------------------------------------------------------------------------
    def _step_slots(self, slots: torch.Tensor, boxes: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                    engine: Optional[str] = None):
        """boxes [n, k, 15, 6] -> (y [n, k, 4], logits [n, 15, k]), with the slot ids (and the lengths of a ragged call)
        already on the device (int32 [n], checked by the caller) and boxes checked: no host synchronisation"""
        self._check_engine(engine, lengths)
        with torch.no_grad(), torch.cuda.device(self.device):
            boxes = boxes.contiguous().float()
            if check_engine(engine, self.engine) == "persistent":
                return self._step_persistent(slots, boxes)
            self._prune_log()
            before = self.state.index_select(0, slots.long()) if len(self._log) else None
            out = self._step_chain(slots, boxes, lengths)
            if before is not None:
                self._log.record(slots, before, ("step", slots, boxes, lengths, *out))
        return out

    def _step_chain(self, slots: torch.Tensor, boxes: torch.Tensor, lengths: Optional[torch.Tensor], out=None):
        """the launch-per-step engine (opnet_stream_step_f32); out: (y, logits) to fill instead of new tensors"""
        n, k = int(boxes.shape[0]), int(boxes.shape[1])
        lib = _lib.load()
        packed = self.model._packed_weights(self.device)
        stream = _stream_ptr(self.device)
        ws = self._ws.get(stream, (n, k), self.device, (lib.opnet_stream_workspace_bytes, n, k, self.H1, self.H2))
        direct = out is not None and out[0].is_contiguous() and out[1].is_contiguous()
        y = out[0] if direct else torch.empty((n, k, 4), dtype=torch.float32, device=self.device)
        logits = out[1] if direct else torch.empty((n, 15, k), dtype=torch.float32, device=self.device)
        call_entry("opnet_stream_step_f32",
                        [boxes.data_ptr(), slots.data_ptr(), self.state.data_ptr(), packed.data_ptr(), y.data_ptr(),
                         logits.data_ptr(), ws.data_ptr(), ws.numel(), n, k, self.capacity, self.H1, self.H2, self._mlp,
                         stream], lengths, 2)
        if out is not None and not direct:
            out[0].copy_(y)
            out[1].copy_(logits)
        return (y, logits) if out is None else out

    def _step_persistent(self, slots: torch.Tensor, boxes: torch.Tensor):
        """the same step as one persistent launch per piece (opnet_stream_step_x4_f32): pieces of at most
        opnet_stream_x4_max_streams() streams, and of as many frames as one workspace holds (chunk invariance makes the cut
        in time exact).  Every launch is watched by the model's monitor and logged for replay."""
        n, k = int(boxes.shape[0]), int(boxes.shape[1])
        lib = _lib.load()
        H1, H2 = self.H1, self.H2
        nmax = int(lib.opnet_stream_x4_max_streams())
        kmax = k
        while kmax > 1 and lib.opnet_stream_x4_workspace_bytes(min(n, nmax), kmax, H1, H2) == 0:
            kmax = (kmax + 1) // 2
        stream = _stream_ptr(self.device)
        x4packed = self.model._x4_packed_weights(self.device, stream)
        y = torch.empty((n, k, 4), dtype=torch.float32, device=self.device)
        logits = torch.empty((n, 15, k), dtype=torch.float32, device=self.device)
        self._prune_log()
        for lo in range(0, n, nmax):
            hi = min(n, lo + nmax)
            m = hi - lo
            sl = slots[lo:hi]
            for t0 in range(0, k, kmax):
                t1 = min(k, t0 + kmax)
                kk = t1 - t0
                whole = kk == k
                bx = boxes[lo:hi] if whole else boxes[lo:hi, t0:t1].contiguous()
                yy = y[lo:hi] if whole else torch.empty((m, kk, 4), dtype=torch.float32, device=self.device)
                ll = logits[lo:hi] if whole else torch.empty((m, 15, kk), dtype=torch.float32, device=self.device)
                ws = self._x4ws.get(stream, (m, kk), self.device, (lib.opnet_stream_x4_workspace_bytes, m, kk, H1, H2))
                if self._gave_up:    # found by a watch of this very loop: the rest of the call runs on the chain, unlogged
                    self._step_chain(sl, bx, None, (yy, ll))
                    if not whole:
                        y[lo:hi, t0:t1].copy_(yy)
                        logits[lo:hi, :, t0:t1].copy_(ll)
                    continue
                entry = self._log.record(sl, self.state.index_select(0, sl.long()), ("step", sl, bx, None, yy, ll))
                _lib.check(lib.opnet_stream_step_x4_f32(bx.data_ptr(), sl.data_ptr(), self.state.data_ptr(),
                                                        x4packed.data_ptr(), yy.data_ptr(), ll.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), m, kk, self.capacity, H1, H2, stream),
                           "opnet_stream_step_x4_f32")
                entry.redo = lambda e=entry: self._heal(e)
                self.model._monitor.watch(ws, lib.opnet_stream_x4_status_offset(m, kk, H1, H2), entry.redo,
                                          "opnet_stream_step_x4")
                if not whole:        # a piece in time -> its place in the caller's tensors, again after a replay of the piece
                    def place(yv=y[lo:hi, t0:t1], lv=logits[lo:hi, :, t0:t1], yy=yy, ll=ll):
                        yv.copy_(yy)
                        lv.copy_(ll)
                    place()
                    self.log_followup(place)
        return y, logits


class LstmStackStreams(_StreamPool):
    """A pool of `capacity` BaselineLstm (or NonLinearLstm) streams on the model's ROCm device.  Calls are enqueued on the
    current torch stream and are inference only (no autograd graph).  The model's own packed weight images (the launch
    chain's, _LstmStackRunner._packed_weights, and the persistent kernel's, _x_packed_weights) are used, so an in-place
    parameter update takes effect on the next call.  A stream's state row is [h_0 | c_0 | h_1 | c_1 ...] over the model's L
    layers.  engine: the pool's default, "chain" or "persistent" (module docstring); `step(..., engine=)` chooses per call."""
    _frames, _frames_are = "x", "x is"

    def __init__(self, model, capacity: int = 1024, engine: str = "chain"):
        if isinstance(model, NonLinearLstm):
            self._embed = True
        elif isinstance(model, BaselineLstm):
            self._embed = False
        else:
            raise TypeError(f"LstmStackStreams serves BaselineLstm and NonLinearLstm, not {type(model).__name__} (OPNet and "
                            "OPNetLstmMlp are streamed by OPNetStreams; transformer_lstm is not streamed: its encoder "
                            "attends over the whole sequence, so it is not causal)")
        engine = check_engine(engine)
        r = model._runner
        self.L, self.KX, self.H = r.L, r.KX, r.H
        if engine == "persistent":
            self._check_persistent_shape()
        super().__init__(model, capacity)
        self.slots_per_frame, self.features = model.max_objects_in_frame, model.bb_in_dim
        self._frame_shape = (self.slots_per_frame, self.features)
        self._alloc_state(_lib.load().opseq_stream_state_floats(self.L, self.H), "opseq_stream_state_floats")
        self._xws = Workspaces(8)
        self._x_ok: Optional[bool] = None
        if engine == "persistent":
            self._check_persistent()
            self.engine = engine

    # -- engines ------------------------------------------------------------------------------
    def _launch_monitor(self):
        return self.model._runner._monitor

    def _check_persistent_shape(self) -> None:
        """the persistent kernel's shapes (a host-side question: asked before the pool exists)"""
        if _lib.load().opseq_stream_x_workspace_bytes(1, 1, self.L, self.KX, self.H) == 0:
            raise ValueError(f"engine='persistent' needs the reference shapes of the stacked reasoners (H = 512; BaselineLstm's "
                             f"one layer with KX <= 80, NonLinearLstm's two with a hoisted input); this model has L={self.L}, "
                             f"KX={self.KX}, H={self.H}: use engine='chain'")

    def _check_persistent(self) -> None:
        """the preconditions of the persistent engine, or an exception"""
        self._check_persistent_shape()
        self._check_not_given_up()
        if self._x_ok is None:
            with torch.cuda.device(self.device):
                self._x_ok = bool(_lib.load().opseq_xcd_supported(self.L, self.KX, self.H))
        if not self._x_ok:
            raise ValueError(f"engine='persistent' needs a whole MI355X (8 XCDs x 32 CUs visible) and the persistent stacked LSTM "
                             f"switched on (OPSEQ_XCD); not so on {self.device}: use engine='chain'")

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
            dst = torch.from_numpy(idx).to(self.device)
            self._log_write(dst, rows)
            self.state.index_copy_(0, dst, rows)

    # -- frames -------------------------------------------------------------------------------
    def _step_slots(self, slots: torch.Tensor, x: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                    engine: Optional[str] = None) -> torch.Tensor:
        """x [n, k, 15, 5] -> y [n, k, 4], with the slot ids (and the lengths of a ragged call) already on the device
        (int32 [n], checked by the caller) and x checked: no host synchronisation"""
        self._check_engine(engine, lengths)
        with torch.no_grad(), torch.cuda.device(self.device):
            x = x.contiguous().float()
            if check_engine(engine, self.engine) == "persistent":
                return self._step_persistent(slots, x)
            self._prune_log()
            before = self.state.index_select(0, slots.long()) if len(self._log) else None
            (y,) = self._step_chain(slots, x, lengths)
            if before is not None:
                self._log.record(slots, before, ("step", slots, x, lengths, y))
        return y

    def _features(self, x: torch.Tensor, stream: int) -> torch.Tensor:
        """the LSTM stack's input rows [n, k, KX] of frames x [n, k, 15, 5]: NonLinearLstm's relu(Linear 5 -> F) per slot, as
        NonLinearLstm.forward (in front of either engine; a replayed step starts from x again); BaselineLstm's are x itself"""
        if not self._embed:
            return x
        n, k = int(x.shape[0]), int(x.shape[1])
        S = self.slots_per_frame
        feats = torch.empty((n, k, self.KX), dtype=torch.float32, device=self.device)
        rc = _lib.load().opseq_slot_embed_relu_f32(x.data_ptr(), self.model.boxes_linear.weight.data_ptr(), feats.data_ptr(),
                                                   n * k, S, self.KX // S, stream)
        _lib.check(rc, "opseq_slot_embed_relu_f32")
        return feats

    def _step_chain(self, slots: torch.Tensor, x: torch.Tensor, lengths: Optional[torch.Tensor], out=None):
        """the launch-per-step engine (opseq_stream_step_f32); out: (y,) to fill instead of a new tensor.  Returns (y,)."""
        n, k = int(x.shape[0]), int(x.shape[1])
        m = self.model
        lib = _lib.load()
        stream = _stream_ptr(self.device)
        feats = self._features(x, stream)
        packed = m._runner._packed_weights(m._runner.weights(m.video_LSTM, m.predictions_layer), self.device, stream)
        ws = self._ws.get(stream, (n, k), self.device, (lib.opseq_stream_workspace_bytes, n, k, self.L, self.KX, self.H))
        direct = out is not None and out[0].is_contiguous()
        y = out[0] if direct else torch.empty((n, k, 4), dtype=torch.float32, device=self.device)
        call_entry("opseq_stream_step_f32",
                        [feats.data_ptr(), slots.data_ptr(), self.state.data_ptr(), packed.data_ptr(), y.data_ptr(),
                         ws.data_ptr(), ws.numel(), n, k, self.capacity, self.L, self.KX, self.H, stream], lengths, 2)
        if out is not None and not direct:
            out[0].copy_(y)
        return (y,) if out is None else out

    def _step_persistent(self, slots: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """the same step as one persistent launch per piece (opseq_stream_step_x_f32): pieces of at most
        opseq_stream_x_max_streams(L) streams, and of as many frames as one workspace holds (chunk invariance makes the cut
        in time exact).  Every launch is watched by the runner's monitor and logged for replay."""
        n, k = int(x.shape[0]), int(x.shape[1])
        m = self.model
        lib = _lib.load()
        L, KX, H = self.L, self.KX, self.H
        nmax = int(lib.opseq_stream_x_max_streams(L))
        kmax = k
        while kmax > 1 and lib.opseq_stream_x_workspace_bytes(min(n, nmax), kmax, L, KX, H) == 0:
            kmax = (kmax + 1) // 2
        stream = _stream_ptr(self.device)
        xpacked = m._runner._x_packed_weights(m._runner.weights(m.video_LSTM, m.predictions_layer), self.device, stream)
        w_head = m.predictions_layer.weight
        y = torch.empty((n, k, 4), dtype=torch.float32, device=self.device)
        self._prune_log()
        for lo in range(0, n, nmax):
            hi = min(n, lo + nmax)
            nn = hi - lo
            sl = slots[lo:hi]
            for t0 in range(0, k, kmax):
                t1 = min(k, t0 + kmax)
                kk = t1 - t0
                whole = kk == k
                xx = x[lo:hi] if whole else x[lo:hi, t0:t1].contiguous()
                yy = y[lo:hi] if whole else torch.empty((nn, kk, 4), dtype=torch.float32, device=self.device)
                if self._gave_up:    # found by a watch of this very loop: the rest of the call runs on the chain, unlogged
                    self._step_chain(sl, xx, None, (yy,))
                    if not whole:
                        y[lo:hi, t0:t1].copy_(yy)
                    continue
                feats = self._features(xx, stream)
                ws = self._xws.get(stream, (nn, kk), self.device, (lib.opseq_stream_x_workspace_bytes, nn, kk, L, KX, H))
                entry = self._log.record(sl, self.state.index_select(0, sl.long()), ("step", sl, xx, None, yy))
                _lib.check(lib.opseq_stream_step_x_f32(feats.data_ptr(), sl.data_ptr(), self.state.data_ptr(),
                                                       xpacked.data_ptr(), w_head.data_ptr(), yy.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), nn, kk, self.capacity, L, KX, H, stream),
                           "opseq_stream_step_x_f32")
                entry.redo = lambda e=entry: self._heal(e)
                self._launch_monitor().watch(ws, lib.opseq_stream_x_status_offset(nn, kk, L, KX, H), entry.redo,
                                             "opseq_stream_step_x")
                if not whole:        # a piece in time -> its place in the caller's tensor, again after a replay of the piece
                    def place(yv=y[lo:hi, t0:t1], yy=yy):
                        yv.copy_(yy)
                    place()
                    self.log_followup(place)
        return y
