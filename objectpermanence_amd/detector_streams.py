"""Live detections encoded on the device into stateful streams: detector -> per-frame encoder -> stream pool.

`OPNetStreams` and `LstmStackStreams` (streaming.py) carry a reasoner's state across calls, but take model input rows.
The offline encoder (datasets.encode_boxes) cannot make those rows for a stream: its slot order is the whole clip's
distinct class ids, snitch first, then ascending.  `DetectorStreams` keeps one slot order per stream instead, in a device
table, and encodes each frame's detections with the reference's per-frame rules (preprocess_perception_main.py:31-36,
then datasets.py:288-324) on the device (opnet_online_encode_f32, csrc/online_encode_kernels.hip):

    ds = DetectorStreams(model, detector=det, capacity=256)       # OPNet, OPNetLstmMlp, BaselineLstm, NonLinearLstm
    ids = ds.open(3)                                              # learned slot orders; or classes=[[140, 3, 7, ...], ...]
    r = ds.step(ids, frames)                  # uint8 BGR [n, k, H, W, 3] -> r.boxes_px int32 [n, k, 4], r.y [n, k, 4],
                                              #   r.logits [n, 15, k] (OPNet models), r.x, r.detections
    r = ds.step_detections(ids, boxes, scores, labels, n_det)     # your own detector's padded device tensors [n, k, md, ...]
    x = ds.encode(ids, boxes, scores, labels, n_det)              # the model input alone [n, k, 15, 5 | 6]

A stream's table row holds 15 class ids (-1 = free) and a mode:
  fixed   : the slot order given at open (datasets.slot_order of a clip already seen, scene metadata ...), never changed;
            ids after the 15th are truncated, as the offline encoder truncates them;
  learned : slot 0 is the snitch's from open; each frame appends its classes not yet in the row, in ascending id order,
            while entries remain.  This equals the offline encoding when the snitch is detected somewhere in the clip and
            every other class of the clip appears in the first frame that has detections.  Otherwise the order is
            first-seen (frame by frame, ascending within a frame), not the clip's ascending order.

Streams may advance by different numbers of frames in one call: `lengths` ([n], 0..k) on encode / step_detections, or a
list of per-stream frame arrays [k_i, H, W, 3] for step.  Frames past a stream's length are padding: they count as frames
without detections for the encoder (nothing is learned from them, they encode as zeros) and never reach the pool's state.

A backlog of many frames can run as one persistent launch instead of the launch chain: `DetectorStreams(..., engine=)` sets the
OPNet pool's default engine (the constructor's `engine=` is served for OPNet only), `step(..., engine=)` /
`step_detections(..., engine=)` choose per call for every pool that has the engine (streaming.OPNetStreams and
streaming.LstmStackStreams; uniform calls only); `verify_launches()` at a sync point, as on the pool.

`encode_detections_numpy` is the readable statement the kernel is held to bit for bit, as encode_boxes is to the native
clip encoder.  step_detections and encode do not synchronise the host: slot ids go up through fresh pinned buffers, and
nothing comes back down.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .datasets import FRAME_SHAPES, MAX_OBJECTS, _cone_table
from .learned_models import BaselineLstm, NonLinearLstm, OPNet, OPNetLstmMlp, _stream_ptr
from .object_indices import SNITCH_INDEX
from .streaming import LstmStackStreams, OPNetStreams, call_entry, check_engine, upload_async

TABLE_INTS = 16                # OPNET_ONLINE_TABLE_INTS: 15 class ids + the mode
MODE_FIXED, MODE_LEARNED = 0, 1
SCORE_THRESHOLD = 0.8          # remove_low_probability_object's default (preprocess_perception_main.py:33)
_CLASS_MAX = 2 ** 31 - 1       # ids outside [0, 2^31 - 1) never enter a table and rank as truncated


def table_row(classes: Optional[Sequence[int]] = None) -> np.ndarray:
    """a fresh table row: learned (None: the snitch in slot 0) or fixed to `classes` (distinct ids, the first 15 kept)"""
    row = np.full(TABLE_INTS, -1, dtype=np.int32)
    if classes is None:
        row[0], row[15] = SNITCH_INDEX, MODE_LEARNED
        return row
    ids = [int(c) for c in classes]
    if any(c < 0 or c >= _CLASS_MAX for c in ids):
        raise ValueError(f"class ids must be in [0, {_CLASS_MAX}), got {ids}")
    if len(set(ids)) != len(ids):
        raise ValueError(f"class ids of a slot order must be distinct, got {ids}")
    ids = ids[:MAX_OBJECTS]
    row[:len(ids)] = ids
    row[15] = MODE_FIXED
    return row


def _kept(scores: np.ndarray, n_det: int, score_thresh: float) -> int:
    """remove_low_probability_object: k = count(scores >= threshold) over the frame's valid rows; the first k are kept"""
    nd = min(max(int(n_det), 0), scores.shape[0])
    return int(np.count_nonzero(scores[:nd] >= np.float32(score_thresh)))


def _valid_class(c: int) -> bool:
    return 0 <= c < _CLASS_MAX


def _valid_n_det(n_det: np.ndarray, lengths) -> np.ndarray:
    """n_det with the padding frames of a ragged call (j >= lengths[i], clamped to [0, k]) counted as empty"""
    if lengths is None:
        return n_det
    n_det = np.array(n_det, copy=True)
    k = n_det.shape[1]
    for i, L in enumerate(np.asarray(lengths).reshape(-1)):
        n_det[i, min(max(int(L), 0), k):] = 0
    return n_det


def learn_tables_numpy(tables: np.ndarray, slots: Sequence[int], scores: np.ndarray, labels: np.ndarray, n_det: np.ndarray,
                       score_thresh: float = SCORE_THRESHOLD, lengths=None) -> None:
    """the learned-table update of one call, in place: tables [capacity, 16] int32, scores [n, k, md], labels [n, k, md],
    n_det [n, k].  Frame by frame, each learned row appends its frame's classes not yet in it, ascending, while entries
    remain; fixed rows are left as they are.  lengths [n] (ragged calls): frames j >= lengths[i] have no detections."""
    n_det = _valid_n_det(n_det, lengths)
    for i, slot in enumerate(slots):
        row = tables[slot]
        if row[15] != MODE_LEARNED:
            continue
        used = next((e for e in range(MAX_OBJECTS) if row[e] == -1), MAX_OBJECTS)
        for j in range(scores.shape[1]):
            if used == MAX_OBJECTS:
                break
            kf = _kept(scores[i, j], n_det[i, j], score_thresh)
            known = set(int(c) for c in row[:used])
            for c in sorted(set(int(c) for c in labels[i, j, :kf] if _valid_class(int(c))) - known)[:MAX_OBJECTS - used]:
                row[used] = c
                used += 1


def encode_frame_numpy(boxes: np.ndarray, labels: np.ndarray, kept: int, row: np.ndarray, cone_mask: np.ndarray,
                       n_tracks: int) -> np.ndarray:
    """one frame's kept detections (boxes [>= kept, 4] fp32 pixels, labels [>= kept]) under the table row -> fp32
    [15, n_tracks] (datasets.py:288-324, as datasets.encode_boxes states them)"""
    out = np.zeros((MAX_OBJECTS, n_tracks), dtype=np.float64)
    if kept == 0:                        # an empty frame is plain zero padding
        return out.astype(np.float32)
    px = boxes[:kept].astype(int)        # preprocess_perception_main.py:35: truncation toward zero
    cls = labels[:kept].astype(np.int64)
    lut = {}
    for e in range(MAX_OBJECTS):
        if row[e] != -1:
            lut.setdefault(int(row[e]), e)
    rank = np.array([lut.get(int(c), MAX_OBJECTS) if _valid_class(int(c)) else MAX_OBJECTS for c in cls], dtype=np.int64)
    cone = np.array([float(cone_mask[c]) if 0 <= c < len(cone_mask) else 0.0 for c in row[:MAX_OBJECTS]])
    if n_tracks == 6:                    # a missing cone keeps its bit only before the frame's last rank
        out[:, 5] = cone * (np.arange(MAX_OBJECTS) < rank.max())
    for s in range(MAX_OBJECTS):
        rows = np.flatnonzero(rank == s)
        if rows.size == 0:
            continue
        r = rows[-1] if row[s] == SNITCH_INDEX else rows[0]     # first occurrence; the last one for the snitch
        out[s, :4] = px[r]
        out[s, 4] = 1.0
        if n_tracks == 6:
            out[s, 5] = cone[s]
    out[:, :4] /= FRAME_SHAPES
    return out.astype(np.float32)


def encode_detections_numpy(boxes: np.ndarray, scores: np.ndarray, labels: np.ndarray, n_det: np.ndarray,
                            slots: Sequence[int], tables: np.ndarray, cone_mask: np.ndarray, n_tracks: int,
                            score_thresh: float = SCORE_THRESHOLD, lengths=None) -> np.ndarray:
    """The statement of opnet_online_encode_f32: padded detections of n streams x k frames (boxes [n, k, md, 4] fp32,
    scores [n, k, md] fp32, labels [n, k, md] int64, n_det [n, k]) and the streams' table rows tables[slots[i]] -> fp32
    [n, k, 15, n_tracks].  Learned rows of `tables` are updated in place first (learn_tables_numpy).  lengths [n]
    (opnet_online_encode_ragged_f32): frames j >= lengths[i] count as n_det = 0, so they learn nothing and encode as zeros."""
    if n_tracks not in (5, 6):
        raise ValueError(f"n_tracks must be 5 or 6, got {n_tracks}")
    n_det = _valid_n_det(n_det, lengths)
    learn_tables_numpy(tables, slots, scores, labels, n_det, score_thresh)
    n, k = scores.shape[:2]
    out = np.zeros((n, k, MAX_OBJECTS, n_tracks), dtype=np.float32)
    for i, slot in enumerate(slots):
        for j in range(k):
            out[i, j] = encode_frame_numpy(boxes[i, j], labels[i, j], _kept(scores[i, j], n_det[i, j], score_thresh),
                                           tables[slot], cone_mask, n_tracks)
    return out


class StreamResult(NamedTuple):
    boxes_px: torch.Tensor                  # int32 [n, k, 4]: the snitch box in pixels (opnet_postprocess_iou of y)
    y: torch.Tensor                         # fp32 [n, k, 4]
    logits: Optional[torch.Tensor]          # fp32 [n, 15, k] (OPNet and OPNetLstmMlp), else None
    x: torch.Tensor                         # the encoded model input [n, k, 15, n_tracks]
    detections: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]   # (boxes, scores, labels, n_det)
    lengths: Optional[torch.Tensor] = None  # int32 [n] frames per stream of a ragged call (boxes_px, y, logits, x are 0
                                            #   past them); None: every stream advanced by k


class DetectorStreams:
    """A detector, a stream pool of `capacity` streams of `model` on its ROCm device and one slot-order table row per
    stream.  Calls are enqueued on the current torch stream and are inference only."""

    def __init__(self, model, detector=None, capacity: int = 1024, score_thresh: float = SCORE_THRESHOLD,
                 n_tracks: Optional[int] = None, engine: str = "chain"):
        if isinstance(model, (OPNet, OPNetLstmMlp)):
            pool, tracks = OPNetStreams(model, capacity, engine=engine), 6
        elif isinstance(model, (BaselineLstm, NonLinearLstm)):
            if check_engine(engine) != "chain":
                raise ValueError(f"engine={engine!r} as a pool default is served for OPNet only: {type(model).__name__} "
                                 "streams (LstmStackStreams) take engine='persistent' per call, step(..., engine=)")
            pool, tracks = LstmStackStreams(model, capacity), 5
        else:
            raise TypeError(f"DetectorStreams serves OPNet, OPNetLstmMlp, BaselineLstm and NonLinearLstm, not "
                            f"{type(model).__name__} (transformer_lstm is not streamed: its encoder attends over the whole "
                            "sequence)")
        if n_tracks is not None and int(n_tracks) != tracks:
            raise ValueError(f"{type(model).__name__} takes {tracks} tracks per slot, not {n_tracks}")
        self.model, self.detector, self.pool = model, detector, pool
        self.device, self.capacity, self.n_tracks = pool.device, pool.capacity, tracks
        self.score_thresh = float(score_thresh)
        with torch.cuda.device(self.device):
            self.tables = torch.from_numpy(np.tile(table_row([]), (self.capacity, 1))).to(self.device)
            self.cone_mask = torch.from_numpy(_cone_table()).to(self.device)

    # -- slots --------------------------------------------------------------------------------
    @property
    def free(self) -> int:
        return self.pool.free

    def open(self, count: int = 1, classes: Optional[Sequence[Sequence[int]]] = None) -> List[int]:
        """`count` new streams with a zero state and a fresh table row: learned (classes None) or one fixed slot order per
        stream (a list of distinct class ids each; longer than 15 is truncated, as the offline encoder does)"""
        count = int(count)
        if classes is None:
            rows = np.tile(table_row(None), (max(count, 0), 1))
        else:
            if len(classes) != count:
                raise ValueError(f"classes must hold one slot order per stream: {count} streams, {len(classes)} orders")
            rows = np.stack([table_row(c) for c in classes]) if count > 0 else None
        ids = self.pool.open(count)
        with torch.cuda.device(self.device):
            self.tables.index_copy_(0, torch.tensor(ids, dtype=torch.int64).to(self.device),
                                    torch.from_numpy(rows).to(self.device))
        return ids

    def close(self, ids: Sequence[int]) -> None:
        self.pool.close(ids)

    def get_state(self, ids: Sequence[int]):
        return self.pool.get_state(ids)

    def set_state(self, ids: Sequence[int], *state) -> None:
        self.pool.set_state(ids, *state)

    def get_slot_classes(self, ids: Sequence[int]) -> torch.Tensor:
        """int32 [n, 15]: the class id of each slot of the streams (-1 = free); a copy on the device"""
        idx = self.pool.slots.check(ids)
        with torch.cuda.device(self.device):
            return self.tables.index_select(0, torch.from_numpy(idx).to(self.device))[:, :MAX_OBJECTS].contiguous()

    # -- encoding -----------------------------------------------------------------------------
    def _upload(self, a: np.ndarray) -> torch.Tensor:
        """a host array on the device without a host sync (streaming.upload_async)"""
        return upload_async(a, self.device)

    def _check_detections(self, ids, boxes, scores, labels, n_det):
        for t, name, dt in ((boxes, "boxes", torch.float32), (scores, "scores", torch.float32),
                            (labels, "labels", torch.int64), (n_det, "n_det", torch.int32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"DetectorStreams runs on MI355X only: `{name}` must be a tensor on a ROCm device")
            if t.device != self.device:
                raise ValueError(f"{name} is on {t.device}, the streams on {self.device}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
        idx = self.pool.slots.check(ids)
        n = idx.size
        if boxes.dim() != 4 or boxes.shape[0] != n or boxes.shape[1] < 1 or boxes.shape[2] < 1 or boxes.shape[3] != 4:
            raise ValueError(f"boxes must be [n={n}, k>=1, md>=1, 4], got {tuple(boxes.shape)}")
        k, md = int(boxes.shape[1]), int(boxes.shape[2])
        if tuple(scores.shape) != (n, k, md) or tuple(labels.shape) != (n, k, md):
            raise ValueError(f"scores and labels must be [{n}, {k}, {md}], got {tuple(scores.shape)} and {tuple(labels.shape)}")
        if tuple(n_det.shape) != (n, k):
            raise ValueError(f"n_det must be [{n}, {k}], got {tuple(n_det.shape)}")
        return idx, k, md

    def _encode_into(self, out: torch.Tensor, slots: torch.Tensor, boxes, scores, labels, n_det,
                     lengths: Optional[torch.Tensor] = None) -> None:
        n, k, md = int(boxes.shape[0]), int(boxes.shape[1]), int(boxes.shape[2])
        boxes, scores, labels, n_det = (t.contiguous() for t in (boxes, scores, labels, n_det))
        assert out.is_contiguous() and tuple(out.shape) == (n, k, MAX_OBJECTS, self.n_tracks)
        call_entry("opnet_online_encode_f32",
                   [boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), n_det.data_ptr(), md, slots.data_ptr(),
                    self.tables.data_ptr(), self.capacity, self.cone_mask.data_ptr(), int(self.cone_mask.numel()), n, k,
                    self.n_tracks, self.score_thresh, out.data_ptr(), _stream_ptr(self.device)], lengths, 4)

    def _encode(self, ids, boxes, scores, labels, n_det, lengths=None):
        idx, k, md = self._check_detections(ids, boxes, scores, labels, n_det)
        with torch.no_grad(), torch.cuda.device(self.device):
            if lengths is None:      # a pinned copy, unlike the pool's uniform route: encode never syncs the host
                slots, lens = self._upload(idx.astype(np.int32)), None
            else:
                slots, lens = self.pool._device_ids(idx, lengths, k)
            x = torch.empty((idx.size, k, MAX_OBJECTS, self.n_tracks), dtype=torch.float32, device=self.device)
            self._encode_into(x, slots, boxes, scores, labels, n_det, lens)
        return slots, lens, x

    def encode(self, ids: Sequence[int], boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor,
               n_det: torch.Tensor, lengths=None) -> torch.Tensor:
        """the model input of k frames of detections (boxes [n, k, md, 4] fp32 pixels, scores [n, k, md] fp32, labels
        [n, k, md] int64, n_det [n, k] int32, padded as RoIHeads writes them) -> [n, k, 15, n_tracks].  Learned slot orders
        are updated; the streams' states are not advanced.  lengths ([n] in 0..k, host or int32 device): frames past a
        stream's length are padding, learn nothing and encode as zeros.  No host sync."""
        return self._encode(ids, boxes, scores, labels, n_det, lengths)[2]

    # -- frames -------------------------------------------------------------------------------
    def verify_launches(self) -> int:
        """as the pool's verify_launches: wait for the model's persistent launches, heal a step that gave up"""
        return self.pool.verify_launches()

    def _check_engine(self, engine, lengths) -> None:
        """before anything is encoded: an engine the pool refuses must not leave the slot tables half updated"""
        self.pool._check_engine(engine, lengths)

    def _advance(self, slots: torch.Tensor, x: torch.Tensor, detections,
                 lengths: Optional[torch.Tensor] = None, engine: Optional[str] = None) -> StreamResult:
        n, k = int(x.shape[0]), int(x.shape[1])
        with torch.no_grad(), torch.cuda.device(self.device):
            out = self.pool._step_slots(slots, x, lengths, engine=engine)
            y, logits = out if isinstance(out, tuple) else (out, None)
            px = torch.empty((n, k, 4), dtype=torch.int32, device=self.device)

            def pixels():
                with torch.cuda.device(self.device):
                    rc = _lib.load().opnet_postprocess_iou(y.data_ptr(), None, px.data_ptr(), None, None, n, k,
                                                           _stream_ptr(self.device))
                _lib.check(rc, "opnet_postprocess_iou")
            pixels()
            # y of an unverified persistent step (and of every step behind it) may still be rewritten by the pool's replay:
            # the pixel boxes are then derived again, into the px the caller holds
            self.pool.log_followup(pixels)
        return StreamResult(px, y, logits, x, detections, lengths)

    def step_detections(self, ids: Sequence[int], boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor,
                        n_det: torch.Tensor, lengths=None, engine: Optional[str] = None) -> StreamResult:
        """encode k frames of detections of your own detector (as `encode`) and advance the streams by them (stream i by
        its first lengths[i] when lengths are given).  engine: "chain" or "persistent" (uniform calls) for this
        call, None = the pool's default.  No host sync."""
        self._check_engine(engine, lengths)
        slots, lens, x = self._encode(ids, boxes, scores, labels, n_det, lengths)
        return self._advance(slots, x, (boxes, scores, labels, n_det), lens, engine)

    def step(self, ids: Sequence[int], frames, engine: Optional[str] = None) -> StreamResult:
        """k frames per stream through the detector, the encoder and the pool: frames uint8 BGR [n, k, H, W, 3] (row i
        belongs to ids[i]; one shape for all).  The detector runs in passes of at most MAX_FRAMES_PER_PASS frames in
        stream-major order (whole streams per pass when k allows it), the encoder once per pass into its slice of x.
        r.detections holds the padded detections used, [n, k, md, ...].

        frames may also be a list of n per-stream arrays uint8 [k_i, H, W, 3] (k_i >= 0, one H, W): the detector then runs
        on the sum(k_i) real frames only, in passes of at most MAX_FRAMES_PER_PASS, their detections are scattered into
        [n, K = max k_i, md, ...] with n_det = 0 on padding, and the encoder and the pool run once with the lengths k_i
        (r.lengths)."""
        if self.detector is None:
            raise RuntimeError("DetectorStreams.step needs a detector: DetectorStreams(model, detector=...)")
        if isinstance(frames, (list, tuple)):
            self._check_engine(engine, frames)
            return self._step_ragged(ids, frames, engine)
        self._check_engine(engine, None)
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[4] != 3 or frames.shape[1] < 1:
            raise ValueError(f"frames must be uint8 [n, k>=1, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
        idx = self.pool.slots.check(ids)
        n, k = idx.size, int(frames.shape[1])
        if frames.shape[0] != n:
            raise ValueError(f"frames hold {frames.shape[0]} streams, ids {n}")
        P = int(self.detector.MAX_FRAMES_PER_PASS)
        if k <= P:       # whole streams per pass
            m = P // k
            passes = [(i, min(n, i + m), 0, k) for i in range(0, n, m)]
        else:            # one stream's frames in chunks
            passes = [(i, i + 1, j, min(k, j + P)) for i in range(n) for j in range(0, k, P)]
        parts = []
        with torch.no_grad(), torch.cuda.device(self.device):
            slots = self._upload(idx.astype(np.int32))
            x = torch.empty((n, k, MAX_OBJECTS, self.n_tracks), dtype=torch.float32, device=self.device)
            for i0, i1, j0, j1 in passes:
                b, s, l, nd = self.detector._enqueue_padded([frames[i, j] for i in range(i0, i1) for j in range(j0, j1)],
                                                            self.device)
                md = int(b.shape[1])
                shape = (i1 - i0, j1 - j0)
                self._encode_into(x[i0:i1, j0:j1], slots[i0:i1], b.view(*shape, md, 4), s.view(*shape, md),
                                  l.view(*shape, md), nd.view(*shape))
                parts.append((b, s, l, nd))
            det = tuple(torch.cat([p[q] for p in parts]).view(n, k, *parts[0][q].shape[1:]) for q in range(4))
        return self._advance(slots, x, det, None, engine)

    def _step_ragged(self, ids: Sequence[int], frames, engine: Optional[str] = None) -> StreamResult:
        idx = self.pool.slots.check(ids)
        n = idx.size
        if len(frames) != n:
            raise ValueError(f"frames hold {len(frames)} streams, ids {n}")
        arrays = [np.asarray(f) for f in frames]
        for f in arrays:
            if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3:
                raise ValueError(f"each stream's frames must be uint8 [k_i, H, W, 3], got {f.dtype} {tuple(f.shape)}")
        if len({f.shape[1:] for f in arrays if f.shape[0] > 0}) > 1:
            raise ValueError("the frames of one call must share one H, W")
        ks = np.array([f.shape[0] for f in arrays], dtype=np.int32)
        K = int(ks.max())
        if K < 1:
            raise ValueError("a ragged step needs at least one frame")
        # the real frames, stream-major, and the padded row (i * K + j) each one lands in
        flat = [f[j] for f in arrays for j in range(f.shape[0])]
        dest = np.concatenate([i * K + np.arange(k, dtype=np.int64) for i, k in enumerate(ks)])
        P = int(self.detector.MAX_FRAMES_PER_PASS)
        parts = []
        with torch.no_grad(), torch.cuda.device(self.device):
            slots, lens = self.pool._device_ids(idx, ks, K)
            rows = self._upload(dest)
            for p0 in range(0, len(flat), P):
                parts.append(self.detector._enqueue_padded(flat[p0:p0 + P], self.device))
            md = int(parts[0][0].shape[1])
            if any(int(p[0].shape[1]) != md for p in parts):
                raise RuntimeError("the detector's passes disagree on the padded detection count")
            det = []
            for q in range(4):
                src = torch.cat([p[q] for p in parts])
                out = torch.zeros((n * K,) + tuple(src.shape[1:]), dtype=src.dtype, device=self.device)
                out.index_copy_(0, rows, src)
                det.append(out.view((n, K) + tuple(src.shape[1:])))
            boxes, scores, labels, n_det = det
            x = torch.empty((n, K, MAX_OBJECTS, self.n_tracks), dtype=torch.float32, device=self.device)
            self._encode_into(x, slots, boxes, scores, labels, n_det, lens)
        return self._advance(slots, x, (boxes, scores, labels, n_det), lens, engine)
