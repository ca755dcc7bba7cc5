"""CPU checks of the per-frame encoder of DetectorStreams (objectpermanence_amd/detector_streams.py): its numpy statement
against the offline encoder and the reference goldens (tests/golden/datasets.npz), the score cut and integer cast against
CaterObjectDetector.remove_low_probability_object + astype(int), the learned slot orders, and the C ABI's refusals
(nothing is launched)."""
import os

import numpy as np
import pytest
import torch

from oracle import synth

VARIANTS = ["plain", "dups", "crowded", "nosnitch0", "sparse"]
FS = np.array([320, 240, 320, 240], dtype=np.float64)


def _cone():
    from objectpermanence_amd.datasets import _cone_table
    return _cone_table()


def pad_clip(bb, lab, rng, extra=2, md=None):
    """a clip's per-frame detections as the detector's padded outputs: the frame's rows (scores >= 0.8), then `extra`
    sub-threshold rows inside n_det, then zero rows -> boxes [T, md, 4] fp32, scores [T, md], labels [T, md], n_det [T]"""
    T = len(lab)
    md = md or max(len(l) for l in lab) + extra + 1
    boxes = np.zeros((T, md, 4), np.float32)
    scores = np.zeros((T, md), np.float32)
    labels = np.zeros((T, md), np.int64)
    n_det = np.zeros(T, np.int32)
    for t in range(T):
        m = len(lab[t])
        e = min(extra, md - m)
        boxes[t, :m] = np.asarray(bb[t]).reshape(-1, 4)
        scores[t, :m] = np.sort(rng.uniform(0.8, 1.0, m))[::-1]
        labels[t, :m] = lab[t]
        boxes[t, m:m + e] = rng.integers(0, 200, size=(e, 4))
        scores[t, m:m + e] = rng.uniform(0.05, 0.79, e)
        labels[t, m:m + e] = rng.integers(1, 193, e)
        n_det[t] = m + e
    return boxes, scores, labels, n_det


def _tables(rows, capacity=8):
    from objectpermanence_amd.detector_streams import table_row
    t = np.tile(table_row([]), (capacity, 1))
    for slot, r in rows.items():
        t[slot] = r
    return t


def _run_chunks(det, slot, tables, chunks, n_tracks):
    """the statement over one stream's frames, k frames per call"""
    from objectpermanence_amd.detector_streams import encode_detections_numpy
    boxes, scores, labels, n_det = det
    out, t = [], 0
    for k in chunks:
        out.append(encode_detections_numpy(boxes[None, t:t + k], scores[None, t:t + k], labels[None, t:t + k],
                                           n_det[None, t:t + k], [slot], tables, _cone(), n_tracks)[0])
        t += k
    assert t == len(n_det)
    return np.concatenate(out)


@pytest.mark.parametrize("n_tracks", [6, 5])
@pytest.mark.parametrize("vi", range(len(VARIANTS)))
def test_fixed_mode_equals_offline_encoder_and_goldens(golden_dir, vi, n_tracks):
    from objectpermanence_amd.datasets import encode_boxes, slot_order
    from objectpermanence_amd.detector_streams import table_row
    g = np.load(os.path.join(golden_dir, "datasets.npz"))
    bb, lab, _ = synth.make_raw_video(vi, VARIANTS[vi])
    det = pad_clip(bb, lab, np.random.default_rng(vi))
    tables = _tables({3: table_row(slot_order(lab))})
    before = tables.copy()
    got = _run_chunks(det, 3, tables, [1] * len(lab), n_tracks)
    assert np.array_equal(tables, before)                               # a fixed row is never written
    assert got.dtype == np.float32 and got.shape == (300, 15, n_tracks)
    assert np.array_equal(got, encode_boxes(bb, lab, n_tracks).astype(np.float32))
    assert np.array_equal(got, g[f"t{n_tracks}/{vi}/boxes"])


def test_score_cut_and_cast_equal_remove_low_probability_object():
    from objectpermanence_amd.datasets import encode_boxes, slot_order
    from objectpermanence_amd.detector import CaterObjectDetector
    from objectpermanence_amd.detector_streams import _kept, encode_frame_numpy, table_row
    t8 = np.float32(0.8)
    edge = [t8, np.nextafter(t8, np.float32(1)), np.nextafter(t8, np.float32(0))]
    rng = np.random.default_rng(7)
    md, cut_inside = 12, 0
    for f in range(200):
        nd = int(rng.integers(0, md + 1))
        scores = rng.choice(np.array(edge + [0.95, 0.5, 0.85, 0.3], np.float32), size=md).astype(np.float32)
        scores[nd:] = 1.0                                        # rows past n_det never count, whatever they hold
        boxes = rng.uniform(-0.9, 319.9, size=(md, 4)).astype(np.float32)
        boxes[:, 0] = np.where(rng.random(md) < 0.2, np.float32(-0.5), boxes[:, 0])
        labels = rng.choice(np.array([140, 0, 4, 65, 70, 98, 3, 12]), size=md).astype(np.int64)
        ref = CaterObjectDetector.remove_low_probability_object(
            {"boxes": torch.from_numpy(boxes[:nd]), "labels": torch.from_numpy(labels[:nd]), "scores": torch.from_numpy(scores[:nd])})
        kept = _kept(scores, nd, 0.8)
        assert kept == ref["scores"].shape[0]
        cut_inside += int(kept < nd and np.any(scores[:kept] < t8))     # a row under the threshold kept by the prefix
        px, lb = ref["boxes"].numpy().astype(int), ref["labels"].numpy()
        for n_tracks in (6, 5):
            want = encode_boxes([px], [lb], n_tracks).astype(np.float32)[0]
            got = encode_frame_numpy(boxes, labels, kept, table_row(slot_order([lb])), _cone(), n_tracks)
            assert np.array_equal(got, want)
    assert cut_inside > 0


def _with_union_first_frame(bb, lab, rng):
    """the clip with its first frame replaced by one detection of every non-snitch class of the clip (shuffled), so the
    learned order's condition holds"""
    ids = sorted(set(int(c) for l in lab for c in l) - {140})
    ids = [ids[i] for i in rng.permutation(len(ids))]
    lab = [np.array(ids, np.int64)] + list(lab[1:])
    bb = [rng.integers(0, 200, size=(len(ids), 4)).astype(np.int64)] + list(bb[1:])
    return bb, lab


@pytest.mark.parametrize("variant", ["plain", "crowded", "dups"])
@pytest.mark.parametrize("chunks", [[1] * 300, [7] * 42 + [6], [300]])
def test_learned_mode_equals_offline_encoder_when_the_condition_holds(variant, chunks):
    from objectpermanence_amd.datasets import encode_boxes, slot_order
    from objectpermanence_amd.detector_streams import table_row
    rng = np.random.default_rng(3)
    bb, lab, _ = synth.make_raw_video(20, variant)
    bb, lab = _with_union_first_frame(bb, lab, rng)
    assert any(140 in l for l in lab)
    tables = _tables({5: table_row(None)})
    got = _run_chunks(pad_clip(bb, lab, rng), 5, tables, chunks, 6)
    assert np.array_equal(got, encode_boxes(bb, lab, 6).astype(np.float32))
    order = slot_order(lab)[:15]
    assert tables[5, :len(order)].tolist() == order and tables[5, 15] == 1


def test_learned_mode_is_first_seen_when_a_lower_id_comes_later():
    from objectpermanence_amd.datasets import encode_boxes
    from objectpermanence_amd.detector_streams import table_row
    A, B, C, D, E, F, G, H, I = ([10 * i, 10 * i + 1, 10 * i + 30, 10 * i + 40] for i in range(1, 10))
    # 20 is a cone, 50, 7 and 3 are not; the snitch repeats in the last frame
    lab = [np.array([50, 140, 20]), np.array([7, 50]), np.array([3, 7, 140, 140])]
    bb = [np.array([A, B, C]), np.array([D, E]), np.array([F, G, H, I])]
    tables = _tables({0: table_row(None)})
    got = _run_chunks(pad_clip(bb, lab, np.random.default_rng(0)), 0, tables, [1, 2], 6)
    assert tables[0].tolist() == [140, 20, 50, 7, 3] + [-1] * 10 + [1]
    box = lambda b, cone: np.array(list(np.array(b, np.float64) / FS) + [1, cone], dtype=np.float32)
    want = np.zeros((3, 15, 6), np.float32)
    want[0, 0], want[0, 1], want[0, 2] = box(B, 0), box(C, 1), box(A, 0)
    want[1, 2], want[1, 3] = box(E, 0), box(D, 0)
    want[1, 1, 5] = 1                                   # the missing cone before the frame's last rank (3)
    want[2, 0], want[2, 3], want[2, 4] = box(I, 0), box(G, 0), box(F, 0)     # the LAST snitch
    want[2, 1, 5] = 1
    assert np.array_equal(got, want)
    assert not np.array_equal(got, encode_boxes(bb, lab, 6).astype(np.float32))   # the clip's order would be 140, 3, 7, 20, 50


def test_learned_table_is_full_after_15_entries():
    from objectpermanence_amd.detector_streams import table_row
    rng = np.random.default_rng(1)
    first = [140, 0, 4, 8, 12, 16, 30, 31, 33, 35, 37, 39, 41, 43, 45, 47, 49]      # 17 classes
    lab = [np.array(first)[rng.permutation(17)], np.array([1, 2, 47, 0]), np.array([2, 8])]
    bb = [rng.integers(0, 200, size=(len(l), 4)) for l in lab]
    tables = _tables({1: table_row(None)})
    got = _run_chunks(pad_clip(bb, lab, rng), 1, tables, [1, 1, 1], 6)
    assert tables[1, :15].tolist() == [140] + sorted(first[1:])[:14]
    # frame 1: ids 1 and 2 are not in the full table, so they rank 15: every missing cone slot keeps its bit
    cone = np.array([float(_cone()[c]) for c in tables[1, :15]])
    assert np.array_equal(got[1, :, 5], np.maximum(cone, got[1, :, 4] * cone))
    assert 47 not in tables[1] and got[1, 1, 4] == 1 and got[1, :, 4].sum() == 1     # 0 only: 47 was the 16th class
    assert got[2, 3, 4] == 1 and got[2, :, 4].sum() == 1   # 8 only


def test_c_abi_refusals_without_gpu():
    from objectpermanence_amd import _lib, build
    build.build()
    lib = _lib.load()
    f = lib.opnet_online_encode_f32
    ok = dict(b=4096, s=4096, l=4096, nd=4096, md=10, slots=4096, tab=4096, cap=4, cone=4096, nc=193, n=1, k=1, nt=6, out=4096)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["b"], a["s"], a["l"], a["nd"], a["md"], a["slots"], a["tab"], a["cap"], a["cone"], a["nc"], a["n"], a["k"],
                 a["nt"], 0.8, a["out"], None)
    # every call below fails its checks before anything is enqueued
    assert call(b=None, nt=7) == -1 and call(tab=None, nt=7) == -1 and call(out=None, nt=7) == -1
    assert call(b=4100, nt=7) == -1 and call(tab=4104, nt=7) == -1 and call(l=4100, nt=7) == -1
    assert call(nt=7) == -2 and call(nt=4) == -2
    assert call(n=0) == -2 and call(k=0) == -2 and call(md=0) == -2 and call(cap=0) == -2 and call(nc=0) == -2
    assert b"must be positive" in lib.opnet_last_error()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opnet_hip.h")).read()
    assert "#define OPNET_ONLINE_TABLE_INTS 16" in hdr
    from objectpermanence_amd.detector_streams import TABLE_INTS
    assert TABLE_INTS == 16


def test_table_rows_refuse_bad_slot_orders():
    from objectpermanence_amd.detector_streams import table_row
    assert table_row(None).tolist() == [140] + [-1] * 14 + [1]
    assert table_row(list(range(20))).tolist() == list(range(15)) + [0]
    with pytest.raises(ValueError):
        table_row([3, 3])
    with pytest.raises(ValueError):
        table_row([-1])
