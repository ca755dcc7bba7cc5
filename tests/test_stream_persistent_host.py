"""CPU-side checks of the persistent engine of the OPNet streams (include/opnet_hip.h opnet_stream_x4_*,
objectpermanence_amd/streaming.py): size queries, argument refusals before anything is launched, `engine` validation, and
the undo / redo log (StreamReplayLog) against a toy pool in numpy."""
import numpy as np
import pytest
import torch


def _lib():
    from objectpermanence_amd import _lib, build
    build.build()
    return _lib.load()


def test_x4_stream_size_queries():
    lib = _lib()
    assert lib.opnet_stream_x4_max_streams() == lib.opnet_xcd4_max_batch() == 128
    w = lib.opnet_stream_x4_workspace_bytes(1, 1, 256, 512)
    assert w > 0
    assert lib.opnet_stream_x4_workspace_bytes(1, 8, 256, 512) > w           # grows with k
    assert lib.opnet_stream_x4_workspace_bytes(33, 1, 256, 512) > w          # and with n (a second row block)
    assert lib.opnet_stream_x4_workspace_bytes(128, 300, 256, 512) > lib.opnet_stream_x4_workspace_bytes(32, 300, 256, 512)
    for n, k in ((1, 1), (5, 7), (70, 300), (128, 300)):
        # the whole-clip entry's workspace is not moved by this feature; the stream step's is that plus the cell-state
        # staging (4 clips x (H1 + H2) floats per group of 8 per row block), and the status words stay where they were
        base = lib.opnet_xcd4_workspace_bytes(n, k, 256, 512)
        groups = (n + 31) // 32 * 8
        assert lib.opnet_stream_x4_workspace_bytes(n, k, 256, 512) == base + groups * 4 * (256 + 512) * 4
        assert lib.opnet_stream_x4_status_offset(n, k, 256, 512) == lib.opnet_xcd4_status_offset(n, k, 256, 512)
        assert lib.opnet_stream_x4_status_offset(n, k, 256, 512) + 16 <= base


def test_x4_stream_shapes_not_served():
    from objectpermanence_amd import _lib as L
    lib = _lib()
    assert lib.opnet_stream_x4_workspace_bytes(1, 1, 16, 32) == 0
    assert b"H1=256" in lib.opnet_last_error()
    assert lib.opnet_stream_x4_status_offset(1, 1, 16, 32) == L.NO_OFFSET
    assert lib.opnet_stream_x4_workspace_bytes(129, 1, 256, 512) == 0
    assert b"129" in lib.opnet_last_error()
    assert lib.opnet_stream_x4_workspace_bytes(1, 0, 256, 512) == 0
    assert b"positive" in lib.opnet_last_error()
    assert lib.opnet_stream_x4_workspace_bytes(0, 1, 256, 512) == 0
    # beyond the 2 GiB one buffer descriptor addresses
    assert lib.opnet_stream_x4_workspace_bytes(128, 100000, 256, 512) == 0
    assert b"2 GiB" in lib.opnet_last_error()
    assert lib.opnet_stream_x4_workspace_bytes(128, 300, 256, 512) < 2 ** 31


def test_x4_stream_step_refuses_bad_arguments():
    lib = _lib()
    # boxes, slots, state, x4packed, y, logits, workspace, bytes, n, k, capacity, H1, H2, stream
    step = lib.opnet_stream_step_x4_f32
    assert step(None, None, None, None, None, None, None, 0, 1, 1, 4, 256, 512, None) == -1
    assert b"null" in lib.opnet_last_error()
    assert step(None, None, None, None, None, None, None, 0, 1, 1, 4, 16, 32, None) == -2
    assert step(None, None, None, None, None, None, None, 0, 129, 1, 256, 256, 512, None) == -2
    assert step(None, None, None, None, None, None, None, 0, 1, 0, 4, 256, 512, None) == -2
    assert step(None, None, None, None, None, None, None, 0, 1, 1, 0, 256, 512, None) == -2
    assert b"capacity" in lib.opnet_last_error()
    p = 1 << 20       # fake, 16-byte aligned addresses: refused before any launch
    assert step(p, p, p, p, p, p, p + 4, 1 << 30, 1, 1, 4, 256, 512, None) == -1
    assert b"aligned" in lib.opnet_last_error()
    assert step(p, p + 2, p, p, p, p, p, 1 << 30, 1, 1, 4, 256, 512, None) == -1
    assert step(p, p, p, p, p, p, p, 64, 1, 1, 4, 256, 512, None) == -3
    assert b"workspace" in lib.opnet_last_error()
    need = lib.opnet_stream_x4_workspace_bytes(5, 7, 256, 512)
    assert step(p, p, p, p, p, p, p, need - 1, 5, 7, 8, 256, 512, None) == -3


def test_engine_validation():
    from objectpermanence_amd import DetectorStreams, ModelsFactory, OPNetStreams
    from objectpermanence_amd.streaming import ENGINES, check_engine
    assert ENGINES == ("chain", "persistent")
    assert check_engine("chain") == "chain" and check_engine("persistent") == "persistent"
    assert check_engine(None, "persistent") == "persistent"
    with pytest.raises(ValueError, match="no automatic choice"):
        check_engine("auto")
    with pytest.raises(TypeError):
        check_engine(None)
    with pytest.raises(TypeError):
        check_engine(1)
    cfg = {"object_to_track_pred_dim": 15, "object_to_track_hidden_dim": 16, "videos_hidden_dim": 32}
    # the engine is looked at first: a bad one is refused even where the pool itself would be (a CPU model)
    with pytest.raises(ValueError, match="engine"):
        OPNetStreams(ModelsFactory.get_model("opnet", cfg), capacity=4, engine="auto")
    with pytest.raises(TypeError, match="OPNet only"):
        OPNetStreams(ModelsFactory.get_model("opnet_lstm_mlp", cfg), capacity=4, engine="persistent")
    with pytest.raises(ValueError, match="OPNet only"):
        DetectorStreams(ModelsFactory.get_model("baseline_lstm", {"videos_hidden_dim": 32}), capacity=4, engine="persistent")
    # the default engine is the chain, and a CPU model is refused as before
    with pytest.raises(RuntimeError, match="ROCm device"):
        OPNetStreams(ModelsFactory.get_model("opnet", cfg), capacity=4, engine="chain")


def test_launch_monitor_watching():
    from objectpermanence_amd.launch_monitor import LaunchMonitor

    class Ev:
        def query(self):
            return True

        def synchronize(self):
            pass

    mon = LaunchMonitor()
    mon._host = torch.zeros((64, 4), dtype=torch.int32)
    a, b = (lambda: None), (lambda: None)
    mon._pending.append((Ev(), mon._free.pop(), a, "a"))
    assert mon.watching(a) and not mon.watching(b)
    assert mon.reap() == 1 and not mon.watching(a)


# ---- the undo / redo log against a toy pool -------------------------------------------------------------------------------
CALLS = [([0, 1, 2], 1.0), ([2, 3], 2.0), ([1, 4], 3.0), ([0, 2, 4], 4.0), ([3, 1], 5.0)]    # overlapping slot sets


class ToyPool:
    """state[slots] = 0.5 * state[slots] + x.sum() is the "step" (it does not commute with itself, so order matters); y = the
    new rows.  A call that "gives up" leaves its rows alone and returns NaN, as opnet_stream_x4_writeback does."""

    def __init__(self):
        from objectpermanence_amd.streaming import StreamReplayLog
        self.state = np.arange(5, dtype=np.float64)
        self.log = StreamReplayLog(self.restore, self.rerun)
        self.reran = []

    def restore(self, slots, before):
        self.state[slots] = before

    def compute(self, slots, x, y):
        self.state[slots] = 0.5 * self.state[slots] + x.sum()
        y[:] = self.state[slots]

    def rerun(self, payload):
        slots, x, y = payload
        self.reran.append(float(x[0]))
        self.compute(slots, x, y)

    def step(self, slots, x, give_up=False):
        slots, x = np.asarray(slots), np.asarray([x, 0.0])
        y = np.empty(len(slots))
        entry = self.log.record(slots, self.state[slots].copy(), (slots, x, y))
        entry.redo = lambda: None          # a watched launch
        if give_up:
            y[:] = np.nan
        else:
            self.compute(slots, x, y)
        return y, entry


def _clean():
    pool = ToyPool()
    ys = [pool.step(s, x)[0] for s, x in CALLS]
    return pool.state.copy(), ys


@pytest.mark.parametrize("bad", range(len(CALLS)))
def test_replay_heals_an_abort_at_any_position(bad):
    state_ref, ys_ref = _clean()
    pool = ToyPool()
    out = [pool.step(s, x, give_up=(i == bad)) for i, (s, x) in enumerate(CALLS)]
    ys, entries = [o[0] for o in out], [o[1] for o in out]
    assert np.isnan(ys[bad]).all()
    if bad < len(CALLS) - 1:
        assert not np.array_equal(pool.state, state_ref)
    assert pool.log.replay(entries[bad]) == len(CALLS) - bad
    assert pool.reran == [x for _, x in CALLS[bad:]]              # that call and every later one, in order
    assert np.array_equal(pool.state, state_ref)
    for y, y_ref in zip(ys, ys_ref):                              # healed in place: the arrays the caller holds
        assert np.array_equal(y, y_ref)
    # a later entry of the same log was run again already: its own redo must not run anything twice
    assert all(e.healed for e in entries[bad:]) and not any(e.healed for e in entries[:bad])
    assert pool.log.replay(entries[-1]) == 0
    assert np.array_equal(pool.state, state_ref)


def test_log_prunes_to_the_oldest_unverified_launch_and_empties_after_a_clean_verify():
    pool = ToyPool()
    entries = [pool.step(s, x)[1] for s, x in CALLS]
    entries[1].redo = entries[3].redo = None                      # chain calls between persistent ones
    unverified = {id(entries[2]), id(entries[4])}
    pool.log.prune(lambda e: id(e) in unverified)
    assert pool.log.entries == entries[2:]                        # calls 0, 1 can no longer be rewound to
    unverified.discard(id(entries[2]))
    pool.log.prune(lambda e: id(e) in unverified)
    assert pool.log.entries == entries[4:]
    pool.log.prune(lambda e: False)                               # a clean verify: nothing is watched any more
    assert len(pool.log) == 0
    assert pool.log.replay(entries[4]) == 0 and pool.reran == []  # a pruned entry is left alone


# ---- OPNetStreams._heal, entered from the launch monitor --------------------------------------------------------------------
def _host_pool(monkeypatch):
    """an OPNetStreams over a CPU state whose chain engine is the toy step above: everything between LaunchMonitor.verify and
    the log runs as in the product (redo -> _heal -> replay -> _rerun -> _step_chain), only the device calls are stubbed"""
    import contextlib
    import types
    from objectpermanence_amd.launch_monitor import LaunchMonitor
    from objectpermanence_amd.streaming import OPNetStreams, StreamReplayLog
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: synced.append(dev))
    pool = OPNetStreams.__new__(OPNetStreams)
    pool.device, pool._mlp, pool._gave_up, pool._x4_ok, pool.engine, pool.healed_calls = torch.device("cpu"), 0, False, True, "persistent", 0
    pool.state = torch.arange(5, dtype=torch.float32).reshape(5, 1).repeat(1, 2).contiguous()
    pool._row = 2
    pool._log = StreamReplayLog(pool._restore_rows, pool._rerun)
    pool.model = types.SimpleNamespace(_monitor=LaunchMonitor())
    pool.model._monitor._host = torch.zeros((64, 4), dtype=torch.int32)

    def chain(slots, boxes, lengths, out=None):
        pool.state[slots.long()] = 0.5 * pool.state[slots.long()] + boxes.sum()
        out[0].copy_(pool.state[slots.long()])
        out[1].copy_(-pool.state[slots.long()])
        return out
    pool._step_chain = chain
    return pool, synced


class _Done:
    def query(self):
        return True

    def synchronize(self):
        pass


def _logged_step(pool, slots, x, code):
    """what _step_persistent does around a launch, with the launch replaced by its outcome: code 0 = the toy step, else the
    write-back of a launch that gave up (rows untouched, NaN outputs) and its status words in the monitor's host mirror"""
    mon = pool.model._monitor
    slots, boxes = torch.tensor(slots, dtype=torch.int32), torch.tensor([x, 0.0])
    y, lg = torch.empty((len(slots), 2)), torch.empty((len(slots), 2))
    entry = pool._log.record(slots, pool.state.index_select(0, slots.long()), ("step", slots, boxes, None, y, lg))
    if code:
        y.fill_(float("nan"))
        lg.fill_(float("nan"))
    else:
        pool._step_chain(slots, boxes, None, (y, lg))
    entry.redo = lambda e=entry: pool._heal(e)
    slot = mon._free.pop()
    mon._host[slot] = torch.tensor([code, 7, 3, 0], dtype=torch.int32)
    mon._pending.append((_Done(), slot, entry.redo, "toy step"))
    return y, lg


@pytest.mark.parametrize("bad", [0, 2, 4])
def test_heal_through_the_monitor_rewinds_reruns_and_pins_the_pool_to_the_chain(monkeypatch, bad):
    from objectpermanence_amd import launch_monitor
    ref, _ = _host_pool(monkeypatch)
    outs_ref = [_logged_step(ref, s, x, 0) for s, x in CALLS]
    pool, synced = _host_pool(monkeypatch)
    monkeypatch.setattr(launch_monitor, "_warned", False)
    outs, derived = [], []
    for i, (s, x) in enumerate(CALLS):
        y, lg = _logged_step(pool, s, x, 1 if i == bad else 0)
        d = torch.empty_like(y)
        follow = lambda y=y, d=d: d.copy_(2 * y)       # what DetectorStreams derives from y
        follow()
        pool.log_followup(follow)
        outs.append((y, lg))
        derived.append(d)
    assert torch.isnan(outs[bad][0]).all() and len(pool._log) == 2 * len(CALLS)
    with pytest.warns(RuntimeWarning, match="gave up"):
        assert pool.verify_launches() == 1
    assert torch.equal(pool.state, ref.state)
    for (y, lg), (y_ref, lg_ref), d in zip(outs, outs_ref, derived):
        assert torch.equal(y, y_ref) and torch.equal(lg, lg_ref)
        assert torch.equal(d, 2 * y_ref)                   # the follow-ups ran again behind their steps
    assert pool.healed_calls == len(CALLS) - bad and synced == [pool.device]
    assert pool.engine == "chain" and pool._gave_up and len(pool._log) == 0
    assert pool.model._monitor.healed == 1 and pool.model._monitor.pending() == 0
    with pytest.raises(RuntimeError, match="gave up earlier"):
        pool._check_engine("persistent", None)
    pool._check_engine(None, None)                         # the default is the chain now
    pool.log_followup(lambda: derived.clear())             # no log, no follow-up kept
    assert len(pool._log) == 0 and derived
