"""CPU-side checks of the persistent engine of the stacked-LSTM streams (include/opnet_hip.h opseq_stream_x_*,
objectpermanence_amd/streaming.py LstmStackStreams): size queries, argument refusals before anything is launched, `engine`
validation, and the replay log / healing that the stack pool shares with OPNetStreams, driven on a CPU state against a toy
chain step."""
import numpy as np
import pytest
import torch

BASE = (1, 75, 512)          # BaselineLstm: L, KX, H
NONLIN = (2, 3840, 512)      # NonLinearLstm at F = 256
SHAPES = [BASE, NONLIN]


def _lib():
    from objectpermanence_amd import _lib, build
    build.build()
    return _lib.load()


def test_x_stream_size_queries():
    lib = _lib()
    assert lib.opseq_stream_x_max_streams(1) == lib.opseq_xcd_max_batch(1) == 256
    assert lib.opseq_stream_x_max_streams(2) == lib.opseq_xcd_max_batch(2) == 128
    for L, KX, H in SHAPES:
        w = lib.opseq_stream_x_workspace_bytes(1, 1, L, KX, H)
        assert w > 0
        assert lib.opseq_stream_x_workspace_bytes(1, 8, L, KX, H) > w            # grows with k
        assert lib.opseq_stream_x_workspace_bytes(5, 1, L, KX, H) > w            # and with n (a second group of four)
        for n, k in ((1, 1), (5, 7), (70, 300), (128, 300)):
            # the whole-clip entry's workspace is not moved by this feature: the stream step's is that plus the cell-state
            # staging (4 clips x 512 floats per group and layer, rounded up to a page), and the status words stay put
            base = lib.opseq_xcd_workspace_bytes(n, k, L, KX, H)
            groups = (n + 3) // 4
            staging = groups * L * 512 * 4 * 4
            got = lib.opseq_stream_x_workspace_bytes(n, k, L, KX, H)
            assert base > 0 and got >= base + staging and got < base + staging + 4096 and got % 4096 == 0
            assert lib.opseq_stream_x_status_offset(n, k, L, KX, H) == lib.opseq_xcd_status_offset(n, k, L, KX, H)
            assert lib.opseq_stream_x_status_offset(n, k, L, KX, H) + 16 <= base
    assert lib.opseq_stream_x_workspace_bytes(256, 300, *BASE) > lib.opseq_stream_x_workspace_bytes(32, 300, *BASE)


def test_x_stream_shapes_not_served():
    from objectpermanence_amd import _lib as L_
    lib = _lib()
    refused = [(1, 1, 1, 75, 32),            # H
               (1, 1, 3, 75, 512),           # three layers
               (1, 1, 1, 200, 512),          # one layer with a wide direct input
               (1, 1, 2, 256, 512),          # transformer_lstm's stack: served as a whole clip, but there is no such stream
               (257, 1, *BASE), (129, 1, *NONLIN),      # n > max_streams
               (0, 1, *BASE), (1, 0, *BASE), (1, -3, *NONLIN)]
    for args in refused:
        assert lib.opseq_stream_x_workspace_bytes(*args) == 0, args
        assert lib.opseq_stream_x_status_offset(*args) == L_.NO_OFFSET, args
    assert lib.opseq_xcd_workspace_bytes(1, 1, 2, 256, 512) > 0
    lib.opseq_stream_x_workspace_bytes(257, 1, *BASE)
    assert b"257" in lib.opnet_last_error()
    lib.opseq_stream_x_workspace_bytes(1, 0, *BASE)
    assert b"positive" in lib.opnet_last_error()
    # beyond the 2 GiB one buffer descriptor addresses
    assert lib.opseq_stream_x_workspace_bytes(256, 100000, *BASE) == 0
    assert b"2 GiB" in lib.opnet_last_error()
    assert lib.opseq_stream_x_status_offset(256, 100000, *BASE) == L_.NO_OFFSET
    assert 0 < lib.opseq_stream_x_workspace_bytes(256, 300, *BASE) < 2 ** 31
    assert 0 < lib.opseq_stream_x_workspace_bytes(128, 300, *NONLIN) < 2 ** 31


@pytest.mark.parametrize("shape", SHAPES)
def test_x_stream_step_refuses_bad_arguments(shape):
    lib = _lib()
    L, KX, H = shape
    nmax = lib.opseq_stream_x_max_streams(L)
    # x, slots, state, xpacked, w_head, y, workspace, bytes, n, k, capacity, L, KX, H, stream
    step = lib.opseq_stream_step_x_f32
    none = [None] * 7
    assert step(*none, 0, 1, 1, 4, L, KX, H, None) == -1
    assert b"null" in lib.opnet_last_error()
    assert step(*none, 0, 1, 1, 4, L, KX, 32, None) == -2               # a shape seqx_dims rejects
    assert step(*none, 0, 1, 1, 4, 3, KX, H, None) == -2
    assert step(*none, 0, 1, 1, 4, 2, 256, 512, None) == -2             # (no stream for transformer_lstm)
    assert step(*none, 0, nmax + 1, 1, 512, L, KX, H, None) == -2       # more than max_streams
    assert step(*none, 0, 0, 1, 4, L, KX, H, None) == -2                # bad n, k, capacity
    assert step(*none, 0, 1, 0, 4, L, KX, H, None) == -2
    assert step(*none, 0, 1, 1, 0, L, KX, H, None) == -2
    assert b"capacity" in lib.opnet_last_error()
    p = 1 << 20       # fake, 16-byte aligned addresses: refused before any launch
    big = 1 << 30
    for i in range(7):                                                  # each pointer null in turn
        args = [p] * 7
        args[i] = None
        assert step(*args, big, 1, 1, 4, L, KX, H, None) == -1
        assert b"null" in lib.opnet_last_error()
    for i in (2, 3, 4, 5, 6):                                           # state, xpacked, w_head, y, workspace: 16 bytes
        args = [p] * 7
        args[i] = p + 4
        assert step(*args, big, 1, 1, 4, L, KX, H, None) == -1, i
        assert b"aligned" in lib.opnet_last_error()
    assert step(p, p + 2, p, p, p, p, p, big, 1, 1, 4, L, KX, H, None) == -1        # slots: 4 bytes
    assert step(p + 2, p, p, p, p, p, p, big, 1, 1, 4, L, KX, H, None) == -1        # x: 4 bytes, 16 when hoisted
    assert (step(p + 4, p, p, p, p, p, p, 64, 1, 1, 4, L, KX, H, None) == -1) == (L == 2)
    assert step(p, p, p, p, p, p, p, 64, 1, 1, 4, L, KX, H, None) == -3
    assert b"workspace" in lib.opnet_last_error()
    need = lib.opseq_stream_x_workspace_bytes(5, 7, L, KX, H)
    assert step(p, p, p, p, p, p, p, need - 1, 5, 7, 8, L, KX, H, None) == -3
    # the whole-clip entry's workspace is too small for the step: it has no room for the staging
    assert step(p, p, p, p, p, p, p, lib.opseq_xcd_workspace_bytes(5, 7, L, KX, H), 5, 7, 8, L, KX, H, None) == -3


def test_engine_validation():
    from objectpermanence_amd import LstmStackStreams, ModelsFactory
    small = {"baseline_lstm": {"videos_hidden_dim": 32}, "non_linear_lstm": {"boxes_features_dim": 8, "videos_hidden_dim": 32}}
    real = {"baseline_lstm": {"videos_hidden_dim": 512}, "non_linear_lstm": {"boxes_features_dim": 256, "videos_hidden_dim": 512}}
    for name in small:
        # the engine is looked at first: a bad one is refused even where the pool itself would be (a CPU model)
        with pytest.raises(ValueError, match="no automatic choice"):
            LstmStackStreams(ModelsFactory.get_model(name, small[name]), capacity=4, engine="auto")
        with pytest.raises(TypeError):
            LstmStackStreams(ModelsFactory.get_model(name, small[name]), capacity=4, engine=None)
        # the shape refusal is a host-side question too
        with pytest.raises(ValueError, match="reference shapes"):
            LstmStackStreams(ModelsFactory.get_model(name, small[name]), capacity=4, engine="persistent")
        # the reference shape passes it, and a CPU model is then refused as before, on either engine
        for engine in ("chain", "persistent"):
            with pytest.raises(RuntimeError, match="ROCm device"):
                LstmStackStreams(ModelsFactory.get_model(name, real[name]), capacity=4, engine=engine)
    with pytest.raises(RuntimeError, match="ROCm device"):
        LstmStackStreams(ModelsFactory.get_model("baseline_lstm", small["baseline_lstm"]), capacity=4)


# ---- the lifted log and healing on a stack pool, entered from the launch monitor ------------------------------------------
CALLS = [([0, 1, 2], 1.0), ([2, 3], 2.0), ([1, 4], 3.0), ([0, 2, 4], 4.0), ([3, 1], 5.0)]    # overlapping slot sets


def _host_pool(monkeypatch, L=1, KX=75, H=512):
    """a LstmStackStreams over a CPU state whose chain engine is a toy step (state = state / 2 + sum x: it does not commute with
    itself, so order matters): everything between LaunchMonitor.verify and the log runs as in the product (redo -> _heal ->
    replay -> _rerun -> _step_chain), only the device calls are stubbed"""
    import contextlib
    import types
    from objectpermanence_amd.launch_monitor import LaunchMonitor
    from objectpermanence_amd.streaming import LstmStackStreams, StreamReplayLog, StreamSlots
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: synced.append(dev))
    pool = LstmStackStreams.__new__(LstmStackStreams)
    pool.device, pool._embed, pool._gave_up, pool._x_ok, pool.engine, pool.healed_calls = torch.device("cpu"), False, False, True, "persistent", 0
    pool.L, pool.KX, pool.H = L, KX, H
    pool.state = torch.arange(5, dtype=torch.float32).reshape(5, 1).repeat(1, 2).contiguous()
    pool._row = 2
    pool.slots = StreamSlots(5)
    pool.capacity = 5
    pool.slots.open(5)
    pool._log = StreamReplayLog(pool._restore_rows, pool._rerun)
    mon = LaunchMonitor()
    mon._host = torch.zeros((64, 4), dtype=torch.int32)
    pool.model = types.SimpleNamespace(_runner=types.SimpleNamespace(_monitor=mon))

    def chain(slots, x, lengths, out=None):
        pool.state[slots.long()] = 0.5 * pool.state[slots.long()] + x.sum()
        out = (torch.empty((len(slots), 2)),) if out is None else out
        out[0].copy_(pool.state[slots.long()])
        return out
    pool._step_chain = chain
    return pool, mon, synced


class _Done:
    def query(self):
        return True

    def synchronize(self):
        pass


def _logged_step(pool, mon, slots, x, code):
    """what _step_persistent does around a launch, with the launch replaced by its outcome: code 0 = the toy step, else the
    write-back of a launch that gave up (rows untouched, NaN output) and its status words in the monitor's host mirror"""
    slots, x = torch.tensor(slots, dtype=torch.int32), torch.tensor([x, 0.0])
    y = torch.empty((len(slots), 2))
    entry = pool._log.record(slots, pool.state.index_select(0, slots.long()), ("step", slots, x, None, y))
    if code:
        y.fill_(float("nan"))
    else:
        pool._step_chain(slots, x, None, (y,))
    entry.redo = lambda e=entry: pool._heal(e)
    slot = mon._free.pop()
    mon._host[slot] = torch.tensor([code, 7, 3, 0], dtype=torch.int32)
    mon._pending.append((_Done(), slot, entry.redo, "toy step"))
    return y


def _chain_only(monkeypatch):
    ref, _, _ = _host_pool(monkeypatch)
    ref.engine = "chain"
    ys = [ref._step_chain(torch.tensor(s, dtype=torch.int32), torch.tensor([x, 0.0]), None)[0] for s, x in CALLS]
    return ref, ys


@pytest.mark.parametrize("bad", range(len(CALLS)))
def test_heal_through_the_monitor_ends_equal_to_a_chain_only_pool(monkeypatch, bad):
    from objectpermanence_amd import launch_monitor
    ref, ys_ref = _chain_only(monkeypatch)
    pool, mon, synced = _host_pool(monkeypatch)
    assert pool._launch_monitor() is mon
    monkeypatch.setattr(launch_monitor, "_warned", False)
    ys, derived = [], []
    for i, (s, x) in enumerate(CALLS):
        y = _logged_step(pool, mon, s, x, 1 if i == bad else 0)
        d = torch.empty_like(y)
        follow = lambda y=y, d=d: d.copy_(2 * y)       # what DetectorStreams derives from y
        follow()
        pool.log_followup(follow)
        ys.append(y)
        derived.append(d)
    assert torch.isnan(ys[bad]).all() and len(pool._log) == 2 * len(CALLS)
    if bad < len(CALLS) - 1:
        assert not torch.equal(pool.state, ref.state)
    with pytest.warns(RuntimeWarning, match="gave up"):
        assert pool.verify_launches() == 1
    assert torch.equal(pool.state, ref.state)
    for y, y_ref, d in zip(ys, ys_ref, derived):           # healed in place: the tensors the caller holds
        assert torch.equal(y, y_ref)
        assert torch.equal(d, 2 * y_ref)                   # the follow-ups ran again behind their steps
    assert pool.healed_calls == len(CALLS) - bad and synced == [pool.device]
    assert pool.engine == "chain" and pool._gave_up and len(pool._log) == 0
    assert mon.healed == 1 and mon.pending() == 0
    with pytest.raises(RuntimeError, match="gave up earlier"):
        pool._check_engine("persistent", None)
    pool._check_engine(None, None)                         # the default is the chain now
    pool.log_followup(lambda: derived.clear())             # no log, no follow-up kept
    assert len(pool._log) == 0 and derived


def test_set_state_and_open_are_logged_while_a_log_is_kept_and_lengths_are_refused(monkeypatch):
    from objectpermanence_amd import launch_monitor
    pool, _, _ = _host_pool(monkeypatch)
    with pytest.raises(ValueError, match="ragged"):
        pool._check_engine("persistent", [1, 2])
    with pytest.raises(ValueError, match="engine='chain'"):
        pool._check_engine(None, torch.zeros(2, dtype=torch.int32))         # the pool's default is "persistent" here
    pool._check_engine("chain", [1, 2])
    pool._check_engine("persistent", None)
    pool, mon, _ = _host_pool(monkeypatch, L=1, H=1)                        # the toy rows are [h_0 | c_0] of H = 1
    # no log kept: neither writes one
    pool.set_state([1], torch.full((1, 1, 1), 7.0), torch.full((1, 1, 1), 8.0))
    pool.slots.close([4])
    assert pool.open(1) == [4] and len(pool._log) == 0
    assert pool.state[1].tolist() == [7.0, 8.0] and pool.state[4].tolist() == [0.0, 0.0]
    # a persistent step that gives up, then a set_state and a re-opened stream behind it: the replay repeats both, in order
    monkeypatch.setattr(launch_monitor, "_warned", True)
    monkeypatch.setattr(mon, "reap", lambda: 0)            # the launch stays unverified until verify
    before = pool.state.clone()
    y = _logged_step(pool, mon, [1, 2], 1.0, 1)
    pool.set_state([2, 3], torch.tensor([[[5.0], [6.0]]]), torch.tensor([[[50.0], [60.0]]]))
    pool.slots.close([0])
    assert pool.open(1) == [0]
    assert len(pool._log) == 3
    y2 = _logged_step(pool, mon, [0, 3], 2.0, 0)
    assert pool.verify_launches() == 1
    want = before.clone()
    want[[1, 2]] = 0.5 * want[[1, 2]] + 1.0
    assert torch.equal(y, want[[1, 2]])
    want[2] = torch.tensor([5.0, 50.0])
    want[3] = torch.tensor([6.0, 60.0])
    want[0] = 0.0
    want[[0, 3]] = 0.5 * want[[0, 3]] + 2.0
    assert torch.equal(pool.state, want) and torch.equal(y2, want[[0, 3]])
    assert pool.healed_calls == 2 and len(pool._log) == 0 and pool.engine == "chain"


def test_the_log_plumbing_is_one_implementation():
    from objectpermanence_amd.streaming import LstmStackStreams, OPNetStreams, _StreamPool
    for name in ("_prune_log", "_log_write", "log_followup", "_restore_rows", "_rerun", "_heal", "verify_launches",
                 "_check_engine", "open"):
        assert getattr(OPNetStreams, name) is getattr(LstmStackStreams, name) is getattr(_StreamPool, name), name


def test_header_declares_the_new_entries():
    import os
    from objectpermanence_amd import _lib as L_
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "opnet_hip.h")).read()
    lib = _lib()
    for name in ("opseq_stream_x_max_streams", "opseq_stream_x_workspace_bytes", "opseq_stream_x_status_offset",
                 "opseq_stream_step_x_f32"):
        assert name + "(" in header and name in L_.EXPORTS and hasattr(lib, name)
    assert lib.opnet_hip_abi_version() == 9
