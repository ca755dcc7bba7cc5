"""CPU-side checks of the per-stream buffer caches (objectpermanence_amd/_device_cache.py) with CPU tensors and a counting
fake pack: when an image is packed, which buffer it lands in, least-recently-used eviction, grow-only workspaces and the
refusals.  Stream ids are plain integers here."""
import pytest
import torch

from objectpermanence_amd._device_cache import PackedImages, TrainingBuffers, Workspaces, check_weights

CPU = torch.device("cpu")


def _bytes64():
    return 64


class _Pack:
    """pack(image, nbytes): counts its calls and writes the call number into the image"""

    def __init__(self):
        self.calls = []

    def __call__(self, buf, nbytes):
        self.calls.append((buf, nbytes))
        buf.fill_(float(len(self.calls)))


def _weights():
    return [torch.ones(4, 4), torch.ones(4)]


def test_one_pack_per_weight_version():
    ws, pack, images = _weights(), _Pack(), PackedImages(4, "Test")
    img = images.get(1, ws, CPU, (_bytes64,), pack)
    assert len(pack.calls) == 1 and img.dtype == torch.float32 and img.numel() == 16 and pack.calls[0][1] == 64
    assert images.get(1, ws, CPU, (_bytes64,), pack) is img and len(pack.calls) == 1        # nothing changed: no pack
    ws[0].mul_(2.0)                                                                          # in place: _version bumps
    assert images.get(1, ws, CPU, (_bytes64,), pack) is img and len(pack.calls) == 2        # re-packed into the same buffer
    assert float(img[0]) == 2.0
    ws[1] = torch.zeros(4)                                                                   # a new tensor: a new data_ptr
    images.get(1, ws, CPU, (_bytes64,), pack)
    assert len(pack.calls) == 3 and pack.calls[2][0] is img


def test_an_image_per_stream():
    ws, pack, images = _weights(), _Pack(), PackedImages(4, "Test")
    a = images.get(1, ws, CPU, (_bytes64,), pack)
    b = images.get(2, ws, CPU, (_bytes64,), pack)
    assert a is not b and len(pack.calls) == 2
    ws[0].add_(1.0)
    assert images.get(2, ws, CPU, (_bytes64,), pack) is b and len(pack.calls) == 3
    assert float(a[0]) == 1.0 and float(b[0]) == 3.0          # stream 1's image is not rewritten by stream 2's re-pack
    assert images.get(1, ws, CPU, (_bytes64,), pack) is a and len(pack.calls) == 4


def test_images_evict_the_least_recently_used():
    ws, pack, images = _weights(), _Pack(), PackedImages(3, "Test")
    first = {s: images.get(s, ws, CPU, (_bytes64,), pack) for s in (1, 2, 3)}
    images.get(1, ws, CPU, (_bytes64,), pack)                  # 1 is now the most recent, 2 the least
    images.get(4, ws, CPU, (_bytes64,), pack)                  # drops 2
    assert len(pack.calls) == 4
    assert images.get(1, ws, CPU, (_bytes64,), pack) is first[1] and images.get(3, ws, CPU, (_bytes64,), pack) is first[3]
    assert len(pack.calls) == 4
    assert images.get(2, ws, CPU, (_bytes64,), pack) is not first[2] and len(pack.calls) == 5


def test_zero_starts_a_new_image_zeroed():
    ws, images = _weights(), PackedImages(4, "Test")
    seen = []
    img = images.get(1, ws, CPU, (_bytes64,), lambda buf, n: seen.append(buf.clone()), zero=True)
    assert torch.equal(seen[0], torch.zeros(16)) and img.numel() == 16
    empty = PackedImages(4, "Test")
    empty.get(1, ws, CPU, (_bytes64,), lambda buf, n: seen.append(buf))
    assert len(seen) == 2 and seen[1].numel() == 16


def test_refusals():
    images, pack = PackedImages(4, "Test"), _Pack()
    with pytest.raises(RuntimeError, match=r"Test parameters must be contiguous fp32 .*model.to\(device\)"):
        images.get(1, [torch.ones(4, 4).t()], CPU, (_bytes64,), pack)
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        images.get(1, [torch.ones(4, dtype=torch.float64)], CPU, (_bytes64,), pack)
    with pytest.raises(RuntimeError, match="on the input's device"):
        check_weights([torch.ones(4)], torch.device("cuda", 0), "Test")
    check_weights(_weights(), CPU, "Test")
    assert pack.calls == []
    # a size of 0 is the library refusing the shape: raised with its message (H1 must be a multiple of 16)
    from objectpermanence_amd import _lib, build
    build.build()
    lib = _lib.load()
    with pytest.raises(_lib.OpnetHipError, match="opnet_packed_weights_bytes.*multiples of 16"):
        images.get(1, _weights(), CPU, (lib.opnet_packed_weights_bytes, 250, 512), pack)
    with pytest.raises(_lib.OpnetHipError, match="opnet_workspace_bytes"):
        Workspaces(4).get(1, (32, 300), CPU, (lib.opnet_workspace_bytes, 32, 300, 250, 512))
    with pytest.raises(_lib.OpnetHipError, match="opnet_train_workspace_bytes"):
        TrainingBuffers().history_for(32, 300, CPU, (lib.opnet_train_workspace_bytes, 32, 300, 250, 512))
    assert pack.calls == []


def test_workspaces_per_shape_and_stream_with_lru():
    sizes = []

    def nbytes(n):
        sizes.append(n)
        return n

    ws = Workspaces(3)
    a = ws.get(1, (8, 300), CPU, (nbytes, 100))
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert ws.get(1, (8, 300), CPU, (nbytes, 100)) is a and sizes == [100]      # asked only when a buffer is made
    b = ws.get(2, (8, 300), CPU, (nbytes, 100))
    c = ws.get(1, (4, 300), CPU, (nbytes, 50))
    assert len({id(a), id(b), id(c)}) == 3
    assert ws.get(1, (8, 300), CPU, (nbytes, 100)) is a                        # b is now the least recently used
    ws.get(3, (8, 300), CPU, (nbytes, 100))
    assert len(list(ws.values())) == 3 and all(v is not b for v in ws.values())
    assert [k for k, _ in ws.items()] == [(4, 300, None, 1), (8, 300, None, 1), (8, 300, None, 3)]


def test_one_workspace_per_stream():
    ws = Workspaces(4, one_per_stream=True)
    a = ws.get(1, (8, 300), CPU, (_bytes64,))
    b = ws.get(2, (8, 300), CPU, (_bytes64,))
    c = ws.get(1, (4, 300), CPU, (_bytes64,))                                 # stream 1's other shape goes
    assert [v for v in ws.values()] == [b, c] and a is not c


def test_grow_only_workspaces():
    ws = Workspaces(2, grow_only=True)
    a = ws.get(1, (), CPU, (int, 100))
    assert ws.get(1, (), CPU, (int, 60)) is a                                  # smaller: the same buffer
    assert ws.get(1, (), CPU, (int, 100)) is a
    b = ws.get(1, (), CPU, (int, 200))                                         # larger: replaced
    assert b.numel() == 200 and len(list(ws.values())) == 1
    ws.get(2, (), CPU, (int, 10))
    ws.get(3, (), CPU, (int, 10))                                              # past the limit: stream 1's goes
    assert all(v is not b for v in ws.values()) and len(list(ws.values())) == 2


def test_training_buffers():
    tb, pack = TrainingBuffers(), _Pack()
    img = tb.packed(CPU, (_bytes64,), pack, zero=True)
    assert tb.packed(CPU, (_bytes64,), pack) is img and len(pack.calls) == 2    # re-packed by every forward
    h = tb.history_for(4, 30, CPU, (int, 100))
    assert tb.key == (4, 30, None) and tb.history is h and h.numel() == 100
    assert tb.history_for(4, 30, CPU, (int, 100)) is h
    h2 = tb.history_for(8, 30, CPU, (int, 200))
    assert h2.numel() == 200 and tb.key == (8, 30, None) and tb.history is h2
