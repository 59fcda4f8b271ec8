"""simq._batch.pack: the one packed upload behind grid_distance_images, grid_dense_paths, occupancy_maps and observation_update.
torch.device('cpu') stands in for the device: a tensor counts as device-resident when it lies on the device asked for, so CPU tensors
take the device-copy path here and numpy arrays the staging path."""
import numpy as np
import pytest
import torch

from simq import _batch

DEV = torch.device('cpu')


def test_device_blocks_are_written_after_the_staging_copy():
    """A device block between two host blocks lies inside the staging span, whose zeros would wipe it if it were copied first."""
    a, c = np.arange(1, 7, dtype=np.uint8).reshape(2, 3), np.arange(50, 54, dtype=np.uint8).reshape(2, 2)
    b = torch.arange(100, 105, dtype=torch.uint8)
    d = torch.arange(200, 203, dtype=torch.uint8)
    buf, offsets = _batch.pack([a, b, c, d], torch.uint8, DEV)
    assert offsets == [0, 6, 11, 15] and buf.dtype == torch.uint8 and buf.numel() == 18
    assert buf[0:6].tolist() == a.reshape(-1).tolist() and buf[11:15].tolist() == c.reshape(-1).tolist()
    assert buf[6:11].tolist() == b.tolist()                              # (inside the span of a .. c)
    assert buf[15:18].tolist() == d.tolist()                             # (outside it)


def test_no_host_array_no_host_touch(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('the host was touched')
    monkeypatch.setattr(torch, 'from_numpy', refuse)
    monkeypatch.setattr(np, 'zeros', refuse)
    t = [torch.full((2, 3), 7, dtype=torch.int32), torch.full((4,), 9, dtype=torch.int32)]
    buf, offsets = _batch.pack(t, torch.int32, DEV, align=16)
    assert offsets == [0, 16] and buf[0:6].tolist() == [7] * 6 and buf[16:20].tolist() == [9] * 4
    with pytest.raises(AssertionError, match='the host was touched'):
        _batch.pack(t + [np.ones(3, np.int32)], torch.int32, DEV)


def test_alignment_keeps_offsets_at_multiples_and_zeroes_the_padding():
    sizes = [1, 15, 16, 17]
    arrays = [np.full(n, 10 + n, np.uint8) if k % 2 == 0 else torch.full((n,), 10 + n, dtype=torch.uint8) for k, n in enumerate(sizes)]
    buf, offsets = _batch.pack(arrays, torch.uint8, DEV, align=16)
    assert offsets == [0, 16, 32, 48] and buf.numel() == 80
    want = np.zeros(80, np.uint8)
    for o, n in zip(offsets, sizes):
        want[o:o + n] = 10 + n
    assert np.array_equal(buf.numpy(), want)
    # the same arrays unaligned: one behind the other, nothing between them
    buf, offsets = _batch.pack(arrays, torch.uint8, DEV)
    assert offsets == [0, 1, 16, 32] and buf.numel() == 49 and np.array_equal(buf.numpy(), want[want != 0])


@pytest.mark.parametrize('on_device', [False, True])
def test_one_contiguous_block_is_one_copy(monkeypatch, on_device):
    """as_maps hands back a contiguous [P, rows, cols] block, and pack uploads it with one copy_ instead of P."""
    block = np.arange(4 * 5 * 6, dtype=np.uint8).reshape(4, 5, 6)
    maps, whole = _batch.as_maps(torch.from_numpy(block) if on_device else block, 'maps')
    assert len(maps) == 4 and whole is not None
    assert _batch.as_maps(block[:, :, ::2].copy()[:, ::2], 'maps', check=lambda m, what: m)[1] is None    # (not contiguous: no block)
    mask = np.ones((5, 6), np.uint8)
    copies = []
    real = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, 'copy_', lambda self, src, *a: (copies.append(src.numel()), real(self, src, *a))[1])
    buf, offsets = _batch.pack([whole, mask], torch.uint8, DEV)
    monkeypatch.undo()
    # a host block and the host mask share the one staging copy; a device block is one device copy behind the mask's staging copy
    assert copies == ([30, 120] if on_device else [150]) and offsets == [0, 120]
    assert np.array_equal(buf.numpy(), np.concatenate([block.reshape(-1), mask.reshape(-1)]))


def test_float32_and_int32_share_a_buffer_of_words():
    """observation_update's frame buffer: float32 tables and depth, int32 ids, as 4-byte words whose bits are kept."""
    px = np.asarray([0.5, -1.25, np.inf], np.float32)
    depth = torch.tensor([[1.5, -0.0], [3.0e-41, float('nan')]], dtype=torch.float32)        # (a denormal, -0 and a NaN: bits, not values)
    ids = np.asarray([[7, -1], [0, 2 ** 31 - 1]], np.int32)
    ids_dev = torch.tensor([-5, 6], dtype=torch.int32)
    buf, offsets = _batch.pack([px, depth, ids, ids_dev], torch.int32, DEV)
    assert buf.dtype == torch.int32 and offsets == [0, 3, 7, 11]
    words = buf.numpy()
    assert np.array_equal(words[0:3], px.view(np.int32)) and np.array_equal(words[3:7], depth.numpy().reshape(-1).view(np.int32))
    assert np.array_equal(words[7:11], ids.reshape(-1)) and np.array_equal(words[11:13], ids_dev.numpy())
