"""Host tests of the layout helpers of tests/_cases.py (`strided_view`, `assert_gaps_untouched`) on CPU tensors: the
GPU parity tests of test_gpu_attention_layouts.py rest on them."""
import numpy as np
import pytest
import torch

from tests._cases import (BROADCAST_LAYOUTS, LAYOUTS, POISON_BITS, align_unit, assert_gaps_untouched, layout_geometry,
                          strided_view)

DTYPES = [torch.float32, torch.bfloat16]
SHAPE = (2, 5, 3, 8)        # small, but two planes in b, three in n, and D a multiple of both alignment units


def _logical(dtype, layout):
  g = torch.Generator().manual_seed(1)
  x = torch.randn(SHAPE, generator=g).to(dtype)
  if layout == 'broadcast_heads':
    x = x[:, :, :1].expand(SHAPE).contiguous()
  if layout == 'broadcast_batch':
    x = x[:1].expand(SHAPE).contiguous()
  return x


def _bits(t):
  return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().astype(np.int64) & \
      (0xFFFF if t.dtype == torch.bfloat16 else 0xFFFFFFFF)


def _addresses(view):
  """Storage element index of every element of the view, from its strides (independent of the helper's own code)."""
  idx = np.full(view.shape, view.storage_offset(), np.int64)
  for dim, (n, st) in enumerate(zip(view.shape, view.stride())):
    shape = [1] * view.dim()
    shape[dim] = n
    idx = idx + (np.arange(n, dtype=np.int64) * st).reshape(shape)
  return idx


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('slot', [0, 1, 2])
@pytest.mark.parametrize('layout', LAYOUTS + BROADCAST_LAYOUTS)
def test_strided_view_layouts(layout, slot, dtype):
  x = _logical(dtype, layout)
  view, storage = strided_view(x, layout, slot=slot)
  a = align_unit(dtype)
  assert view.shape == x.shape and view.dtype == x.dtype
  assert (_bits(view) == _bits(x)).all()                                  # the view is the logical array
  assert view.stride(3) == 1 and all(s >= 0 and s % a == 0 for s in view.stride()[:3])
  assert view.stride()[:3] == layout_geometry(layout, SHAPE, dtype, slot)[0]
  assert view.storage_offset() % a == 0                                  # 16-byte aligned base
  addr = _addresses(view)
  assert addr.min() >= 0 and addr.max() < storage.numel()
  if layout in BROADCAST_LAYOUTS:
    assert np.unique(addr).size * (SHAPE[2] if layout == 'broadcast_heads' else SHAPE[0]) == addr.size
  else:
    assert np.unique(addr).size == addr.size                             # no two logical elements share storage
  outside = np.ones(storage.numel(), bool)
  outside[addr.ravel()] = False
  if layout != 'contiguous' and layout not in BROADCAST_LAYOUTS and layout != 'head_major' and layout != 'time_major':
    assert outside.any()                                                 # these layouts do have gaps
  assert (_bits(storage)[outside] == POISON_BITS[str(dtype)]).all()       # and every gap element is poison
  assert torch.isnan(storage.float()[torch.from_numpy(outside)]).all()    # ... which is a NaN
  assert_gaps_untouched(storage, view)
  assert (_bits(view) == _bits(x)).all()                                  # the check put the view back


def test_padded_rows_are_16_but_not_128_byte_aligned():
  for dtype in DTYPES:
    view, _ = strided_view(torch.zeros(1, 4, 2, 64, dtype=dtype), 'padded')
    esz = view.element_size()
    assert (view.storage_offset() * esz) % 16 == 0 and (view.storage_offset() * esz) % 128 != 0
    assert (view.stride(2) * esz) % 16 == 0 and (view.stride(2) * esz) % 128 != 0


def test_the_poison_is_a_quiet_nan():
  assert POISON_BITS['torch.bfloat16'] & 0x7FC0 == 0x7FC0 and POISON_BITS['torch.float32'] & 0x7FC00000 == 0x7FC00000
  view, storage = strided_view(torch.zeros(1, 2, 1, 8), 'padded')
  assert torch.isnan(storage).sum() == storage.numel() - view.numel()
  view, storage = strided_view(torch.zeros(1, 2, 1, 8), 'padded', poison=False)
  assert not torch.isnan(storage).any()


def test_hand_made_geometry_passes_through():
  x = torch.arange(2 * 3 * 2 * 8, dtype=torch.float32).reshape(2, 3, 2, 8)
  view, storage = strided_view(x, ((200, 24, 12), 4, 400))
  assert torch.equal(view, x) and view.stride() == (200, 24, 12, 1) and storage.numel() == 400
  assert_gaps_untouched(storage, view)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('layout', [l for l in LAYOUTS if l not in ('contiguous', 'head_major', 'time_major')])
def test_assert_gaps_untouched_sees_one_written_gap_element(layout, dtype):
  x = _logical(dtype, layout)
  view, storage = strided_view(x, layout)
  view.copy_(x * 2)                               # writing the view is what a kernel may do
  assert_gaps_untouched(storage, view, chunk=64)
  outside = np.ones(storage.numel(), bool)
  outside[_addresses(view).ravel()] = False
  for at in (np.flatnonzero(outside)[0], np.flatnonzero(outside)[-1]):
    saved = storage[at].clone()
    storage[at] = 0.0
    with pytest.raises(AssertionError, match=f'element {at} '):
      assert_gaps_untouched(storage, view, chunk=64)
    storage[at] = float('nan')                    # a NaN of another bit pattern is a write as well
    with pytest.raises(AssertionError):
      assert_gaps_untouched(storage, view, chunk=64)
    storage[at] = saved
  assert_gaps_untouched(storage, view, chunk=64)
