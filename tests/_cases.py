"""Shared seeded input builders for the parity tests (oracle vs HIP path)."""
import numpy as np

from oracle import side_inputs as si


def attention_inputs(B, S, N, R, seed=0, D=64, scale_q=1.0):
  rng = np.random.default_rng(seed)
  q = (rng.standard_normal((B, S, N, D)) * scale_q).astype(np.float32)
  k = rng.standard_normal((B, S, N, D)).astype(np.float32)
  v = rng.standard_normal((B, S, N, D)).astype(np.float32)
  emb = (rng.standard_normal((R, N, D)) * 0.5).astype(np.float32) if R else None
  bias = (rng.standard_normal((R, N)) * 0.5).astype(np.float32) if R else None
  return q, k, v, emb, bias


def dense_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P=0, r=0, gidx=None):
  """Materialised [B,S,S] mask + ids for a pattern (what the reference would be fed)."""
  valid = valid if valid is not None else [S] * B
  mask = np.stack([si.sparse_pattern_mask(S, vl, radius, g0, ng, gidx) for vl in valid]).astype(np.int32)
  if id_mode:
    ids = si.relative_ids_from_desc(S, id_mode, m, P, r)
    ids = np.broadcast_to(ids, (B, S, S)).astype(np.int32).copy()
  else:
    ids = None
  return mask, ids


def bf16_round(x):
  import torch
  return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


# ---- strided [B,S,N,D] views inside poisoned storages (the layouts include/mmt_attn.h promises to take) --------------
# One bit pattern serves inputs and outputs: a QUIET NaN (top mantissa bit set, so that it propagates through any
# arithmetic that reads it) whose low bits are recognisable, so that "untouched" is checked bit for bit through an
# integer view of the storage.
POISON_BITS = {'torch.bfloat16': 0x7FE5, 'torch.float32': 0x7FE5A5A5}
LAYOUTS = ('contiguous', 'head_major', 'time_major', 'qkv_slices', 'qkv_per_head', 'padded', 'gapped_batch')
BROADCAST_LAYOUTS = ('broadcast_heads', 'broadcast_batch')


def align_unit(dtype):
  """Elements in 16 bytes: the unit every stride must be a multiple of."""
  import torch
  return 8 if dtype == torch.bfloat16 else 4


def layout_geometry(layout, shape, dtype, slot=1):
  """(strides of (b, s, n), offset, storage elements) of a named layout for a logical [B,S,N,D] array; `slot` picks
  the q / k / v place of the two fused layouts.  A tuple `(strides, offset, numel)` passes through (hand-made cases)."""
  if not isinstance(layout, str):
    strides, offset, numel = layout
    return tuple(int(s) for s in strides), int(offset), int(numel)
  B, S, N, D = shape
  a = align_unit(dtype)
  if layout == 'contiguous':
    return (S * N * D, N * D, D), 0, B * S * N * D
  if layout == 'head_major':                      # storage [B,N,S,D]
    return (N * S * D, D, S * D), 0, B * S * N * D
  if layout == 'time_major':                      # storage [S,B,N,D]
    return (N * D, B * N * D, D), 0, B * S * N * D
  if layout == 'qkv_slices':                      # storage [B,S,3,N,D]
    return (S * 3 * N * D, 3 * N * D, D), slot * N * D, B * S * 3 * N * D
  if layout == 'qkv_per_head':                    # storage [B,S,N,3,D]
    return (S * N * 3 * D, N * 3 * D, 3 * D), slot * D, B * S * N * 3 * D
  if layout == 'padded':                          # storage [B,S,N,D+a] sliced to D, base moved by a: rows 16-byte, not 128-byte aligned
    return (S * N * (D + a), N * (D + a), D + a), a, B * S * N * (D + a) + a
  if layout == 'gapped_batch':                    # poison between the examples
    gap = 41 * a
    return (S * N * D + gap, N * D, D), 0, B * (S * N * D + gap)
  if layout == 'broadcast_heads':                 # storage [B,S,1,D]
    return (S * D, D, 0), 0, B * S * D
  if layout == 'broadcast_batch':                 # storage [1,S,N,D]
    return (0, N * D, D), 0, S * N * D
  raise ValueError(f'unknown layout {layout!r}')


def _int_view(t):
  import torch
  return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _poison_int(dtype):
  bits = POISON_BITS[str(dtype)]
  width = 16 if '16' in str(dtype) else 32
  return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def strided_view(x, layout, poison=True, slot=1):
  """Places the logical [B,S,N,D] tensor `x` (bf16 or fp32, any device) into a larger flat storage and returns
  (view, storage): `view` has x's shape and values and the strides of `layout` (layout_geometry), every other element
  of `storage` holds POISON_BITS (zero with poison=False).  For the two broadcast layouts x must be constant along the
  broadcast axis (the view reads one copy)."""
  import torch
  B, S, N, D = x.shape
  strides, offset, numel = layout_geometry(layout, x.shape, x.dtype, slot)
  storage = torch.empty(numel, dtype=x.dtype, device=x.device)
  _int_view(storage).fill_(_poison_int(x.dtype) if poison else 0)
  view = storage.as_strided((B, S, N, D), strides + (1,), offset)
  if strides[0] == 0:
    assert bool((_int_view(x.contiguous()) == _int_view(x[:1].expand_as(x).contiguous())).all()), 'x varies along the batch'
    view[:1].copy_(x[:1])
  elif strides[2] == 0:
    assert bool((_int_view(x.contiguous()) == _int_view(x[:, :, :1].expand_as(x).contiguous())).all()), 'x varies along the heads'
    view[:, :, :1].copy_(x[:, :, :1])
  else:
    view.copy_(x)
  return view, storage


def assert_gaps_untouched(storage, view, chunk=1 << 27):
  """Every element of `storage` outside `view` still holds POISON_BITS, bit for bit.  The view's own elements are set
  to the pattern for the duration of the check (and put back), so that the comparison is one pass over the storage in
  chunks, with no index tensor of the storage's size."""
  pat = _poison_int(storage.dtype)
  views = []
  for view in (view if isinstance(view, (list, tuple)) else [view]):      # several disjoint views of one storage
    if view.stride(0) == 0:                     # a broadcast view: one copy is stored
      view = view[:1]
    if view.stride(2) == 0:
      view = view[:, :, :1]
    views.append(view)
  keeps = [view.clone() for view in views]
  iv = _int_view(storage)
  try:
    for view in views:
      iv.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(pat)
    for lo in range(0, iv.numel(), chunk):
      part = iv[lo:lo + chunk]
      bad = part != pat
      if bool(bad.any()):
        at = lo + int(bad.nonzero()[0])
        raise AssertionError(f'storage element {at} outside the view was written: bits {int(iv[at]) & 0xFFFFFFFF:#x}')
  finally:
    for view, keep in zip(views, keeps):
      view.copy_(keep)
