"""Host side of the hot path: torch tensors as buffer carriers over the C ABI.

`relative_attention` is the operator `etcmodel.layers.attention.QkvRelativeAttention`
computes inside `RelativeTransformerLayers` (reference call site
src/modeling/models/mmt_encoder.py:220-224; math SURVEY.md App. A.3).  Two input forms:

  * dense   : `att_mask`, `relative_att_ids` int32 [B,S,S] exactly as the reference feeds
              them (literal operator);
  * pattern : an `AttentionPattern` descriptor -- mask and ids are generated in-kernel and
              never materialised (the long-sequence fast path).

The segmented term of a pattern comes from `valid_len` (int32 [B]: one example and a padding tail per row) or from
`example_ids` (int32 [B,S]: packed rows, positions attend each other only inside one example -- the reference's
`make_segmented_att_mask` over `cumsum(long_breakpoints, reverse=True)`, src/data/data_utils.py:305-332; see
`input_utils.example_ids_from_breakpoints`).  The two are mutually exclusive.

Packed MULTIMODAL examples add `example_starts` (int32 [B,S], with `example_ids` only): the first position of the example
each position belongs to.  Relative ids, the image grid and the global range are then read at positions local to the
example (`x - start`), so that an example in a packed row sees what it would see alone at the start of a row
(`input_utils.packed_example_layout` builds ids and starts).  The structured kernels take this with an image grid and with
a contiguous range of global tokens (`MMT_FLAG_EXAMPLE_GLOBALS`: every example has its global tokens at its own
[global_start, global_start + n_global)); a listed global set, and global tokens with id_mode 3, go to the dense operator,
which is fed the composed mask and ids.
"""
from __future__ import annotations

import dataclasses
import math
import weakref
from typing import Optional

import torch

from . import _lib, step_scalars
from .deferred import notify_grad_ready


@dataclasses.dataclass(frozen=True)
class AttentionPattern:
  """Structured mask + relative-id generator (mirrors `mmt_mask_desc`).

  local_radius >= seq_len with n_global == 0 is the reference's segmented mask
  (src/data/data_utils.py:321-322); id_mode 1 is the etcmodel 1-D generator
  (data_utils.py:300-301), id_mode 2 `MmtRelativePositionGenerator`
  (src/feature_utils.py:29), which takes positions [0, P^2) for the image.  id_mode 3 (`MMT_IDS_2D_IMAGE`, not the
  reference's ids) is id_mode 2 with the image where the patches are, at [grid_start, grid_start + P^2): the
  positions before it are text-like; with example starts `grid_start` is local to every example.

  Global tokens: the contiguous range [global_start, global_start + n_global), or `global_index`, any set of
  positions (a tuple of ints).  A listed set that is in fact a contiguous run takes the structured kernels like
  the range form; any other set is served through the dense operator with the materialised mask (correct, but
  O(S^2) work and memory: there is no structured kernel for scattered global tokens).

  Image grid (`grid_radius` a > 0; SURVEY.md App. A.5 `grid_radius`): patches at most a image rows and a columns
  apart also attend each other -- the image at positions [grid_start, grid_start + P^2) in raster order,
  P = `patches_per_row` (which must then be set, whatever `id_mode`; with 1-D ids it changes no id).  0 = off.
  `grid_start` is one field of the descriptor: the grid term and the ids of id_mode 3 cannot disagree about the image.
  """
  local_radius: int = 1 << 30
  global_start: int = 0
  n_global: int = 0
  id_mode: int = _lib.MMT_IDS_1D
  max_dist: int = 12
  patches_per_row: int = 0
  core_layers: int = 0
  global_index: Optional[tuple] = None
  grid_radius: int = 0
  grid_start: int = 2

  def normalized(self) -> 'AttentionPattern':
    """The same pattern with a listed global set sorted, de-duplicated and -- when it is a contiguous run -- turned
    into the range form."""
    if self.global_index is None:
      return self
    idx = tuple(sorted({int(i) for i in self.global_index}))
    if any(i < 0 for i in idx):
      raise ValueError('global_index must hold non-negative positions')
    if not idx:
      return dataclasses.replace(self, global_index=None, global_start=0, n_global=0)
    if idx[-1] - idx[0] + 1 == len(idx):
      return dataclasses.replace(self, global_index=None, global_start=idx[0], n_global=len(idx))
    return dataclasses.replace(self, global_index=idx, global_start=0, n_global=len(idx))

  def to_desc(self, valid_len: Optional[torch.Tensor] = None, device=None) -> _lib.MaskDesc:
    m = _lib.MaskDesc()
    m.valid_len = valid_len.data_ptr() if valid_len is not None else None
    m.local_radius = min(int(self.local_radius), (1 << 31) - 1)
    m.global_start, m.n_global = int(self.global_start), int(self.n_global)
    m.id_mode, m.max_dist = int(self.id_mode), int(self.max_dist)
    m.patches_per_row, m.core_layers = int(self.patches_per_row), int(self.core_layers)
    # the word's first-image-position field is read with a grid radius, and by MMT_IDS_2D_IMAGE without one too
    reads_start = self.grid_radius > 0 or int(self.id_mode) == _lib.MMT_IDS_2D_IMAGE
    m.image_grid = _lib.image_grid(max(int(self.grid_radius), 0), self.grid_start) if reads_start else 0
    m.global_index = None
    if self.global_index is not None:
      if device is None:
        raise ValueError('a pattern with global_index needs the device its index list lives on')
      m.n_global = len(self.global_index)
      m.global_index = _index_list(self.global_index, device).data_ptr()
    return m


_INDEX_LISTS = {}


def _index_list(idx: tuple, device) -> torch.Tensor:
  """Device copy of a listed global set (kept alive here: descriptors carry raw pointers)."""
  key = (idx, str(device))
  t = _INDEX_LISTS.get(key)
  if t is None:
    if len(_INDEX_LISTS) > 64:
      _INDEX_LISTS.clear()
    t = _INDEX_LISTS[key] = torch.tensor(idx, dtype=torch.int32, device=device)
  return t


_DENSE_CACHE = {}
_ORIGIN_CACHE = {}       # what is derived from the last (example_ids, example_starts) pair: see _origin_cached


def _origin_cached(slot, key, example_ids, example_starts, build):
  """`build()` once per (key, ids tensor, starts tensor): the last result of each `slot` is kept, so that the layers
  of one encoder pass, forward and backward, share it.  As `_DENSE_CACHE`, the entry is tied to the two tensor OBJECTS
  (weak references + version counters) and dropped when either dies; `clear_pattern_cache` drops it too."""
  hit = _ORIGIN_CACHE.get(slot)
  vers = (example_ids._version, example_starts._version)
  if hit is not None and hit[0] == key and hit[1]() is example_ids and hit[2]() is example_starts and hit[3] == vers:
    return hit[4]
  value = build()
  drop = lambda _r, slot=slot: _ORIGIN_CACHE.pop(slot, None) if (_ORIGIN_CACHE.get(slot) or (None, None, None))[1:3].count(_r) else None
  _ORIGIN_CACHE[slot] = (key, weakref.ref(example_ids, drop), weakref.ref(example_starts, drop), vers, value)
  return value


def compose_origin(pat_mask, pat_ids, example_ids, example_starts):
  """Dense [B,S,S] mask and relative ids of packed examples with a per-example origin, from the single-example [S,S]
  pattern mask / ids: both gathered at the local positions (lq, lk) = (q - start[q], k - start[k]), clamped into
  [0, S), and ANDed with the equality of the example ids (ids outside an example are 0).  Plain torch, any device."""
  S = example_ids.shape[1]
  pos = torch.arange(S, device=example_ids.device)
  loc = (pos[None] - example_starts.long()).clamp_(0, S - 1)
  same = example_ids[:, :, None] == example_ids[:, None, :]
  lq, lk = loc[:, :, None], loc[:, None, :]
  mask = pat_mask[lq, lk].to(torch.int32) * same.to(torch.int32)
  ids = None if pat_ids is None else torch.where(same, pat_ids[lq, lk], torch.zeros_like(pat_ids[:1, :1])).to(torch.int32)
  return mask, ids


def _materialized(pattern: 'AttentionPattern', valid_len, B: int, S: int, device, example_ids=None, example_starts=None):
  """(att_mask, relative_att_ids) int32 [B,S,S] of a pattern the structured kernels do not take (a listed global set;
  with example ids also an image grid), through `mmt_side_inputs`;
  the last result is kept, so that the layers of one encoder pass (same pattern, same valid_len tensor) share it.
  The entry is tied to the valid_len tensor OBJECT (a weak reference + its version counter), never to its address:
  a later batch's tensor that the caching allocator places at the same address is a different object and misses;
  when the tensor dies the entry (two B*S*S int32 tensors) is dropped with it.
  With `example_ids` the pattern mask is built without a length and `ids[:, :, None] == ids[:, None, :]` is ANDed into
  it on the device; the entry is then tied to the ids tensor in the same way.  With `example_starts` as well the
  single-example [S,S] pattern is built once and gathered at the local positions (`compose_origin`); the last result is
  kept in the same manner, tied to both tensors (`_origin_cached`)."""
  packed = example_ids is not None
  if example_starts is not None:
    def build():
      one = torch.full((1,), S, dtype=torch.int32, device=device)
      pm = torch.empty((1, S, S), dtype=torch.int32, device=device)
      pi = torch.empty((1, S, S), dtype=torch.int32, device=device) if pattern.id_mode != _lib.MMT_IDS_NONE else None
      with torch.cuda.device(device):
        _lib.check(_lib.lib().mmt_side_inputs(pattern.to_desc(None, device), 1, S, one.data_ptr(), torch.zeros_like(one).data_ptr(),
                                              1, pm.data_ptr(), None if pi is None else pi.data_ptr(), None, _stream_ptr(device)))
      return compose_origin(pm[0], None if pi is None else pi[0], example_ids, example_starts)
    return _origin_cached('dense', (pattern, B, S, str(device)), example_ids, example_starts, build)
  if packed:
    valid_len = example_ids           # the tensor the entry is tied to
  key = (pattern, B, S, str(device), packed)
  hit = _DENSE_CACHE.get('last')
  if hit is not None and hit[0] == key:
    ref, ver = hit[3]
    if (valid_len is None and ref is None) or (ref is not None and valid_len is not None and ref() is valid_len
                                               and ver == valid_len._version):
      return hit[1], hit[2]
  if pattern.global_index is not None and any(i >= S for i in pattern.global_index):
    raise ValueError('global_index position outside the sequence')
  img = valid_len if (valid_len is not None and not packed) else torch.full((B,), S, dtype=torch.int32, device=device)
  txt = torch.zeros(B, dtype=torch.int32, device=device)
  mask = torch.empty((B, S, S), dtype=torch.int32, device=device)
  ids = torch.empty((B, S, S), dtype=torch.int32, device=device) if pattern.id_mode != _lib.MMT_IDS_NONE else None
  desc = pattern.to_desc(None, device)
  with torch.cuda.device(device):
    _lib.check(_lib.lib().mmt_side_inputs(desc, B, S, img.data_ptr(), txt.data_ptr(), 1, mask.data_ptr(),
                                          None if ids is None else ids.data_ptr(), None, _stream_ptr(device)))
  if packed:
    mask &= (example_ids[:, :, None] == example_ids[:, None, :]).to(torch.int32)
  if valid_len is None:
    tie = (None, 0)
  else:
    tie = (weakref.ref(valid_len, lambda _r: _DENSE_CACHE.pop('last', None) if _DENSE_CACHE.get('last', (None,) * 4)[3][0] is _r else None),
           valid_len._version)
  _DENSE_CACHE['last'] = (key, mask, ids, tie)
  return mask, ids


def clear_pattern_cache() -> None:
  """Drops the cached dense side inputs of listed global sets (and the device copies of their index lists)."""
  _DENSE_CACHE.clear()
  _ORIGIN_CACHE.clear()
  _INDEX_LISTS.clear()


def _resolve_pattern(pattern, att_mask, rel_ids, valid_len, q, example_ids=None, example_starts=None):
  """Listed global sets: contiguous runs become the range form, anything else the dense operator's inputs.  So does,
  with example ids, a pattern with an image grid (the structured kernels refuse that pair) -- unless example starts are
  given: they take the grid and a contiguous global range on the structured kernels (`_make_desc` sets
  MMT_FLAG_EXAMPLE_GLOBALS), and send a listed set, or global tokens under id_mode 3, to the dense operator."""
  if example_ids is not None and (att_mask is not None or rel_ids is not None):
    raise ValueError('example_ids go with a pattern: dense att_mask/relative_att_ids already hold the segmented mask')
  if pattern is None:
    return pattern, att_mask, rel_ids
  if pattern.global_index is not None:
    pattern = pattern.normalized()
  if example_starts is not None:
    structured = pattern.global_index is None and (pattern.n_global == 0 or int(pattern.id_mode) != _lib.MMT_IDS_2D_IMAGE)
  else:
    structured = pattern.global_index is None and not (example_ids is not None and pattern.grid_radius > 0)
  if structured:
    return pattern, att_mask, rel_ids
  if att_mask is not None or rel_ids is not None:
    raise ValueError('pass either dense att_mask/relative_att_ids or a pattern, not both')
  mask, ids = _materialized(pattern, valid_len, q.shape[0], q.shape[1], q.device, example_ids, example_starts)
  return None, mask, ids


def _stream_ptr(device) -> int:
  return torch.cuda.current_stream(device).cuda_stream


def _dtype_code(t: torch.Tensor) -> int:
  if t.dtype == torch.float32:
    return _lib.MMT_F32
  if t.dtype == torch.bfloat16:
    return _lib.MMT_BF16
  raise TypeError(f'relative_attention supports float32 and bfloat16, got {t.dtype}')


def _strides(t: torch.Tensor):
  if t.dim() != 4 or t.stride(3) != 1:
    raise ValueError('q/k/v/out must be [B,S,N,D] views with a contiguous head dimension')
  return (t.stride(0), t.stride(1), t.stride(2))


# Arrival counters of the kernels that merge partial results inside one launch (`mmt_attn_desc.sync`).  Who owns them:
#   * eager calls: `_SYNC`, one zero-filled buffer per (device, stream), created and grown here on that stream.  Calls
#     that share one are stream-ordered and every call leaves it zeroed.  Never named by a captured launch, so an entry
#     may be replaced by a larger one or evicted: the allocator frees it in the order of the stream it was made on.
#   * launches recorded into a graph: ONLY counters reserved before the capture (`reserve_sync_words`).  Whoever records
#     the graph holds that tensor for as long as the graph lives; it is handed out on its stream between `reserve` and
#     `release` only, so no eager call and no other graph shares it.  Without a reservation a capturing call gets no
#     counters (nothing is allocated or zero-filled by a captured node -- a fill that exists only as a node of a graph
#     that is abandoned, or never replayed, never runs) and the library takes its forms without an in-launch merge.
_SYNC = {}
_SYNC_RESERVED = {}
_SYNC_MAX_KEYS = 64
_SYNC_MIN_WORDS = 1024


def _sync_key(device, stream_ptr):
  device = torch.device(device)
  if device.index is None:
    device = torch.device(device.type, torch.cuda.current_device())
  return (str(device), int(stream_ptr))


def reserve_sync_words(device, stream, words: int) -> torch.Tensor:
  """Zero-filled arrival counters for the launches about to be CAPTURED on `stream` (a `torch.cuda.Stream` the caller
  owns and passes to `torch.cuda.graph(..., stream=stream)`).  Call it before the capture begins, keep the tensor until
  the graph is dropped, and call `release_sync_words` when the capture has ended (or raised)."""
  if torch.cuda.is_current_stream_capturing():
    raise RuntimeError('reserve_sync_words: reserve the counters before the capture begins')
  key = _sync_key(device, stream.cuda_stream)
  with torch.cuda.stream(stream):
    t = torch.zeros(max(int(words), _SYNC_MIN_WORDS), dtype=torch.int32, device=device)
  stream.synchronize()             # the fill has run: replays may come from any stream
  _SYNC_RESERVED[key] = t
  return t


def release_sync_words(device, stream) -> None:
  """Ends the reservation of `reserve_sync_words`: the counters are handed to no further call (the caller keeps them
  alive for the recorded launches that name them)."""
  _SYNC_RESERVED.pop(_sync_key(device, stream.cuda_stream), None)


def _sync_words(device, stream_ptr: int, words: int) -> Optional[torch.Tensor]:
  """The arrival counters for a call on (device, stream), or None: a call that is being captured on a stream nobody
  reserved counters for (or too few)."""
  key = _sync_key(device, stream_ptr)
  if torch.cuda.is_current_stream_capturing():
    t = _SYNC_RESERVED.get(key)
    return t if t is not None and t.numel() >= words else None
  t = _SYNC.get(key)
  if t is None or t.numel() < words:
    if key not in _SYNC and len(_SYNC) >= _SYNC_MAX_KEYS:
      _SYNC.pop(next(iter(_SYNC)))            # (oldest first; eager-only buffers, see above)
    t = _SYNC[key] = torch.zeros(max(int(words), _SYNC_MIN_WORDS), dtype=torch.int32, device=device)
  return t


def _origin_planes(example_ids, example_starts) -> torch.Tensor:
  """int32 [B,2,S] -- ids and starts as MMT_FLAG_EXAMPLE_STARTS wants them; the last pair's is kept (`_origin_cached`)."""
  return _origin_cached('planes', None, example_ids, example_starts,
                        lambda: torch.stack([example_ids, example_starts], 1).contiguous())


def _make_desc(q, k, v, out, R, pattern, valid_len, scale, mask_value, scale_before_add,
               dropout_p, dropout_seed, tuning=0, example_ids=None, example_starts=None) -> _lib.AttnDesc:
  B, S, N, D = q.shape
  d = _lib.AttnDesc()
  d.B, d.S, d.N, d.D, d.R = B, S, N, D, R
  d.dtype = _dtype_code(q)
  for name, t in (('q_stride', q), ('k_stride', k), ('v_stride', v), ('o_stride', out)):
    getattr(d, name)[:] = _strides(t)
  d.scale = float(scale if scale is not None else 1.0 / math.sqrt(D))
  d.mask_value = float(mask_value)
  d.flags = _lib.MMT_FLAG_SCALE_BEFORE_ADD if scale_before_add else 0
  d.dropout_p = float(dropout_p)
  d.dropout_seed = (int(dropout_seed) + step_scalars.host_epoch(q.device)) & ((1 << 64) - 1)
  d.dropout_epoch = step_scalars.epoch_ptr(q.device) if dropout_p else None
  if example_ids is not None:        # packed examples: the ids travel in the valid_len slot, named by the flag
    d.flags |= _lib.MMT_FLAG_EXAMPLE_IDS
    valid_len = example_ids
    if example_starts is not None:   # ... and with starts, both planes of one [B,2,S] tensor (kept alive by the descriptor)
      d.flags |= _lib.MMT_FLAG_EXAMPLE_STARTS
      if pattern is not None and pattern.global_index is None and pattern.n_global > 0:
        d.flags |= _lib.MMT_FLAG_EXAMPLE_GLOBALS     # per-example global tokens: the range at local positions
      valid_len = d._origin_planes = _origin_planes(example_ids, example_starts)
  d.mask = (pattern or AttentionPattern(id_mode=_lib.MMT_IDS_NONE)).to_desc(valid_len, q.device)
  d.tuning = int(tuning)
  sync = _sync_words(q.device, _stream_ptr(q.device), B * N)
  if sync is not None:
    d.sync, d.sync_words = sync.data_ptr(), sync.numel()
  else:
    d.sync, d.sync_words = None, 0
  return d


def _check_inputs(q, k, v, rel_emb, rel_bias, att_mask, rel_ids, valid_len, example_ids=None, example_starts=None):
  if not q.is_cuda:
    raise RuntimeError('relative_attention runs on the GPU only (no CPU fallback)')
  for t in (k, v):
    if t.shape != q.shape or t.dtype != q.dtype or t.device != q.device:
      raise ValueError('q, k, v must agree in shape, dtype and device')
  B, S, N, D = q.shape
  R = 0
  if rel_emb is not None:
    if rel_emb.dim() != 3 or rel_emb.shape[1:] != (N, D) or rel_emb.dtype != q.dtype:
      raise ValueError('rel_emb must be [R,N,D] in the dtype of q')
    R = rel_emb.shape[0]
    if not rel_emb.is_contiguous():
      raise ValueError('rel_emb must be contiguous')
    if rel_bias is not None and (rel_bias.shape != (R, N) or rel_bias.dtype != q.dtype
                                 or not rel_bias.is_contiguous()):
      raise ValueError('rel_bias must be contiguous [R,N] in the dtype of q')
  for t in (att_mask, rel_ids):
    if t is not None and (t.dtype != torch.int32 or t.shape != (B, S, S) or not t.is_contiguous()):
      raise ValueError('att_mask / relative_att_ids must be contiguous int32 [B,S,S]')
  if valid_len is not None and (valid_len.dtype != torch.int32 or valid_len.shape != (B,)
                                or not valid_len.is_contiguous()):
    raise ValueError('valid_len must be contiguous int32 [B]')
  if example_ids is not None:
    if valid_len is not None:
      raise ValueError('pass valid_len or example_ids, not both (ids 1 on [0, vl) and 0 after are valid_len = vl)')
    if (not torch.is_tensor(example_ids) or example_ids.dtype != torch.int32 or example_ids.shape != (B, S)
        or not example_ids.is_contiguous() or example_ids.device != q.device):
      raise ValueError('example_ids must be a contiguous int32 [B,S] tensor on the device of q')
  if example_starts is not None:
    if example_ids is None:
      raise ValueError('example_starts needs example_ids: a start says where the example of that id begins')
    if (not torch.is_tensor(example_starts) or example_starts.dtype != torch.int32 or example_starts.shape != (B, S)
        or not example_starts.is_contiguous() or example_starts.device != q.device):
      raise ValueError('example_starts must be a contiguous int32 [B,S] tensor on the device of q')
  return R


def relative_attention_forward(q, k, v, rel_emb=None, rel_bias=None, *, att_mask=None,
                               relative_att_ids=None, pattern: Optional[AttentionPattern] = None,
                               valid_len=None, scale=None, mask_value=-10000.0,
                               scale_before_add=False, dropout_p=0.0, dropout_seed=0,
                               return_lse=True, tuning=0, example_ids=None, example_starts=None):
  """Forward only.  Returns (out [B,S,N,D] in q.dtype, lse fp32 [B,N,S]).  `tuning`: `_lib.MMT_TUNE_*` kernel-selection
  switches (0 = the library's defaults; the parity tests use them to reach every kernel).  `example_ids`: contiguous
  int32 [B,S] on the device of q, instead of `valid_len` (packed rows; module docstring); `example_starts`: likewise, the
  first position of each position's example (packed multimodal examples)."""
  R = _check_inputs(q, k, v, rel_emb, rel_bias, att_mask, relative_att_ids, valid_len, example_ids, example_starts)
  pattern, att_mask, relative_att_ids = _resolve_pattern(pattern, att_mask, relative_att_ids, valid_len, q, example_ids, example_starts)
  dense = att_mask is not None or relative_att_ids is not None
  if dense and pattern is not None:
    raise ValueError('pass either dense att_mask/relative_att_ids or a pattern, not both')
  B, S, N, D = q.shape
  out = torch.empty((B, S, N, D), dtype=q.dtype, device=q.device)
  lse = torch.empty((B, N, S), dtype=torch.float32, device=q.device) if return_lse else None
  desc = _make_desc(q, k, v, out, R, pattern, valid_len, scale, mask_value, scale_before_add,
                    dropout_p, dropout_seed, tuning, None if dense else example_ids, None if dense else example_starts)
  L = _lib.lib()
  ws_bytes = 0 if dense else L.mmt_workspace_bytes(desc)
  ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=q.device)
  ptr = lambda t: None if t is None else t.data_ptr()
  with torch.cuda.device(q.device):
    _lib.check(L.mmt_attn_fwd(desc, ptr(q), ptr(k), ptr(v), ptr(rel_emb), ptr(rel_bias),
                              ptr(att_mask), ptr(relative_att_ids), ptr(out), ptr(lse), ptr(ws),
                              ws.numel(), _stream_ptr(q.device)))
  return out, lse


def side_inputs(pattern: AttentionPattern, num_image_wordpieces: torch.Tensor,
                num_text_wordpieces: torch.Tensor, max_seq_len: int, *, want_mask=True,
                want_ids=True, want_segment_ids=True, materialize_pattern=False):
  """Device-side `add_side_input_features` (src/data/data_utils.py:335-379), batched.

  Returns dict(segment_ids [B,S], att_mask [B,S,S], relative_att_ids [B,S,S]) int32.
  """
  if not num_image_wordpieces.is_cuda:
    raise RuntimeError('side_inputs runs on the GPU only (no CPU fallback)')
  dev = num_image_wordpieces.device
  B, S = num_image_wordpieces.shape[0], int(max_seq_len)
  img = num_image_wordpieces.to(torch.int32).contiguous()
  txt = num_text_wordpieces.to(torch.int32).contiguous()
  want_ids = want_ids and pattern.id_mode != _lib.MMT_IDS_NONE and pattern.max_dist > 0
  mask = torch.empty((B, S, S), dtype=torch.int32, device=dev) if want_mask else None
  ids = torch.empty((B, S, S), dtype=torch.int32, device=dev) if want_ids else None
  seg = torch.empty((B, S), dtype=torch.int32, device=dev) if want_segment_ids else None
  pattern = pattern.normalized()
  desc = pattern.to_desc(None, dev)
  ptr = lambda t: None if t is None else t.data_ptr()
  with torch.cuda.device(dev):
    _lib.check(_lib.lib().mmt_side_inputs(desc, B, S, ptr(img), ptr(txt), int(materialize_pattern),
                                          ptr(mask), ptr(ids), ptr(seg), _stream_ptr(dev)))
  return {'segment_ids': seg, 'att_mask': mask, 'relative_att_ids': ids}


def relative_attention_backward(dout, q, k, v, rel_emb, rel_bias, out, lse, *, att_mask=None,
                                relative_att_ids=None, pattern: Optional[AttentionPattern] = None,
                                valid_len=None, scale=None, mask_value=-10000.0,
                                scale_before_add=False, dropout_p=0.0, dropout_seed=0, grads_out=None,
                                rel_grads_accum=None, tuning=0, example_ids=None, example_starts=None):
  """Backward of `relative_attention_forward` (recomputes P from `lse`).

  Returns (dq, dk, dv, drel_emb, drel_bias); the table gradients are fp32.  `grads_out` may
  give preallocated (dq, dk, dv) with the strides of (q, k, v) -- e.g. the three slices of one
  fused [B,S,3,N,D] gradient buffer; they are written in place, and buffers of other strides raise
  ValueError.  `rel_grads_accum` = (demb [R,N,D], dbias [R,N] | None), fp32
  and contiguous: the table gradients are ADDED to these buffers (the fp32 master gradients) and
  returned as such."""
  R = _check_inputs(q, k, v, rel_emb, rel_bias, att_mask, relative_att_ids, valid_len, example_ids, example_starts)
  pattern, att_mask, relative_att_ids = _resolve_pattern(pattern, att_mask, relative_att_ids, valid_len, q, example_ids, example_starts)
  if att_mask is not None or relative_att_ids is not None:
    example_ids = example_starts = None     # the dense operator: the materialised mask holds the ids' term
  B, S, N, D = q.shape
  dout = dout if dout.stride() == out.stride() else dout.contiguous()
  if out.stride() != dout.stride():
    out = out.contiguous()
  if grads_out is not None:
    dq, dk, dv = grads_out
    for g, t in ((dq, q), (dk, k), (dv, v)):       # the caller's buffers are written or the call fails: never replaced
      if g.shape != t.shape or g.dtype != t.dtype or g.device != t.device or g.stride() != t.stride():
        raise ValueError('grads_out must be (dq, dk, dv) with the shape, dtype, device and strides of (q, k, v)')
  else:
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if dq.stride() != q.stride() or dk.stride() != k.stride() or dv.stride() != v.stride():
      # views that are not dense (fused-qkv slices, padded rows, expanded operands): gradients of their own layout
      q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
      dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
  desc = _make_desc(q, k, v, out, R, pattern, valid_len, scale, mask_value, scale_before_add,
                    dropout_p, dropout_seed, tuning, example_ids, example_starts)
  if rel_grads_accum is not None and R:
    drel_emb, drel_bias = rel_grads_accum
    for t, shape in ((drel_emb, (R, N, D)), (drel_bias, (R, N))):
      if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()
                            or t.device != q.device):
        raise ValueError(f'rel_grads_accum buffers must be contiguous fp32 {shape} on {q.device}')
    if rel_bias is not None and drel_bias is None:
      raise ValueError('rel_grads_accum needs a dbias buffer when rel_bias is given')
    desc.flags |= _lib.MMT_FLAG_ACCUM_REL_GRADS
  else:
    drel_emb = torch.empty((R, N, D), dtype=torch.float32, device=q.device) if R else None
    drel_bias = torch.empty((R, N), dtype=torch.float32, device=q.device) if (R and rel_bias is not None) else None
  L = _lib.lib()
  ws_bytes = L.mmt_workspace_bytes(desc)
  ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=q.device)
  ptr = lambda t: None if t is None else t.data_ptr()
  with torch.cuda.device(q.device):
    _lib.check(L.mmt_attn_bwd(desc, ptr(q), ptr(k), ptr(v), ptr(rel_emb), ptr(rel_bias),
                              ptr(att_mask), ptr(relative_att_ids), ptr(out), ptr(dout), ptr(lse),
                              ptr(dq), ptr(dk), ptr(dv), ptr(drel_emb), ptr(drel_bias), ptr(ws),
                              ws.numel(), _stream_ptr(q.device)))
  return dq, dk, dv, drel_emb, drel_bias


class _RelativeAttentionFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, rel_emb, rel_bias, kw):
    out, lse = relative_attention_forward(q, k, v, rel_emb, rel_bias, **kw)
    ctx.save_for_backward(q, k, v, rel_emb, rel_bias, out, lse)
    ctx.kw = kw
    return out

  @staticmethod
  def backward(ctx, dout):
    q, k, v, rel_emb, rel_bias, out, lse = ctx.saved_tensors
    kw = {a: b for a, b in ctx.kw.items() if a != 'return_lse'}
    dq, dk, dv, de, db = relative_attention_backward(dout, q, k, v, rel_emb, rel_bias, out, lse, **kw)
    de = None if de is None else de.to(rel_emb.dtype)
    db = None if db is None else db.to(rel_bias.dtype)
    return dq, dk, dv, de, db, None


def relative_attention(q, k, v, rel_emb=None, rel_bias=None, **kw):
  """Differentiable QkvRelativeAttention (see module docstring); kwargs as
  `relative_attention_forward` (att_mask / relative_att_ids or pattern / valid_len or example_ids (+ example_starts), scale,
  mask_value, scale_before_add, dropout_p, dropout_seed)."""
  kw.pop('return_lse', None)
  return _RelativeAttentionFn.apply(q, k, v, rel_emb, rel_bias, kw)


class _RelativeAttentionQkvFn(torch.autograd.Function):
  """Same operator on the fused projection output qkv [B,S,3,N,D]: the backward writes dq, dk, dv
  into the three slices of ONE gradient buffer (no per-slice zero-fill / copy in autograd)."""

  @staticmethod
  def forward(ctx, qkv, rel_emb, rel_bias, kw, sinks):
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    out, lse = relative_attention_forward(q, k, v, rel_emb, rel_bias, **kw)
    ctx.save_for_backward(qkv, rel_emb, rel_bias, out, lse)
    ctx.kw, ctx.sinks = kw, sinks
    return out

  @staticmethod
  def backward(ctx, dout):
    qkv, rel_emb, rel_bias, out, lse = ctx.saved_tensors
    kw = {a: b for a, b in ctx.kw.items() if a != 'return_lse'}
    dqkv = torch.empty_like(qkv)
    accum = None
    if ctx.sinks is not None and rel_emb is not None:     # fp32 master tables: add straight into .grad
      for p in ctx.sinks:
        if p is not None and p.grad is None:
          p.grad = torch.zeros_like(p, dtype=torch.float32)
      accum = (ctx.sinks[0].grad, None if ctx.sinks[1] is None else ctx.sinks[1].grad)
    _, _, _, de, db = relative_attention_backward(
        dout, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], rel_emb, rel_bias, out, lse,
        grads_out=(dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]), rel_grads_accum=accum, **kw)
    if accum is not None:
      for p in ctx.sinks:
        if p is not None:
          notify_grad_ready(p)
      return dqkv, None, None, None, None
    de = None if de is None else de.to(rel_emb.dtype)
    db = None if db is None else db.to(rel_bias.dtype)
    return dqkv, de, db, None, None


def relative_attention_qkv(qkv, rel_emb=None, rel_bias=None, rel_grad_sinks=None, **kw):
  """`relative_attention` on a fused, contiguous qkv [B,S,3,N,D] tensor.

  `rel_grad_sinks` = (emb_master, bias_master | None): fp32 master parameters whose low-precision
  copies are `rel_emb` / `rel_bias` (passed detached).  The backward then adds the fp32 table
  gradients straight into their `.grad` (no bf16 round trip, no separate accumulate kernels) and
  runs their `_mmt_grad_ready_hooks`."""
  if qkv.dim() != 5 or qkv.shape[2] != 3 or not qkv.is_contiguous():
    raise ValueError('qkv must be a contiguous [B,S,3,N,D] tensor')
  kw.pop('return_lse', None)
  if rel_grad_sinks is not None:
    for p in rel_grad_sinks:
      if p is not None and (p.dtype != torch.float32 or not p.is_contiguous()):
        raise ValueError('rel_grad_sinks must be contiguous fp32 parameters')
  return _RelativeAttentionQkvFn.apply(qkv, rel_emb, rel_bias, kw, rel_grad_sinks)
