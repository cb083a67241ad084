"""Input contract of the models (`src/input_utils.py:21-103`) and the synthetic feature
generator that stands in for the reference's tf.data pipeline wherever no local records are named
(its OUTPUT feature contract is what is kept here, SURVEY.md 8(d), and
what `pretrain_dataloader.MmtPretrainDataLoader` produces from TFRecord shards)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .ops import AttentionPattern, side_inputs

CLS_ID, PATCH_ID, SEP_ID, ATT_ID = 101, 1, 102, 2   # [CLS], [PATCH]=[unused0], [SEP], [ATT]=[unused1]
MASK_ID = 103                                         # [MASK] of the BERT vocabulary
PATCH_START_UNUSED_INDEX = 104                        # src/data/data_utils.py:31


def encoder_input_spec(data_cfg) -> Dict[str, Tuple[tuple, torch.dtype]]:
  """`create_mmt_encoder_inputs` (`input_utils.py:21-53`): names, per-example shapes, dtypes."""
  P = data_cfg.image_size // data_cfg.patch_size
  S = data_cfg.max_seq_len
  return {
      'word_ids': ((S,), torch.int32),
      'segment_ids': ((S,), torch.int32),
      'relative_att_ids': ((S, S), torch.int32),
      'att_mask': ((S, S), torch.int32),
      'patch_embeddings': ((P * P, data_cfg.patch_size ** 2 * 3), torch.float32),
  }


def mtm_input_and_label_spec(data_cfg):
  """`create_mtm_inputs_and_labels` (`input_utils.py:56-103`)."""
  a, b = data_cfg.mlm_max_selections_per_seq, data_cfg.mpp_max_selections_per_seq
  inputs = {'mlm_positions': ((a,), torch.int32), 'mpp_positions': ((b,), torch.int32)}
  labels = {'mlm_label_ids': ((a,), torch.int32), 'mlm_label_weights': ((a,), torch.int32),
            'mpp_label_ids': ((b,), torch.int32), 'mpp_label_weights': ((b,), torch.int32)}
  return inputs, labels


def attention_pattern_from_config(data_cfg, encoder_cfg=None) -> AttentionPattern:
  """Pattern descriptor equivalent to the side inputs `get_add_side_input_features_fn` builds
  (`src/data/data_utils.py:285-332`) plus the build's band/global extension."""
  P = data_cfg.image_size // data_cfg.patch_size
  m = data_cfg.relative_pos_max_distance
  r = data_cfg.relative_att_num_core_layers
  n_img = 2 + P * P
  g = int(getattr(data_cfg, 'num_global_tokens', 0))
  a = int(getattr(data_cfg, 'image_grid_radius', 0))
  # relative_att_align_image: the 2-D ids read the image at grid_start like the grid term (no effect without 2-D ids)
  ids_2d = _lib.MMT_IDS_2D_IMAGE if getattr(data_cfg, 'relative_att_align_image', False) else _lib.MMT_IDS_2D
  return AttentionPattern(
      local_radius=int(getattr(data_cfg, 'local_radius', 1 << 30)),
      global_start=n_img if g else 0, n_global=g,     # the [ATT] marker and the tokens after it
      id_mode=_lib.MMT_IDS_NONE if m <= 0 else (ids_2d if r > 0 else _lib.MMT_IDS_1D),
      max_dist=m, patches_per_row=P if (r > 0 or a > 0) else 0, core_layers=r,
      grid_radius=a, grid_start=2)                    # the patches sit behind [CLS][PATCH]


def example_ids_from_breakpoints(long_breakpoints) -> torch.Tensor:
  """Example ids of packed rows from their ending breakpoints (1 at the last position of every example, 0 elsewhere):
  the reverse cumulative sum of `src/data/data_utils.py:321`, int32, same shape and device.  Positions of one example
  share an id; ids fall along the row and the padding after the last breakpoint gets 0."""
  bp = torch.as_tensor(long_breakpoints)
  return torch.flip(torch.cumsum(torch.flip(bp.to(torch.int64), [-1]), -1), [-1]).to(torch.int32)


def example_ids_from_lengths(lengths, S: int, device=None) -> torch.Tensor:
  """int32 [B,S] example ids of rows packed with examples of the given lengths (one list of lengths per row): the ids
  `example_ids_from_breakpoints` gives for breakpoints at the examples' last positions -- they fall from the row's
  example count to 1, and the tail after the last example is 0."""
  rows = []
  for row in lengths:
    row = [int(n) for n in row]
    if any(n <= 0 for n in row) or sum(row) > S:
      raise ValueError('example lengths must be positive and sum to at most S')
    bp = torch.zeros(S, dtype=torch.int32)
    if row:
      bp[torch.cumsum(torch.tensor(row), 0) - 1] = 1
    rows.append(bp)
  ids = example_ids_from_breakpoints(torch.stack(rows))
  return ids if device is None else ids.to(device)


def packed_example_layout(lengths, has_image, S: int, device=None):
  """Layout of rows packed with multimodal examples, from one list of example lengths per row and one list of "has an
  image" flags per row.  Returns (example_ids, example_starts, patch_slots, first_positions):
    example_ids    int32 [B,S]  as `example_ids_from_lengths` (falling to 1, the tail after the last example 0);
    example_starts int32 [B,S]  first position of the run each position belongs to (the tail is a run too);
    patch_slots    int32 [B,S]  index of the position's example among the IMAGED examples of the batch, in (row, run)
                                order -- its row of `patch_embeddings` [E, P^2, F]; -1 for examples without an image
                                and for the tail;
    first_positions int64 [E_all, 2]  (row, first position) of every example in (row, run) order, tails not counted."""
  ids = example_ids_from_lengths(lengths, S)
  if len(has_image) != len(lengths) or any(len(f) != len(row) for f, row in zip(has_image, lengths)):
    raise ValueError('has_image must hold one flag per example')
  starts = torch.zeros_like(ids)
  slots = torch.full_like(ids, -1)
  firsts, slot = [], 0
  for b, (row, flags) in enumerate(zip(lengths, has_image)):
    at = 0
    for n, img in zip(row, flags):
      n = int(n)
      starts[b, at:at + n] = at
      firsts.append((b, at))
      if img:
        slots[b, at:at + n] = slot
        slot += 1
      at += n
    starts[b, at:] = at
  first = torch.tensor(firsts, dtype=torch.int64).reshape(-1, 2)
  if device is not None:
    ids, starts, slots, first = (t.to(device) for t in (ids, starts, slots, first))
  return ids, starts, slots, first


def pack_examples_per_row(data_cfg, row_len: int) -> int:
  """Examples a row of `row_len` positions can hold at the most: every example has [CLS][PATCH], P*P patches, the field
  token and [SEP] at the least."""
  P = data_cfg.image_size // data_cfg.patch_size
  return max(1, int(row_len) // (2 + P * P + 2))


def pack_max_examples(data_cfg, batch_size: int, row_len: int) -> int:
  """The example slots of a packed batch (`MmtDataConfig.pack_rows`): the per-replica batch size times the examples a
  row can hold, capped at the kernel's limit (`MMT_PACK_MAX_EXAMPLES`)."""
  return min(int(batch_size) * pack_examples_per_row(data_cfg, row_len), _lib.MMT_PACK_MAX_EXAMPLES)


def pack_batch(inputs, labels, rows: int, row_len: int, max_examples: int):
  """Packs a prefix of an unpacked structured batch (`word_ids`, `segment_ids` [E,S], `valid_len` [E], optional
  `mlm_positions` / `mpp_positions`, per-example tensors such as `patch_embeddings`, and per-example `labels`) into `rows`
  rows of `row_len` positions: next-fit in arrival order, at most `max_examples` examples (`fused.pack_rows`,
  include/mmt_layer.h).  Returns (packed_inputs, packed_labels, consumed).

  Per-example tensors are not moved: packed example e is pool example e, so `patch_embeddings` and every label are the
  pool's first `max_examples` entries (zero entries behind a shorter pool).  Every `*_weights` label is multiplied by
  `example_weight` (0 for the slots at or behind `consumed`), so absent slots count in no loss and no metric, and every
  per-example input whose name ends in `_index` (`image_index`, `text_index`, `gt_image_index` of the retrieval loader)
  is -1 there, whatever the pool holds behind the prefix: `predict.predict` drops those slots.
  `packed_inputs` carries `example_ids`, `example_starts`, `patch_slots`, `first_positions`, the positions as flat
  indices into [rows * row_len] (the models' `flat_positions=True`) and the batch's `attention_pattern`; with
  `num_global_tokens > 0` the attention calls set MMT_FLAG_EXAMPLE_GLOBALS themselves (ops.py).  `consumed` is an int32
  [1] tensor on the batch's device: nothing here waits for it -- the loader reads it, the step never does."""
  from . import fused
  for k in ('word_ids', 'segment_ids', 'valid_len'):
    if inputs.get(k) is None:
      raise ValueError(f'pack_batch needs the structured batch\'s {k!r}')
  if 'att_mask' in inputs or 'relative_att_ids' in inputs:
    raise ValueError('pack_batch takes the structured batch (attention_pattern + valid_len), not dense side inputs')
  E, M = inputs['word_ids'].shape[0], int(max_examples)
  packed = fused.pack_rows(inputs['word_ids'], inputs['segment_ids'], inputs['valid_len'], rows, row_len, M,
                           mlm_positions=inputs.get('mlm_positions'), mpp_positions=inputs.get('mpp_positions'))
  weight = packed.pop('example_weight')
  consumed = packed.pop('consumed')

  def head(t):                                                   # the pool's first M entries, zeros behind a shorter pool
    if E >= M:
      return t[:M]
    return torch.cat([t, t.new_zeros((M - E,) + tuple(t.shape[1:]))])

  out_inputs = {}
  for k, v in inputs.items():
    if k == 'valid_len':
      continue
    if k in packed:
      out_inputs[k] = packed.pop(k)
    elif not torch.is_tensor(v):
      out_inputs[k] = v
    elif k.endswith('_index'):                                   # ids of the example (the retrieval loader's): -1 names an absent slot
      out_inputs[k] = torch.where(weight.reshape((M,) + (1,) * (v.dim() - 1)) > 0, head(v), torch.full_like(head(v), -1))
    else:
      out_inputs[k] = head(v)
  out_inputs.update(packed)                                      # example_ids, example_starts, patch_slots, first_positions
  out_labels = {}
  for k, v in labels.items():
    v = head(v)
    if k.endswith('_weights'):
      v = v * weight.to(v.dtype).reshape((M,) + (1,) * (v.dim() - 1))
    out_labels[k] = v
  return out_inputs, out_labels, consumed


def synthetic_retrieval_sets(data_cfg, n_images: int, n_texts: int, device, generator: Optional[torch.Generator] = None,
                             vocab_size: int = 30522):
  """A synthetic image set and text set (`retrieval.RetrievalSets`) with the layout and id ranges of `synthetic_batch`:
  the shared prefix `[CLS][PATCH] patch_1..patch_{P^2}`, every text `[ATT] text ... [SEP]` zero-padded to
  Lt = max_seq_len - 2 - P^2, ragged lengths in [2, Lt], ids 0 .. n - 1 for both sets and every text's ground-truth
  image drawn from the image set."""
  from .retrieval import RetrievalSets
  S = data_cfg.max_seq_len
  P = data_cfg.image_size // data_cfg.patch_size
  n_patch = P * P
  n_img = 2 + n_patch
  Lt = S - n_img
  if Lt < 2:
    raise ValueError('max_seq_len leaves no room for text')
  g = generator
  ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=device, generator=g, dtype=torch.int32)
  prefix = torch.empty(n_img, device=device, dtype=torch.int32)
  prefix[0], prefix[1] = CLS_ID, PATCH_ID
  prefix[2:] = PATCH_START_UNUSED_INDEX + torch.arange(n_patch, device=device, dtype=torch.int32)
  n_text = ri(2, Lt + 1, (n_texts,))
  text = ri(1000, vocab_size, (n_texts, Lt))
  text[:, 0] = ATT_ID
  text[torch.arange(n_texts, device=device), (n_text - 1).long()] = SEP_ID
  text = torch.where(torch.arange(Lt, device=device)[None] < n_text[:, None], text, torch.zeros_like(text))
  image_index = torch.arange(n_images, device=device, dtype=torch.int64)
  return RetrievalSets(
      data_cfg=data_cfg,
      patch_embeddings=torch.randn(n_images, n_patch, data_cfg.patch_size ** 2 * 3, device=device, generator=g),
      image_index=image_index, prefix_ids=prefix, text_token_ids=text, num_text_wordpieces=n_text,
      text_index=torch.arange(n_texts, device=device, dtype=torch.int64),
      gt_image_index=image_index[torch.randint(0, n_images, (n_texts,), device=device, generator=g)])


def synthetic_batch(data_cfg, batch_size: int, device, generator: Optional[torch.Generator] = None,
                    vocab_size: int = 30522, dense_side_inputs: bool = False,
                    ragged: bool = False, task: str = 'pretrain', pack_rows: int = 0, pack_row_len: int = 0,
                    text_lengths=None):
  """One (inputs, labels) pair with the shapes/dtypes of the reference's feature contract.
  Layout `[CLS][PATCH] patch_1..patch_{P^2} [ATT] text ... [SEP] pad` (data_utils.py:224-231).

  `pack_rows > 0` (structured inputs only): `batch_size * (row_len // (2 + P^2 + 2))` examples are drawn (capped at the
  kernel limit) and as many of them as fit go into `pack_rows` rows of `pack_row_len` positions (0 = max_seq_len) through
  `pack_batch`; the slots of the others carry weight 0 -- the stand-in draws afresh every batch and keeps no pool.
  `text_lengths`: int32 [B] text wordpiece counts to use instead of the drawn ones (clamped into [2, S - 2 - P^2])."""
  if pack_rows:
    if dense_side_inputs:
      raise ValueError('packed batches take the structured side inputs (dense_side_inputs=False)')
    row_len = int(pack_row_len) or data_cfg.max_seq_len
    n = pack_max_examples(data_cfg, batch_size, row_len)
    inputs, labels = synthetic_batch(data_cfg, n, device, generator, vocab_size, False, ragged, task, text_lengths=text_lengths)
    inputs, labels, _ = pack_batch(inputs, labels, int(pack_rows), row_len, n)
    return inputs, labels
  S = data_cfg.max_seq_len
  P = data_cfg.image_size // data_cfg.patch_size
  n_patch = P * P
  n_img = 2 + n_patch
  if n_img >= S:
    raise ValueError('max_seq_len leaves no room for text')
  g = generator
  B = batch_size
  ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=device, generator=g, dtype=torch.int32)
  word_ids = ri(1000, vocab_size, (B, S))
  word_ids[:, 0], word_ids[:, 1] = CLS_ID, PATCH_ID
  word_ids[:, 2:n_img] = PATCH_START_UNUSED_INDEX + torch.arange(n_patch, device=device, dtype=torch.int32)
  word_ids[:, n_img] = ATT_ID
  max_text = S - n_img
  if text_lengths is not None:
    n_text = torch.as_tensor(text_lengths).to(device=device, dtype=torch.int32).clamp(2, max_text)
  elif ragged:
    lo = max(2, int(0.75 * S) - n_img)
    n_text = ri(lo, max_text + 1, (B,))
  else:
    n_text = torch.full((B,), max_text, device=device, dtype=torch.int32)
  n_image = torch.full((B,), n_img, device=device, dtype=torch.int32)
  valid_len = (n_image + n_text).to(torch.int32)
  pos = torch.arange(S, device=device)[None]
  word_ids = torch.where(pos < valid_len[:, None], word_ids, torch.zeros_like(word_ids))
  pattern = attention_pattern_from_config(data_cfg)
  inputs = {
      'word_ids': word_ids,
      'patch_embeddings': torch.randn(B, n_patch, data_cfg.patch_size ** 2 * 3, device=device, generator=g),
  }
  if dense_side_inputs:     # exactly what the reference feeds: int32 [B,S,S] tensors
    si = side_inputs(pattern, n_image, n_text, S,
                     materialize_pattern=pattern.local_radius < S or pattern.n_global > 0 or pattern.grid_radius > 0)
    inputs.update(si)
    if si['relative_att_ids'] is None:
      inputs.pop('relative_att_ids')
  else:                     # structured fast path: descriptor + valid lengths only
    si = side_inputs(pattern, n_image, n_text, S, want_mask=False, want_ids=False)
    inputs['segment_ids'] = si['segment_ids']
    inputs['attention_pattern'] = pattern
    inputs['valid_len'] = valid_len
  labels = {}
  if task == 'pretrain':
    # MLM / MPP masking exactly as the reference's data pipeline applies it (`get_masking_fn`,
    # data_utils.py:383-639), on the device: feature_pipeline.make_mlm_and_mpp_features
    from . import feature_pipeline as fp
    rf = lambda *shape: torch.rand(*shape, device=device, generator=g)
    word_ids[torch.arange(B, device=device), (valid_len - 1).long()] = SEP_ID
    feats = {'patch_token_ids': word_ids[:, :n_img].contiguous(), 'text_token_ids': word_ids[:, n_img:].contiguous(),
             'num_text_wordpieces': n_text, 'patch_embeddings': inputs['patch_embeddings'],
             'unnormalized_patch_embeddings': rf(B, n_patch, data_cfg.patch_size ** 2 * 3)}
    randoms = {'mlm_item_keys': rf(B, max_text), 'mlm_value_u': rf(B, max_text), 'mlm_random_ids': ri(0, vocab_size, (B, max_text)),
               'mpp_item_keys': rf(B, n_img), 'mpp_value_u': rf(B, n_img), 'mpp_random_ids': ri(0, vocab_size, (B, n_img))}
    m = fp.make_mlm_and_mpp_features(
        feats, randoms, max_seq_len=S, num_patches=n_patch, patch_size=data_cfg.patch_size, vocab_size=vocab_size,
        mask_token_id=MASK_ID, unselectable_ids=(CLS_ID, SEP_ID, PATCH_ID, ATT_ID),
        mlm_fraction_to_mask=data_cfg.mlm_fraction_to_mask, mpp_fraction_to_mask=data_cfg.mpp_fraction_to_mask,
        mlm_max_selections_per_seq=data_cfg.mlm_max_selections_per_seq,
        mpp_max_selections_per_seq=data_cfg.mpp_max_selections_per_seq,
        output_channel_bits=data_cfg.output_channel_bits)
    inputs.update(word_ids=m['word_ids'], patch_embeddings=m['patch_embeddings'],
                  mlm_positions=m['mlm_positions'], mpp_positions=m['mpp_positions'])
    labels.update(mlm_label_ids=m['mlm_label_ids'], mlm_label_weights=m['mlm_label_weights'],
                  mpp_label_ids=m['mpp_label_ids'], mpp_label_weights=m['mpp_label_weights'])
    if 'itm' in (data_cfg.tasks or 'mlm,itm'):
      labels.update(itm_label_ids=ri(0, 2, (B,)),
                    itm_label_weights=torch.ones(B, device=device, dtype=torch.float32))
  else:
    labels.update(label_ids=ri(0, 2, (B,)), label_weights=torch.ones(B, device=device),
                  pos_weights=torch.ones(B, device=device))
  return inputs, labels
