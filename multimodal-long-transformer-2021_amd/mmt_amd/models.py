"""Model wrappers of the reference: `MmtPretrainingModel`
(`src/modeling/models/mmt_pretraining_model.py:23-173`) and `MmtClassificationModel`
(`src/modeling/models/mmt_classification_model.py:23-93`) around `MmtEncoder`."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import layers
from .encoder import MmtEncoder


def _check_unique(heads):
  if len({h.name for h in heads}) != len(heads):
    raise ValueError('Classification heads should have unique names.')


def _gather_flat(seq, position_sets):
  """Rows of `seq.view(B * S, H)` at flat indices: one index_select (and one scatter backward) for all the [E, n_i]
  tables of `position_sets`; returns the [E * n_i, H] row blocks.  Indices are clamped into the rows (they are data)."""
  B, S, H = seq.shape
  flat = [p.reshape(-1).to(torch.int64) for p in position_sets]
  rows = seq.reshape(B * S, H).index_select(0, torch.cat(flat).clamp(0, B * S - 1))
  return list(torch.split(rows, [f.numel() for f in flat]))


def _packed_heads(model, outputs, seq, first_positions, training, mlm_positions=None, mpp_positions=None,
                  flat_positions=False):
  """Head outputs of packed multimodal rows: the row of every example a head reads is `first position + cls_token_idx`,
  gathered into [E_all, 1, H] -- a batch of one-row sequences, which the heads read at index 0.  `flat_positions`: the
  MLM / MPP positions are [E_max, n] flat indices into the rows (`input_utils.pack_batch`), gathered once for both
  heads, so their logits are [E_max, n, classes] -- per example, like the labels."""
  if first_positions is None:
    raise ValueError('packed multimodal rows need first_positions: the heads read one row per example')
  if flat_positions:
    sets = [p for p in (mlm_positions, mpp_positions) if p is not None]
    rows = iter(_gather_flat(seq, sets) if sets else [])
    if mlm_positions is not None:
      outputs['mlm_logits'] = model.masked_lm(seq, masked_positions=mlm_positions, gathered=next(rows))
    if mpp_positions is not None:
      outputs['mpp_logits'] = model.masked_pp(seq, masked_positions=mpp_positions, gathered=next(rows))
    mlm_positions = mpp_positions = None
  if mlm_positions is not None:
    outputs['mlm_logits'] = model.masked_lm(seq, masked_positions=mlm_positions)
  if mpp_positions is not None:
    outputs['mpp_logits'] = model.masked_pp(seq, masked_positions=mpp_positions)
  S = seq.shape[1]
  for head in model.classification_heads:
    at = (first_positions[:, 1] + int(head.cls_token_idx)).clamp(max=S - 1)
    rows = seq[first_positions[:, 0], at]
    outputs[f'{head.name}_logits'] = head(seq, training=bool(training), gathered=rows)
  return outputs


class MmtPretrainingModel(nn.Module):

  def __init__(self, encoder: MmtEncoder, mpp_output_num_classes: Optional[int] = None,
               mlm_activation=None, mlm_initializer: str = 'glorot_uniform', mpp_activation=None,
               mpp_initializer: str = 'glorot_uniform',
               classification_heads: Optional[List[layers.ClassificationHead]] = None,
               bind_word_embedding_table: bool = True, name: str = 'mmt_pretraining_model'):
    super().__init__()
    self.name = name
    self.encoder = encoder
    self.classification_heads = nn.ModuleList(classification_heads or [])
    _check_unique(self.classification_heads)
    hidden = encoder.get_config()['hidden_size']
    self.masked_lm = layers.MaskedLM(encoder.get_word_embedding_layer(),
                                     layers.get_activation(mlm_activation),
                                     bind=bind_word_embedding_table)
    self.masked_pp = layers.MaskedPP(hidden, mpp_output_num_classes,
                                     layers.get_activation(mpp_activation), output='logits')

  def forward(self, word_ids, segment_ids=None, att_mask=None, relative_att_ids=None,
              patch_embeddings=None, mlm_positions=None, mpp_positions=None, training=None,
              attention_pattern=None, valid_len=None, example_ids=None, example_starts=None, patch_slots=None,
              first_positions=None, flat_positions=False):
    """Packed multimodal rows (`example_starts`, `patch_slots`, `first_positions`; `input_utils.packed_example_layout`):
    every classification head reads row `first position + cls_token_idx` of every example and returns
    [E_all, classes] in (row, run) order; MLM / MPP positions stay row positions unless `flat_positions` is true: then
    they are [E_max, n] indices into `sequence_output.view(R * S_row, H)` (`input_utils.pack_batch`), the rows are
    gathered once and the logits are [E_max, n, classes]."""
    if flat_positions and example_starts is None:
      raise ValueError('flat_positions goes with packed rows (example_starts)')
    outputs = dict(self.encoder(word_ids=word_ids, segment_ids=segment_ids, att_mask=att_mask,
                                relative_att_ids=relative_att_ids,
                                patch_embeddings=patch_embeddings, training=training,
                                attention_pattern=attention_pattern, valid_len=valid_len,
                                example_ids=example_ids, example_starts=example_starts, patch_slots=patch_slots,
                                first_positions=first_positions))
    seq = outputs['sequence_output']
    if example_starts is not None:
      return _packed_heads(self, outputs, seq, first_positions, training, mlm_positions, mpp_positions, flat_positions)
    # every head reads a few rows of the sequence output: pick them with one merged gather
    B = seq.shape[0]
    sets, names = [], []
    if mlm_positions is not None:
      sets.append(mlm_positions); names.append('/mlm')
    if mpp_positions is not None:
      sets.append(mpp_positions); names.append('/mpp')
    for head in self.classification_heads:
      sets.append(int(head.cls_token_idx))
      names.append(head.name)
    rows = dict(zip(names, layers.gather_rows_merged(seq, sets))) if sets else {}
    if mlm_positions is not None:
      outputs['mlm_logits'] = self.masked_lm(seq, masked_positions=mlm_positions, gathered=rows['/mlm'])
    if mpp_positions is not None:
      outputs['mpp_logits'] = self.masked_pp(seq, masked_positions=mpp_positions, gathered=rows['/mpp'])
    for head in self.classification_heads:
      outputs[f'{head.name}_logits'] = head(seq, training=bool(training), gathered=rows[head.name])
    return outputs

  @property
  def checkpoint_items(self):
    items = dict(encoder=self.encoder, masked_lm=self.masked_lm, masked_pp=self.masked_pp)
    for head in self.classification_heads:
      for key, item in head.checkpoint_items.items():
        items[f'{head.name}.{key}'] = item
    return items


class MmtClassificationModel(nn.Module):

  def __init__(self, encoder: MmtEncoder, classification_heads: List[layers.ClassificationHead],
               name: str = 'mmt_classification_model'):
    super().__init__()
    self.name = name
    self.encoder = encoder
    self.classification_heads = nn.ModuleList(classification_heads)
    _check_unique(self.classification_heads)

  def forward(self, word_ids=None, segment_ids=None, att_mask=None, relative_att_ids=None,
              patch_embeddings=None, training=None, attention_pattern=None, valid_len=None, example_ids=None,
              example_starts=None, patch_slots=None, first_positions=None, pairs=None, flat_positions=False):
    """Packed multimodal rows: as `MmtPretrainingModel.forward` -- head logits are [E_all, classes].  `flat_positions` is
    taken for the packed batches' sake (`input_utils.pack_batch`); this model has no position tables to read with it.
    `pairs=(sets, image_entry, text_entry)`: score the named pairs of a `retrieval.RetrievalSets` (`MmtEncoder.forward`);
    `word_ids`, `segment_ids`, `patch_embeddings` and `valid_len` must then be None."""
    if pairs is not None and any(x is not None for x in (word_ids, segment_ids, patch_embeddings, valid_len)):
      raise ValueError('with pairs=, word_ids, segment_ids, patch_embeddings and valid_len must be None')
    if pairs is None and word_ids is None:
      raise TypeError('forward() needs word_ids or pairs=')
    outputs = dict(self.encoder(word_ids=word_ids, segment_ids=segment_ids, att_mask=att_mask,
                                relative_att_ids=relative_att_ids,
                                patch_embeddings=patch_embeddings, training=training,
                                attention_pattern=attention_pattern, valid_len=valid_len,
                                example_ids=example_ids, example_starts=example_starts, patch_slots=patch_slots,
                                first_positions=first_positions, pairs=pairs))
    if example_starts is not None:
      return _packed_heads(self, outputs, outputs['sequence_output'], first_positions, training)
    for head in self.classification_heads:
      outputs[f'{head.name}_logits'] = head(outputs['sequence_output'], training=bool(training))
    return outputs

  @property
  def checkpoint_items(self):
    return dict(encoder=self.encoder, classification_heads=self.classification_heads)
