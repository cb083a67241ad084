"""`MmtEncoder` on MI355X: the reference's encoder surface (`src/modeling/models/mmt_encoder.py`)
over the HIP relative-attention path.

Same constructor arguments (`mmt_encoder.py:45-65`), same argument errors (`:69-80`), same
call contract `encoder(word_ids, segment_ids, att_mask, relative_att_ids, patch_embeddings,
training) -> {'sequence_output'}` (`:166-172,226-227`), same accessors (`:239-261`).
Extension: `attention_pattern` / `valid_len` run the structured fast path (mask and relative
ids generated in-kernel, nothing [S,S]-shaped is ever materialised).
"""
from __future__ import annotations

import collections
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused, layers
from .ops import AttentionPattern

_NUM_OTHER_RELATIVE_IDS = 3   # mmt_encoder.py:25


class MmtEncoder(nn.Module):

  def __init__(self, vocab_size: int, segment_vocab_size: int = 16, embedding_size: int = None,
               hidden_size: int = 768, num_hidden_layers: int = 12, num_attention_heads: int = 12,
               intermediate_size: int = 3072, inner_activation='gelu',
               hidden_dropout_prob: float = 0.1, attention_probs_dropout_prob: float = 0.1,
               max_absolute_position_embeddings: Optional[int] = None,
               relative_vocab_size: int = 32, relative_pos_max_distance: int = 12,
               initializer_range: float = 0.02, use_pre_activation_order: bool = False,
               use_one_hot_lookup: bool = True, use_pooler_layer: bool = False,
               patch_embedding_size: int = 768, compute_dtype: torch.dtype = torch.float32,
               name: str = 'mmt_encoder'):
    super().__init__()
    if relative_vocab_size is None:
      if relative_pos_max_distance != 0:
        raise ValueError('`relative_pos_max_distance` must be 0 when `relative_vocab_size` '
                         'is None.')
    elif relative_vocab_size < 2 * relative_pos_max_distance + 1 + _NUM_OTHER_RELATIVE_IDS:
      raise ValueError(f'`relative_vocab_size` ({relative_vocab_size}) too small for '
                       f'`relative_pos_max_distance` ({relative_pos_max_distance}')
    if embedding_size is None:
      embedding_size = hidden_size
    self.name = name
    self.compute_dtype = compute_dtype
    activation = layers.get_activation(inner_activation)

    self._word_embedding_layer = layers.EmbeddingLookup(
        vocab_size, embedding_size, projection_size=hidden_size,
        initializer_range=initializer_range, name='word_embeddings')
    if max_absolute_position_embeddings is None:
      self._position_embeddings = None
    else:
      self._position_embeddings = nn.Parameter(torch.empty(max_absolute_position_embeddings, hidden_size))
      layers.truncated_normal_(self._position_embeddings, initializer_range)
    self._segment_embedding_layer = layers.EmbeddingLookup(
        segment_vocab_size, embedding_size, projection_size=hidden_size,
        initializer_range=initializer_range, use_one_hot_lookup=use_one_hot_lookup,
        name='segment_embeddings')
    self._patch_projection_weight = nn.Parameter(torch.empty(hidden_size, patch_embedding_size))
    layers.truncated_normal_(self._patch_projection_weight, initializer_range)
    self._patch_projection_bias = nn.Parameter(torch.zeros(hidden_size))
    self._embedding_norm_layer = nn.LayerNorm(hidden_size, eps=1e-12)
    self._hidden_dropout_prob = hidden_dropout_prob
    self._transformer_layers = layers.RelativeTransformerLayers(
        hidden_size=hidden_size, num_hidden_layers=num_hidden_layers,
        num_attention_heads=num_attention_heads, intermediate_size=intermediate_size,
        hidden_act=activation, hidden_dropout_prob=hidden_dropout_prob,
        attention_probs_dropout_prob=attention_probs_dropout_prob,
        initializer_range=initializer_range, relative_vocab_size=relative_vocab_size,
        use_pre_activation_order=use_pre_activation_order, use_one_hot_lookup=use_one_hot_lookup)
    if use_pooler_layer:
      self._pooler_weight = nn.Parameter(torch.empty(hidden_size, hidden_size))
      layers.truncated_normal_(self._pooler_weight, initializer_range)
      self._pooler_bias = nn.Parameter(torch.zeros(hidden_size))
    config_dict = {
        'vocab_size': vocab_size, 'segment_vocab_size': segment_vocab_size,
        'hidden_size': hidden_size, 'num_hidden_layers': num_hidden_layers,
        'num_attention_heads': num_attention_heads, 'intermediate_size': intermediate_size,
        'inner_activation': inner_activation if isinstance(inner_activation, str) else 'custom',
        'hidden_dropout_prob': hidden_dropout_prob,
        'attention_probs_dropout_prob': attention_probs_dropout_prob,
        'max_absolute_position_embeddings': max_absolute_position_embeddings,
        'relative_vocab_size': relative_vocab_size,
        'relative_pos_max_distance': relative_pos_max_distance,
        'initializer_range': initializer_range,
        'use_pre_activation_order': use_pre_activation_order,
        'use_one_hot_lookup': use_one_hot_lookup, 'use_pooler_layer': use_pooler_layer,
    }
    self._config = collections.namedtuple('Config', config_dict.keys())(**config_dict)
    self.use_fused_embedding = True

  def _fused_embed_ok(self, word_ids):
    w, sg = self._word_embedding_layer, self._segment_embedding_layer
    H = w.embedding_table.shape[1]
    return (word_ids.is_cuda and w.embedding_projection is None and sg.embedding_projection is None
            and self.compute_dtype in (torch.float32, torch.bfloat16) and H % 8 == 0 and H <= 2048
            and w.embedding_table.dtype == torch.float32 and sg.embedding_table.dtype == torch.float32
            and sg.embedding_table.shape[1] == H and self.use_fused_embedding)

  def embed(self, word_ids, segment_ids=None, patch_embeddings=None, training=False, example_starts=None,
            patch_slots=None):
    """Embedding assembly, `mmt_encoder.py:189-218`: LayerNorm + dropout on
    the WORD embeddings only; segment / position / projected patches are added afterwards.
    On the GPU this is one HIP kernel (`fused.embed_assemble`) writing the compute dtype; the
    patch projection runs in the compute dtype like every other Dense layer of the stack.

    Packed multimodal rows (`example_starts`, `patch_slots` int32 [B,S]; `input_utils.packed_example_layout`): position s
    of an example that starts at `start` takes the absolute position row `s - start` and, when its `slot >= 0` and
    `0 <= s - start - 2 < P^2`, the projected patch `patch_embeddings[slot][s - start - 2]` -- `patch_embeddings` is then
    [E, P^2, F], one entry per imaged example of the batch.  Same kernel path on the GPU (`mmt_embed_fwd_packed`); the
    torch branch (`_embed_packed`) states the same rule and is the CPU yardstick."""
    if segment_ids is None:
      segment_ids = torch.ones_like(word_ids)
    ln = self._embedding_norm_layer
    if example_starts is not None and patch_embeddings is not None and patch_slots is None:
      raise ValueError('packed rows with patch_embeddings need patch_slots')
    if self._fused_embed_ok(word_ids):
      cd = self.compute_dtype
      pe = None
      if patch_embeddings is not None:
        pe = layers._linear(patch_embeddings.to(cd), self._patch_projection_weight, self._patch_projection_bias)
        if word_ids.shape[1] < 2 + pe.shape[1]:
          raise ValueError('sequence too short for [CLS], [PATCH] and the patches')
      p = self._hidden_dropout_prob if training else 0.0
      return fused.embed_assemble(word_ids, segment_ids, self._word_embedding_layer.embedding_table,
                                  self._segment_embedding_layer.embedding_table, ln.weight, ln.bias,
                                  pos_table=self._position_embeddings, patch_proj=pe, eps=ln.eps, p=p,
                                  seed=fused.next_seed(0) if p else 0, patch_start=2, out_dtype=cd,
                                  example_starts=example_starts, patch_slots=patch_slots)
    if example_starts is not None:
      return self._embed_packed(word_ids, segment_ids, patch_embeddings, training, example_starts, patch_slots)
    word = self._word_embedding_layer(word_ids)
    seg = self._segment_embedding_layer(segment_ids)
    word = F.layer_norm(word, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
    word = F.dropout(word, self._hidden_dropout_prob, training)
    emb = word + seg
    S = word.shape[1]
    if self._position_embeddings is not None:
      emb = emb + self._position_embeddings[:S]
    if patch_embeddings is not None:
      pe = F.linear(patch_embeddings.to(emb.dtype), self._patch_projection_weight,
                    self._patch_projection_bias)
      n_patch = pe.shape[1]
      # 2 is for CLS and [PATCH] (`:213-218`): patches live at [2, 2 + n_patch)
      emb = emb + F.pad(pe, (0, 0, 2, S - 2 - n_patch))
    return emb

  def _embed_packed(self, word_ids, segment_ids, patch_embeddings, training, example_starts, patch_slots):
    ln = self._embedding_norm_layer
    word = self._word_embedding_layer(word_ids)
    seg = self._segment_embedding_layer(segment_ids)
    word = F.layer_norm(word, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
    word = F.dropout(word, self._hidden_dropout_prob, training)
    emb = word + seg
    B, S = word_ids.shape
    local = torch.arange(S, device=word_ids.device)[None] - example_starts.long()
    if self._position_embeddings is not None:
      emb = emb + self._position_embeddings[local.clamp(0, self._position_embeddings.shape[0] - 1)]
    if patch_embeddings is not None:
      pe = F.linear(patch_embeddings.to(emb.dtype), self._patch_projection_weight, self._patch_projection_bias)
      E, n_patch = pe.shape[0], pe.shape[1]
      pj = local - 2                          # 2 is for CLS and [PATCH] (`:213-218`), now of every example
      has = (patch_slots >= 0) & (patch_slots < E) & (pj >= 0) & (pj < n_patch)
      rows = pe[patch_slots.long().clamp(0, max(E - 1, 0)), pj.clamp(0, n_patch - 1)]
      emb = emb + torch.where(has[..., None], rows, torch.zeros_like(rows[:1, :1]))
    return emb

  _PROJECTION_CHUNK = 64      # images per projection GEMM of an image table: M = 64 * P^2 rows at the most

  def project_image_table(self, sets, out=None):
    """Projected patches [I, P^2, H] (bias included, compute dtype) of `sets.patch_embeddings` with the projection's
    CURRENT weight and bias, in chunks of `_PROJECTION_CHUNK` images through `layers._linear`.  Nothing is cached here:
    the fused optimizer and a replayed train step write the parameters without touching torch's version counters, so
    no key on the host can tell a stale projection from a fresh one.  Whoever scores many batches of one set owns the
    result and says when it is recomputed (`retrieval.PairScorer`: at the start of every scoring call).  `out`: a
    buffer of that shape and dtype to write in place (its address may be baked into a recorded graph)."""
    w, b = self._patch_projection_weight, self._patch_projection_bias
    pe = sets.patch_embeddings
    I, C = pe.shape[0], self._PROJECTION_CHUNK
    with torch.no_grad():
      if out is None:
        out = torch.empty((I, pe.shape[1], w.shape[0]), dtype=self.compute_dtype, device=pe.device)
      elif out.shape != (I, pe.shape[1], w.shape[0]) or out.dtype != self.compute_dtype or out.device != pe.device:
        raise ValueError('out must be [I, P^2, H] in the compute dtype on the sets\' device')
      for i in range(0, I, C):
        out[i:i + C].copy_(layers._linear(pe[i:i + C].to(self.compute_dtype), w, b))
    return out

  def embed_pairs(self, sets, image_entry, text_entry, patch_proj=None):
    """Embedding assembly of all pairs from separate sets (`retrieval.RetrievalSets`): row b is image `image_entry[b]`
    followed by text `text_entry[b]` (int32 [B]), i.e. `embed` on `sets.materialize(image_entry, text_entry)` without
    that batch -- returns (emb [B,S,H], valid_len int32 [B]).  Prediction only (no dropout, no gradient).  An entry
    outside its table means "no image" / "empty text" (the padded tail of a batch).  `patch_proj`: the projected image
    table (`project_image_table`) of a caller that scores many batches and keeps it; None projects the table in this
    call, with the weights as they are now.  On the GPU one HIP kernel gathers from the resident tables
    (`fused.embed_assemble_pairs`, `mmt_embed_fwd_pairs`); the torch branch below states the same rule and is the CPU
    yardstick."""
    ln = self._embedding_norm_layer
    proj = self.project_image_table(sets) if patch_proj is None else patch_proj
    image_entry, text_entry = image_entry.to(torch.int32), text_entry.to(torch.int32)
    I, n_patch = proj.shape[0], proj.shape[1]
    n_img = 2 + n_patch
    T, Lt = sets.text_token_ids.shape
    S = n_img + Lt
    if self._fused_embed_ok(sets.text_token_ids):
      return fused.embed_assemble_pairs(image_entry, text_entry, sets.prefix_ids, sets.text_token_ids,
                                        sets.num_text_wordpieces, self._word_embedding_layer.embedding_table,
                                        self._segment_embedding_layer.embedding_table, ln.weight, ln.bias,
                                        pos_table=self._position_embeddings, patch_proj=proj, eps=ln.eps, patch_start=2,
                                        out_dtype=self.compute_dtype)
    with torch.no_grad():
      dev = sets.text_token_ids.device
      i_ok = (image_entry >= 0) & (image_entry < I)
      t_ok = (text_entry >= 0) & (text_entry < T)
      ti = text_entry.long().clamp(0, T - 1)
      text = torch.where(t_ok[:, None], sets.text_token_ids[ti], torch.zeros_like(sets.text_token_ids[:1]))
      n_text = torch.where(t_ok, sets.num_text_wordpieces[ti].clamp(0, Lt), torch.zeros_like(text_entry))
      B = image_entry.shape[0]
      word_ids = torch.cat([sets.prefix_ids[None].expand(B, n_img), text], 1)
      pos = torch.arange(S, device=dev)[None]
      segment_ids = ((pos < n_img).to(torch.int32)
                     + 2 * ((pos > n_img) & (pos < n_img + n_text[:, None])).to(torch.int32))
      word = self._word_embedding_layer(word_ids)
      seg = self._segment_embedding_layer(segment_ids)
      word = F.layer_norm(word, ln.normalized_shape, ln.weight, ln.bias, ln.eps)
      emb = word + seg
      if self._position_embeddings is not None:
        emb = emb + self._position_embeddings[:S]
      rows = proj[image_entry.long().clamp(0, max(I - 1, 0))].to(emb.dtype)
      rows = torch.where(i_ok[:, None, None], rows, torch.zeros_like(rows[:1, :1]))
      emb = emb + F.pad(rows, (0, 0, 2, S - 2 - n_patch))
      return emb, (n_img + n_text).to(torch.int32)

  def forward(self, word_ids=None, segment_ids=None, att_mask=None, relative_att_ids=None,
              patch_embeddings=None, training: Optional[bool] = None,
              attention_pattern: Optional[AttentionPattern] = None, valid_len=None, example_ids=None,
              example_starts=None, patch_slots=None, first_positions=None, pairs=None):
    """`example_starts` / `patch_slots` (with `example_ids`): packed multimodal rows (`embed`, ops.py).  `first_positions`
    int64 [E_all, 2] = (row, first position) of every example: `pooled_output` is then [E_all, H], gathered there.
    `pairs=(sets, image_entry, text_entry[, patch_proj])`: the batch is all the named pairs of a
    `retrieval.RetrievalSets` (`embed_pairs`; the optional fourth item is a projected image table the caller keeps); `word_ids`, `segment_ids`, `patch_embeddings` and `valid_len` must then be None -- they follow from
    the sets -- and `attention_pattern` is the structured pattern of the data config as for any structured call."""
    training = bool(training)
    if pairs is not None:
      if any(x is not None for x in (word_ids, segment_ids, patch_embeddings, valid_len)):
        raise ValueError('with pairs=, word_ids, segment_ids, patch_embeddings and valid_len must be None')
      if training:
        raise ValueError('pairs= is for prediction only')
      if any(x is not None for x in (example_ids, example_starts, patch_slots, first_positions)):
        raise ValueError('pairs= does not combine with packed rows')
      emb, valid_len = self.embed_pairs(*pairs)
      emb = emb.to(self.compute_dtype)
    else:
      if word_ids is None:
        raise TypeError('forward() needs word_ids or pairs=')
      emb = None
    if example_starts is not None and example_ids is None:
      raise ValueError('example_starts needs example_ids')
    if emb is None:
      emb = self.embed(word_ids, segment_ids, patch_embeddings, training, example_starts, patch_slots).to(self.compute_dtype)
    out = self._transformer_layers(inputs=emb, att_mask=att_mask, relative_att_ids=relative_att_ids,
                                   training=training, pattern=attention_pattern, valid_len=valid_len,
                                   example_ids=example_ids, example_starts=example_starts,
                                   dropout_seed=(fused.next_seed(0) >> 24) if training else 0)
    outputs = {'sequence_output': out}
    if hasattr(self, '_pooler_weight'):
      first = out[:, 0] if first_positions is None else out[first_positions[:, 0], first_positions[:, 1]]
      outputs['pooled_output'] = torch.tanh(layers._linear(first, self._pooler_weight, self._pooler_bias))
    return outputs

  # accessors, `mmt_encoder.py:239-261`
  def get_word_embedding_table(self):
    return self._word_embedding_layer.embedding_table

  def get_word_embedding_layer(self):
    return self._word_embedding_layer

  def get_config(self):
    return dict(self._config._asdict())

  @property
  def transformer_layers(self):
    return self._transformer_layers

  @property
  def pooler_layer(self):
    if hasattr(self, '_pooler_weight'):
      return self._pooler_weight
    raise ValueError('pooler layers is not initialized.')

  @classmethod
  def from_config(cls, config, custom_objects=None):
    return cls(**config)
