"""Pretraining loader on TFRecord shards (`MmtPretrainDataLoader`, src/data/pretrain_dataloader.py:74-224): the
reference's tf.data stages in its order, with the host doing files, frames and field lookup and the device doing
checksums, JPEG and PNG decode, RandAugment, patches, tokenisation, masking, matching and side inputs.  DESIGN.md section 4,
"Records", has the stage table against the reference's lines.

tf.data's shuffle order cannot be reproduced (another generator); the contract is that the same seed, rank and files
give the same batches, and that the stages and their order are the reference's."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import feature_pipeline as fp
from .record_stages import RecordStages, _Pool, check_input_patterns, wants_records      # noqa: F401  (the last two are read through this module)

MIN_TEXT_WORDPIECES = 6               # pretrain_dataloader.py:156


class MmtPretrainDataLoader(RecordStages):
  """`MmtPretrainDataLoader(params).load(...)`: an iterator of (inputs, labels) with the keys, shapes and dtypes of
  `input_utils.synthetic_batch(task='pretrain')`.

  params: an `MmtPretrainDataConfig`.  device: where the batches live (a GPU: the side inputs are HIP only).
  shuffle_buffer / example_shuffle_buffer: the record shuffle (host, payloads) and the example shuffle behind the
  matching step (device) -- 4096 in the reference.  `image_data` may hold JPEG or PNG files, mixed at will
  (`feature_pipeline.decode_images`).  entropy: `decode_jpeg_images`'s mode; 'auto' decodes the Huffman scan on the device
  from the blob that is uploaded once; PNG files are inflated on the host and uploaded as scanlines."""

  def __init__(self, params, *, device=None, shuffle_buffer: int = 4096, example_shuffle_buffer: int = 4096,
               entropy: str = 'auto', dense_side_inputs: bool = False, chunk_bytes: int = 1 << 22):
    super().__init__(params, device=device, shuffle_buffer=shuffle_buffer, entropy=entropy, dense_side_inputs=dense_side_inputs,
                     chunk_bytes=chunk_bytes)
    self.example_shuffle_buffer = int(example_shuffle_buffer)
    self.names = [params.image_data_field, params.image_key_field] + list(self.field_dict)

  # ---- stages 1 to 3 (:106-138): files, interleave and record shuffle are `RecordStages`' -------------------------------

  # ---- stage 4: decode on the device (:140-150) ---------------------------------------------------------------------
  def _decode(self, group, gen) -> Dict[str, torch.Tensor]:
    """One group of (payload, stored crc, file, index) -> the decoded features of its examples on the device."""
    cfg, dev = self.params, self.device
    n = len(group)
    blob, blob_d, fields = self._open_group(group, self.names)
    images, image_at, keys, t_off, t_len = self._image_key_text_fields(group, blob.numpy(), fields)
    try:
      im = fp.decode_image_features(cfg, images, generator=gen, keep_unnormalized=True, device=dev, entropy=self.entropy,
                                    uploaded=(blob_d, image_at))
    except ValueError as e:
      raise ValueError(f'{group[0][2]} (records from {group[0][3]}): {e}') from None
    tx = self._decode_texts(blob_d, t_off, t_len)
    return {'patch_token_ids': self._patch_token_ids(n, im['patch_embeddings'].shape[1]), 'patch_embeddings': im['patch_embeddings'],
            'unnormalized_patch_embeddings': im['unnormalized_patch_embeddings'],
            'text_token_ids': tx['text_token_ids'], 'num_text_wordpieces': tx['num_text_wordpieces'],
            'text_word_start': tx['text_word_start'], 'image_key': self._meta(keys, torch.int64)}

  # ---- stage 6: masking (:165-181) ------------------------------------------------------------------------------------
  def _mask(self, feats, gen) -> Dict[str, torch.Tensor]:
    cfg, dev = self.params, self.device
    n, T = feats['text_token_ids'].shape
    W = feats['patch_token_ids'].shape[1]
    V = len(self.vocab())
    rf = lambda *shape: torch.rand(*shape, device=dev, generator=gen)
    ri = lambda *shape: torch.randint(0, V, shape, device=dev, generator=gen, dtype=torch.int32)
    randoms = {'mlm_item_keys': rf(n, T), 'mlm_value_u': rf(n, T), 'mlm_random_ids': ri(n, T),
               'mpp_item_keys': rf(n, W), 'mpp_value_u': rf(n, W), 'mpp_random_ids': ri(n, W)}
    src = dict(feats)
    key = src.pop('image_key')
    if not cfg.mlm_use_whole_word:
      src.pop('text_word_start')
    unselectable = [self._special(t) for t in ('[CLS]', '[SEP]', '[PATCH]')] + [self._special(t) for t in self.field_dict.values()]
    out = fp.make_mlm_and_mpp_features(
        src, randoms, max_seq_len=cfg.max_seq_len, num_patches=W - 2, patch_size=cfg.patch_size, vocab_size=V,
        mask_token_id=self._special('[MASK]'), unselectable_ids=unselectable,
        mlm_fraction_to_mask=cfg.mlm_fraction_to_mask, mpp_fraction_to_mask=cfg.mpp_fraction_to_mask,
        mlm_max_selections_per_seq=cfg.mlm_max_selections_per_seq, mpp_max_selections_per_seq=cfg.mpp_max_selections_per_seq,
        patch_mask_token_id=self._special('[PATCH_MASK]') if cfg.use_patch_mask_token_id else None,
        channels=cfg.input_channels, output_channel_bits=cfg.output_channel_bits, max_pixel_val=cfg.max_pixel_val)
    keep = ('patch_token_ids', 'text_token_ids', 'num_text_wordpieces', 'patch_embeddings', 'mlm_positions', 'mlm_label_ids',
            'mlm_label_weights', 'mpp_positions', 'mpp_label_ids', 'mpp_label_weights')
    out = {k: out[k] for k in keep}
    out['image_key'] = key
    return out

  # ---- stage 8: side inputs and the split (:199-221), as synthetic_batch builds them ------------------------------------
  def _finish(self, ex, with_itm: bool):
    inputs = self._encoder_inputs(ex)
    inputs.update(mlm_positions=ex['mlm_positions'], mpp_positions=ex['mpp_positions'])
    labels = {k: ex[k] for k in ('mlm_label_ids', 'mlm_label_weights', 'mpp_label_ids', 'mpp_label_weights')}
    if with_itm:
      labels.update(itm_label_ids=ex['itm_label_ids'], itm_label_weights=ex['itm_label_weights'])
    return inputs, labels

  def load(self, rank: int = 0, num_replicas: int = 1, batch_size: Optional[int] = None):
    """The iterator.  rank / num_replicas: the input pipeline (`input_context`); batch_size: the per-replica batch
    (default global_batch_size // num_replicas)."""
    cfg, dev = self.params, self.device
    B = int(batch_size or max(1, cfg.global_batch_size // num_replicas))
    training = bool(cfg.is_training)
    with_itm = 'itm' in cfg.tasks.split(',')
    self.files()                                                 # a pattern without a match fails here, not at the first batch
    gen = torch.Generator(device=dev).manual_seed(int(cfg.seed) * 7919 + rank)
    stream = self._shuffle(self._interleave(self._file_stream(rank, num_replicas)), rank)

    def decoded():                                               # stages 4 and 5: chunks of decoded, filtered examples
      group = []
      for item in stream:
        group.append(item)
        if len(group) == B:
          yield self._decode(group, gen)
          group = []
      if group:
        yield self._decode(group, gen)

    def matched():                                               # stages 5 to 7: chunks of masked (and matched) examples
      pool = _Pool()
      for feats in decoded():
        if training:                                             # :153-163
          keep = torch.nonzero(feats['num_text_wordpieces'] >= MIN_TEXT_WORDPIECES).reshape(-1)
          feats = {k: v[keep] for k, v in feats.items()}
        pool.push(feats)
        while pool.n >= B:
          ex = self._mask(pool.pop(B), gen)
          if with_itm:                                           # :183-197: batch(B, drop_remainder=True), matching, unbatch
            key = ex.pop('image_key')
            ex = fp.make_matching_features(ex, key, negative_positive_ratio=1, min_shift=int(cfg.min_shift))
          yield ex
      if pool.n and not with_itm:
        yield self._mask(pool.pop(pool.n), gen)

    def shuffled():                                              # :214-215, on the device
      if not (with_itm and training):
        return matched()
      return self._example_shuffle(matched(), gen, self.example_shuffle_buffer)

    def batches():                                               # :221
      pool = _Pool()
      for ex in shuffled():
        ex.pop('image_key', None)
        pool.push(ex)
        while pool.n >= B:
          yield self._finish(pool.pop(B), with_itm)
      if pool.n and not training:
        yield self._finish(pool.pop(pool.n), with_itm)

    return self._maybe_packed(batches(), B)
