"""Fine-tuning loader on TFRecord shards (`MmtClassificationDataLoader`, src/data/classification_dataloader.py:97-188):
image-text matching with in-batch negatives.  The record stages are `record_stages.RecordStages`'; the decode, the
matching step and the side inputs are the device stages the pretraining loader uses.  DESIGN.md section 4,
"Records: fine-tuning and retrieval", has the stage table against the reference's lines.

Against the pretraining loader there is no short-text filter and no masking (the reference's classification loader has
neither), the unnormalised patches are not kept, the matching step takes `negative_positive_ratio` from the config and
works on `feature_pipeline.matching_batch_size` examples, and the labels carry `itm_pos_weights`."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import feature_pipeline as fp
from .record_stages import RecordStages, _Pool

LABEL_KEYS = ('itm_label_ids', 'itm_label_weights', 'itm_pos_weights')       # classification_dataloader.py:77-79


class MmtClassificationDataLoader(RecordStages):
  """`MmtClassificationDataLoader(params).load(...)`: an iterator of (inputs, labels); inputs with the keys, shapes and
  dtypes of `input_utils.synthetic_batch(task='classification')`, labels `LABEL_KEYS` (int32, float32, float32, [B]).

  params: an `MmtClassificationDataConfig`.  The other arguments are `MmtPretrainDataLoader`'s."""

  def __init__(self, params, *, device=None, shuffle_buffer: int = 4096, example_shuffle_buffer: int = 4096,
               entropy: str = 'auto', dense_side_inputs: bool = False, chunk_bytes: int = 1 << 22):
    super().__init__(params, device=device, shuffle_buffer=shuffle_buffer, entropy=entropy, dense_side_inputs=dense_side_inputs,
                     chunk_bytes=chunk_bytes)
    self.example_shuffle_buffer = int(example_shuffle_buffer)
    self.names = [params.image_data_field, params.image_key_field] + list(self.field_dict)

  # ---- stage 4: decode on the device (:124-130, :154-156) -----------------------------------------------------------
  def _decode(self, group, gen) -> Dict[str, torch.Tensor]:
    """One group of (payload, stored crc, file, index) -> the decoded features of its examples on the device.
    `decode_image_features` applies RandAugment and the flip only when the config says is_training."""
    cfg, dev = self.params, self.device
    blob, blob_d, fields = self._open_group(group, self.names)
    images, image_at, keys, t_off, t_len = self._image_key_text_fields(group, blob.numpy(), fields)
    try:
      im = fp.decode_image_features(cfg, images, generator=gen, keep_unnormalized=False, device=dev, entropy=self.entropy,
                                    uploaded=(blob_d, image_at))
    except ValueError as e:
      raise ValueError(f'{group[0][2]} (records from {group[0][3]}): {e}') from None
    tx = self._decode_texts(blob_d, t_off, t_len)
    return {'patch_token_ids': self._patch_token_ids(len(group), im['patch_embeddings'].shape[1]),
            'patch_embeddings': im['patch_embeddings'], 'text_token_ids': tx['text_token_ids'],
            'num_text_wordpieces': tx['num_text_wordpieces'], 'image_key': self._meta(keys, torch.int64)}

  # ---- stage 5: the batch of the matching step (:132-137) ---------------------------------------------------------------
  def group_size(self, batch_size_per_replica: int) -> int:
    """Records the matching step takes at a time: enough that no roll creates a false negative, and a whole number of
    per-replica batches."""
    return fp.matching_batch_size(self.params, int(batch_size_per_replica))

  # ---- stage 8: word ids, side inputs and the split (:142-152, :166-184) -------------------------------------------------
  def _finish(self, ex):
    return self._encoder_inputs(ex), {k: ex[k] for k in LABEL_KEYS}

  def load(self, rank: int = 0, num_replicas: int = 1, batch_size: Optional[int] = None):
    """The iterator.  rank / num_replicas: the input pipeline (`input_context`); batch_size: the per-replica batch
    (default global_batch_size // num_replicas)."""
    cfg, dev = self.params, self.device
    B = int(batch_size or max(1, cfg.global_batch_size // num_replicas))
    Bm = self.group_size(B)
    training = bool(cfg.is_training)
    self.files()                                                 # a pattern without a match fails here, not at the first batch
    gen = torch.Generator(device=dev).manual_seed(int(cfg.seed) * 7919 + rank)
    stream = self._shuffle(self._interleave(self._file_stream(rank, num_replicas)), rank)

    def matched():                                               # stages 4 to 6: batch(Bm, drop_remainder=True), matching, unbatch
      group = []
      for item in stream:
        group.append(item)
        if len(group) == Bm:                                     # records short of a group at the end of a pass are dropped (:160)
          feats = self._decode(group, gen)
          group = []
          key = feats.pop('image_key')
          yield fp.make_matching_features_from_config(cfg, feats, key)

    def batches():                                               # :186
      pool = _Pool()
      chunks = self._example_shuffle(matched(), gen, self.example_shuffle_buffer) if training else matched()    # :179-180
      for ex in chunks:
        pool.push(ex)
        while pool.n >= B:
          yield self._finish(pool.pop(B))
      if pool.n and not training:
        yield self._finish(pool.pop(pool.n))

    return self._maybe_packed(batches(), B)
