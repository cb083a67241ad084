"""Pretraining loader on TFRecord shards (`MmtPretrainDataLoader`, src/data/pretrain_dataloader.py:74-224): the
reference's tf.data stages in its order, with the host doing files, frames and field lookup and the device doing
checksums, JPEG and PNG decode, RandAugment, patches, tokenisation, masking, matching and side inputs.  DESIGN.md section 4,
"Records", has the stage table against the reference's lines.

tf.data's shuffle order cannot be reproduced (another generator); the contract is that the same seed, rank and files
give the same batches, and that the stages and their order are the reference's."""
from __future__ import annotations

import glob
import json
import os
import random
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from . import feature_pipeline as fp
from . import input_utils, records, text_frontend
from .ops import side_inputs

MIN_TEXT_WORDPIECES = 6               # pretrain_dataloader.py:156


def wants_records(input_path: str, vocab_filename: str) -> bool:
  """Whether `tasks.build_inputs` reads records: a non-empty input_path without a URL scheme, and a vocabulary file.
  Everything else -- the empty path and the `gs://` placeholder of the committed YAMLs -- stays synthetic; a path with a
  scheme is never opened."""
  return bool(input_path) and '://' not in input_path and bool(vocab_filename) and os.path.isfile(vocab_filename)


def check_input_patterns(patterns) -> List[str]:
  """`data_utils.check_input_patterns`: every pattern must match at least one file.  Returns the sorted files."""
  files: List[str] = []
  for pattern in patterns:
    hit = glob.glob(pattern)
    if not hit:
      raise ValueError(f'input pattern {pattern!r} matches no file')
    files.extend(hit)
  return sorted(files)


def _cat(chunks: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
  return chunks[0] if len(chunks) == 1 else {k: torch.cat([c[k] for c in chunks]) for k in chunks[0]}


class _Pool:
  """Examples in hand, as one dict of tensors with a common leading dimension."""

  def __init__(self):
    self.chunks: List[Dict[str, torch.Tensor]] = []
    self.n = 0

  def push(self, feats: Dict[str, torch.Tensor]):
    n = next(iter(feats.values())).shape[0]
    if n:
      self.chunks.append(feats)
      self.n += n

  def pop(self, n: int) -> Dict[str, torch.Tensor]:
    allf = _cat(self.chunks)
    head = {k: v[:n] for k, v in allf.items()}
    self.n -= n
    self.chunks = [{k: v[n:] for k, v in allf.items()}] if self.n else []
    return head


class MmtPretrainDataLoader:
  """`MmtPretrainDataLoader(params).load(...)`: an iterator of (inputs, labels) with the keys, shapes and dtypes of
  `input_utils.synthetic_batch(task='pretrain')`.

  params: an `MmtPretrainDataConfig`.  device: where the batches live (a GPU: the side inputs are HIP only).
  shuffle_buffer / example_shuffle_buffer: the record shuffle (host, payloads) and the example shuffle behind the
  matching step (device) -- 4096 in the reference.  `image_data` may hold JPEG or PNG files, mixed at will
  (`feature_pipeline.decode_images`).  entropy: `decode_jpeg_images`'s mode; 'auto' decodes the Huffman scan on the device
  from the blob that is uploaded once; PNG files are inflated on the host and uploaded as scanlines."""

  def __init__(self, params, *, device=None, shuffle_buffer: int = 4096, example_shuffle_buffer: int = 4096,
               entropy: str = 'auto', dense_side_inputs: bool = False, chunk_bytes: int = 1 << 22):
    self.params = params
    self.device = torch.device(device) if device is not None else torch.device('cuda')
    self.shuffle_buffer, self.example_shuffle_buffer = int(shuffle_buffer), int(example_shuffle_buffer)
    self.entropy, self.dense_side_inputs, self.chunk_bytes = entropy, bool(dense_side_inputs), int(chunk_bytes)
    self.field_dict = json.loads(params.text_special_token_field_dict)
    if not isinstance(self.field_dict, dict) or not self.field_dict:
      raise ValueError('text_special_token_field_dict must name at least one field')
    self.names = [params.image_data_field, params.image_key_field] + list(self.field_dict)
    self._vocab = None
    self._key_ids: Dict[bytes, int] = {}

  # ---- stage 1: files (:106-130) ----------------------------------------------------------------------------------
  def files(self) -> List[str]:
    return check_input_patterns(self.params.input_path.split(','))

  def _file_stream(self, rank: int, num_replicas: int) -> Iterator[str]:
    files = self.files()
    if len(files) < num_replicas:
      raise ValueError(f'{len(files)} input files cannot be sharded over {num_replicas} input pipelines')
    rng = random.Random(int(self.params.seed))
    while True:
      order = list(files)
      if self.params.is_training:
        rng.shuffle(order)                                       # every pipeline draws the same order, so the shards are disjoint
      yield from order[rank::num_replicas] if num_replicas > 1 else order
      if not self.params.is_training:
        return

  # ---- stage 2: interleave (:132-135), one record of each of cycle_length files in turn --------------------------------
  def _interleave(self, file_stream) -> Iterator[Tuple[bytes, int, str, int]]:
    def open_next():
      for path in file_stream:
        return ((p, c, path, i) for i, (p, c) in enumerate(records.read_shard(path, self.chunk_bytes)))
      return None
    slots = []
    for _ in range(max(int(self.params.cycle_length), 1)):
      it = open_next()
      if it is None:
        break
      slots.append(it)
    while slots:
      for s in range(len(slots)):
        while slots[s] is not None:
          item = next(slots[s], None)
          if item is not None:
            yield item
            break
          slots[s] = open_next()
      slots = [it for it in slots if it is not None]

  # ---- stage 3: record shuffle (:137-138) ----------------------------------------------------------------------------
  def _shuffle(self, stream, rank: int):
    if not self.params.is_training or self.shuffle_buffer <= 1:
      yield from stream
      return
    rng = random.Random(int(self.params.seed) * 7919 + rank)
    buf = []
    for item in stream:
      if len(buf) < self.shuffle_buffer:
        buf.append(item)
        continue
      i = rng.randrange(len(buf))
      buf[i], item = item, buf[i]
      yield item
    rng.shuffle(buf)
    yield from buf

  # ---- stage 4: decode on the device (:140-150) ---------------------------------------------------------------------
  def vocab(self) -> text_frontend.WordpieceVocab:
    if self._vocab is None:
      self._vocab = text_frontend.WordpieceVocab(self.params.vocab_filename).to(self.device)
    return self._vocab

  def _special(self, token: str) -> int:
    try:
      return self.vocab().id(token)
    except KeyError:
      raise ValueError(f'the vocabulary {self.params.vocab_filename!r} has no token {token!r}') from None

  def _decode(self, group, gen) -> Dict[str, torch.Tensor]:
    """One group of (payload, stored crc, file, index) -> the decoded features of its examples on the device."""
    from . import _lib
    cfg, dev = self.params, self.device
    n = len(group)
    try:
      blob, recs, fields = records.pack_records([g[0] for g in group], [g[1] for g in group], self.names)
    except ValueError as e:
      i = int(str(e).split()[1])
      raise ValueError(f'{group[i][2]}: record {group[i][3]}: {e}') from None
    blob_d = blob.to(dev, non_blocking=True)                    # the one upload of the group's bytes
    bad = records.payload_checksums(blob_d, recs, n).cpu()
    if bool(bad.any()):
      i = int(torch.nonzero(bad)[0])
      raise ValueError(f'{group[i][2]}: record {group[i][3]}: the payload checksum does not match (corrupt record)')
    view = blob.numpy()
    images, image_at, keys, t_off, t_len = [], [], [], [], []
    for i, f in enumerate(fields):
      for j, what in ((0, cfg.image_data_field), (1, cfg.image_key_field)):
        if f[j].kind != _lib.MMT_FIELD_BYTES or f[j].count != 1:
          raise ValueError(f'{group[i][2]}: record {group[i][3]}: feature {what!r} must hold exactly one bytes value')
      images.append(view[f[0].offset:f[0].offset + f[0].length])
      image_at.append(int(f[0].offset))
      key = view[f[1].offset:f[1].offset + f[1].length].tobytes()
      keys.append(self._key_ids.setdefault(key, len(self._key_ids)))
      for j, name in enumerate(self.field_dict, start=2):
        if f[j].kind == _lib.MMT_FIELD_MISSING or (f[j].kind == _lib.MMT_FIELD_BYTES and f[j].count == 0):
          t_off.append(0); t_len.append(0)                       # FixedLenFeature(default_value='')
        elif f[j].kind != _lib.MMT_FIELD_BYTES or f[j].count != 1:
          raise ValueError(f'{group[i][2]}: record {group[i][3]}: text feature {name!r} must hold one bytes value')
        else:
          t_off.append(int(f[j].offset)); t_len.append(int(f[j].length))
    try:
      im = fp.decode_image_features(cfg, images, generator=gen, keep_unnormalized=True, device=dev, entropy=self.entropy,
                                    uploaded=(blob_d, image_at))
    except ValueError as e:
      raise ValueError(f'{group[0][2]} (records from {group[0][3]}): {e}') from None
    meta = lambda v, dt: torch.tensor(v, dtype=dt).to(dev)
    tx = text_frontend.decode_text_features(cfg, self.vocab(), (blob_d, meta(t_off, torch.int64), meta(t_len, torch.int32)))
    P2 = im['patch_embeddings'].shape[1]
    ptok = torch.empty(n, 2 + P2, dtype=torch.int32, device=dev)
    ptok[:, 0], ptok[:, 1] = self._special('[CLS]'), self._special('[PATCH]')
    ptok[:, 2:] = input_utils.PATCH_START_UNUSED_INDEX + torch.arange(P2, dtype=torch.int32, device=dev)
    return {'patch_token_ids': ptok, 'patch_embeddings': im['patch_embeddings'],
            'unnormalized_patch_embeddings': im['unnormalized_patch_embeddings'],
            'text_token_ids': tx['text_token_ids'], 'num_text_wordpieces': tx['num_text_wordpieces'],
            'text_word_start': tx['text_word_start'], 'image_key': meta(keys, torch.int64)}

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
    cfg, dev = self.params, self.device
    S = cfg.max_seq_len
    B, W = ex['patch_token_ids'].shape
    n_image = torch.full((B,), W, device=dev, dtype=torch.int32)
    n_text = ex['num_text_wordpieces'].to(torch.int32)
    pattern = input_utils.attention_pattern_from_config(cfg)
    inputs = {'word_ids': torch.cat([ex['patch_token_ids'], ex['text_token_ids']], dim=1),       # make_word_ids_features
              'patch_embeddings': ex['patch_embeddings']}
    if self.dense_side_inputs:
      si = side_inputs(pattern, n_image, n_text, S,
                       materialize_pattern=pattern.local_radius < S or pattern.n_global > 0 or pattern.grid_radius > 0)
      inputs.update(si)
      if si['relative_att_ids'] is None:
        inputs.pop('relative_att_ids')
    else:
      si = side_inputs(pattern, n_image, n_text, S, want_mask=False, want_ids=False)
      inputs['segment_ids'] = si['segment_ids']
      inputs['attention_pattern'] = pattern
      inputs['valid_len'] = (n_image + n_text).to(torch.int32)
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
      N = self.example_shuffle_buffer
      if not (with_itm and training) or N <= 1:
        yield from matched()
        return
      held, count = None, 0
      for ex in matched():
        m = next(iter(ex.values())).shape[0]
        while m:
          if count < N:                                          # filling
            take = min(N - count, m)
            head = {k: v[:take] for k, v in ex.items()}
            held = head if held is None else _cat([held, head])
            count += take
          else:                                                  # full: every newcomer takes a random place and frees its holder
            take = min(m, N)
            slots = torch.randperm(N, generator=gen, device=dev)[:take]
            yield {k: v[slots] for k, v in held.items()}
            for k in held:
              held[k][slots] = ex[k][:take]
          ex = {k: v[take:] for k, v in ex.items()}
          m -= take
      if held is not None:
        order = torch.randperm(count, generator=gen, device=dev)
        yield {k: v[order] for k, v in held.items()}

    def batches():                                               # :221
      pool = _Pool()
      for ex in shuffled():
        ex.pop('image_key', None)
        pool.push(ex)
        while pool.n >= B:
          yield self._finish(pool.pop(B), with_itm)
      if pool.n and not training:
        yield self._finish(pool.pop(pool.n), with_itm)

    return batches()
