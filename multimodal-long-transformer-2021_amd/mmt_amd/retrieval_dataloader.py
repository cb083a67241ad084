"""Retrieval loader on TFRecord shards (`MmtRetrievalDataLoader`, src/data/retrieval_dataloader.py:80-246): fills a
`retrieval.RetrievalSets` from files.  Two modes, chosen as the reference chooses them (:116):

  separate sets    `input_path` empty: `image_input_path` records carry `image_index` (or `index`, data_utils.py:190-193)
                   and the image; `text_input_path` records carry `text_index`, `gt_image_index` and the text fields.
                   Every image meets every text (`retrieval.pair_entries`).
  pairs in records `input_path` set: every record carries all of the above and lists one pair.  An image that many
                   records list is decoded once: images are keyed by `image_index` and texts by `text_index` on the
                   host, before anything is uploaded, and only the first record of an index is decoded.  The bytes of
                   a repeated index are NOT compared with those of its first record, and the payload checksum of a
                   record of which nothing is decoded is not verified.  A record that brings both a new image and a
                   new text is uploaded once for each side.

Either way the files are walked twice: once on the host for the ids alone (`records.example_fields`), which gives the
table sizes, and once to decode, in chunks of `chunk` records, into tables allocated once.  The files are taken in sorted
order and interleaved over `cycle_length` files as the reference does (:124-127, :154-161), without a shuffle; decode
runs with is_training false (the loader is "for prediction only", :104).  DESIGN.md section 4, "Records: fine-tuning and
retrieval"."""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import feature_pipeline as fp
from . import records
from .record_stages import RecordStages, _where, one_bytes_field, one_int64_field, text_field
from .retrieval import RetrievalSets, num_shard_pairs, pair_entries


def first_appearance(ids: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
  """(unique int64 [U], entry int32 [n]): the distinct ids in the order in which they first appear, and for every item
  the place of its id among them, so that unique[entry[k]] == ids[k]."""
  ids = np.asarray(ids, dtype=np.int64).reshape(-1)
  if ids.size == 0:
    return ids.copy(), np.zeros(0, dtype=np.int32)
  values, first, inverse = np.unique(ids, return_index=True, return_inverse=True)      # sorted values
  order = np.argsort(first, kind='stable')                     # sorted place -> place by first appearance
  place = np.empty(len(values), dtype=np.int64)
  place[order] = np.arange(len(values))
  return values[order], place[inverse.reshape(-1)].astype(np.int32)


class MmtRetrievalDataLoader(RecordStages):
  """params: an `MmtRetrievalDataConfig`.  device: where the tables live.  chunk: records decoded at a time.

    sets()    the `RetrievalSets`, built at the first call
    pairs()   None (every image meets every text), or (image_entry, text_entry): int32 numpy arrays, the rows of the
              tables each record lists, in record order
    load()    batches of (inputs, labels) in the reference's contract (`RetrievalSets.materialize`)
    images_decoded / texts_decoded   how many records were decoded for each table"""

  def __init__(self, params, *, device=None, chunk: int = 64, entropy: str = 'auto', chunk_bytes: int = 1 << 22):
    super().__init__(params, device=device, entropy=entropy, chunk_bytes=chunk_bytes)
    self.chunk = int(chunk)
    if self.chunk < 1:
      raise ValueError('chunk must be positive')
    self.eval_params = dataclasses.replace(params, is_training=False)
    self._sets: Optional[RetrievalSets] = None
    self._pairs = None
    self.images_decoded = self.texts_decoded = 0

  # ---- the record streams ------------------------------------------------------------------------------------------------
  def _records(self, input_path: str):
    return self._interleave(iter(self.files(input_path)))

  def _image_names(self):
    return ['image_index', 'index', self.params.image_data_field]

  def _text_names(self):
    return ['text_index', 'gt_image_index'] + list(self.field_dict)

  @staticmethod
  def _image_index(item, f_image_index, f_index) -> int:
    from . import _lib
    if f_image_index.kind == _lib.MMT_FIELD_MISSING and f_index.kind != _lib.MMT_FIELD_MISSING:
      return one_int64_field([item], 0, f_index, 'index')
    return one_int64_field([item], 0, f_image_index, 'image_index')

  def _scan_ids(self, input_path: str, image: bool, text: bool):
    """The host pass: (image_index, text_index, gt_image_index) lists over the records of a stream; a side not asked
    for stays empty."""
    names = (self._image_names()[:2] if image else []) + (self._text_names()[:2] if text else [])
    img, txt, gt = [], [], []
    for item in self._records(input_path):
      try:
        f = records.example_fields(item[0], names)
      except ValueError as e:
        raise ValueError(f'{_where([item], 0)}: {e}') from None
      at = 0
      if image:
        img.append(self._image_index(item, f[0], f[1]))
        at = 2
      if text:
        txt.append(one_int64_field([item], 0, f[at], 'text_index'))
        gt.append(one_int64_field([item], 0, f[at + 1], 'gt_image_index'))
    return img, txt, gt

  # ---- decode into the tables --------------------------------------------------------------------------------------------
  def _decode_images(self, group, rows, table):
    blob, blob_d, fields = self._open_group(group, self._image_names())
    view = blob.numpy()
    images, image_at = [], []
    for i, f in enumerate(fields):
      off, length = one_bytes_field(group, i, f[2], self.params.image_data_field)
      images.append(view[off:off + length])
      image_at.append(off)
    try:
      im = fp.decode_image_features(self.eval_params, images, keep_unnormalized=False, device=self.device, entropy=self.entropy,
                                    uploaded=(blob_d, image_at))
    except ValueError as e:
      raise ValueError(f'{group[0][2]} (records from {group[0][3]}): {e}') from None
    table[torch.as_tensor(rows, device=self.device)] = im['patch_embeddings']
    self.images_decoded += len(group)

  def _decode_text_rows(self, group, rows, ids_table, count_table):
    blob, blob_d, fields = self._open_group(group, self._text_names())
    t_off, t_len = [], []
    for i, f in enumerate(fields):
      for j, name in enumerate(self.field_dict, start=2):
        off, length = text_field(group, i, f[j], name)
        t_off.append(off); t_len.append(length)
    tx = self._decode_texts(blob_d, t_off, t_len)
    rows = torch.as_tensor(rows, device=self.device)
    ids_table[rows] = tx['text_token_ids']
    count_table[rows] = tx['num_text_wordpieces']
    self.texts_decoded += len(group)

  def _fill(self, input_path: str, image_rows, text_rows, tables):
    """The decode pass over a stream.  image_rows / text_rows: {place of a record in the stream: row of its table} for
    the records to decode (None: that side is not in this stream)."""
    patches, text_ids, text_count = tables
    iq, ir, tq, tr = [], [], [], []
    for at, item in enumerate(self._records(input_path)):
      if image_rows is not None and at in image_rows:
        iq.append(item); ir.append(image_rows[at])
        if len(iq) == self.chunk:
          self._decode_images(iq, ir, patches)
          iq, ir = [], []
      if text_rows is not None and at in text_rows:
        tq.append(item); tr.append(text_rows[at])
        if len(tq) == self.chunk:
          self._decode_text_rows(tq, tr, text_ids, text_count)
          tq, tr = [], []
    if iq:
      self._decode_images(iq, ir, patches)
    if tq:
      self._decode_text_rows(tq, tr, text_ids, text_count)

  def _check_count(self, what: str, configured: int, read: int):
    if int(configured) > 0 and int(configured) != read:
      raise ValueError(f'{what} is {int(configured)}, but {read} were read')

  def sets(self) -> RetrievalSets:
    if self._sets is not None:
      return self._sets
    cfg, dev = self.params, self.device
    paired = bool(cfg.input_path)
    if paired:                                                   # :116-138
      img, txt, gt = self._scan_ids(cfg.input_path, True, True)
      image_index, image_entry = first_appearance(img)
      text_index, text_entry = first_appearance(txt)
      _, image_first = np.unique(image_entry, return_index=True)       # the record that brings row r of a table
      _, text_first = np.unique(text_entry, return_index=True)
      gt_index = np.asarray(gt, dtype=np.int64)[text_first]
    else:                                                        # :139-186
      self.files(cfg.image_input_path)                           # both patterns must match before either is read
      self.files(cfg.text_input_path)
      image_index = np.asarray(self._scan_ids(cfg.image_input_path, True, False)[0], dtype=np.int64)
      _, txt, gt = self._scan_ids(cfg.text_input_path, False, True)
      text_index, gt_index = np.asarray(txt, dtype=np.int64), np.asarray(gt, dtype=np.int64)
      image_first, text_first = np.arange(len(image_index)), np.arange(len(text_index))
    self._check_count('num_image_examples', cfg.num_image_examples, len(image_index))
    self._check_count('num_text_examples', cfg.num_text_examples, len(text_index))
    n_patch = (int(cfg.image_size) // int(cfg.patch_size)) ** 2
    Lt = int(cfg.max_seq_len) - 2 - n_patch
    if Lt < 1:
      raise ValueError('max_seq_len leaves no room for text')
    tables = (torch.zeros(len(image_index), n_patch, int(cfg.patch_size) ** 2 * 3, dtype=torch.float32, device=dev),
              torch.zeros(len(text_index), Lt, dtype=torch.int32, device=dev),
              torch.zeros(len(text_index), dtype=torch.int32, device=dev))
    image_rows = {int(at): r for r, at in enumerate(image_first)}
    text_rows = {int(at): r for r, at in enumerate(text_first)}
    self.images_decoded = self.texts_decoded = 0
    if paired:
      self._fill(cfg.input_path, image_rows, text_rows, tables)
    else:
      self._fill(cfg.image_input_path, image_rows, None, tables)
      self._fill(cfg.text_input_path, None, text_rows, tables)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    sets = RetrievalSets(data_cfg=cfg, patch_embeddings=tables[0], image_index=to_dev(image_index),
                         prefix_ids=self._patch_token_ids(1, n_patch)[0], text_token_ids=tables[1],
                         num_text_wordpieces=tables[2], text_index=to_dev(text_index), gt_image_index=to_dev(gt_index))
    self._pairs = (image_entry, text_entry) if paired else None
    self._sets = sets
    return sets

  def pairs(self):
    self.sets()
    return self._pairs

  def load(self, rank: int = 0, num_replicas: int = 1, batch_size: Optional[int] = None):
    """An iterator of (inputs, labels): `RetrievalSets.materialize` over windows of batch_size pairs of the pipeline's
    share of the pair list -- the pairs p with p % num_replicas == rank, sharded after enumeration as the reference
    does (:204-207).  The last short batch is kept unless the config says drop_remainder (:241-242).  One pass."""
    cfg = self.params
    B = int(batch_size or max(1, cfg.global_batch_size // num_replicas))
    sets, listed = self.sets(), self.pairs()
    shard = (int(rank), int(num_replicas))
    if listed is None:
      total = num_shard_pairs(sets.num_images, sets.num_texts, shard)
    else:
      num_shard_pairs(0, 0, shard)                               # the shard check
      ie_all = torch.from_numpy(listed[0][shard[0]::shard[1]].copy()).to(self.device)
      te_all = torch.from_numpy(listed[1][shard[0]::shard[1]].copy()).to(self.device)
      total = ie_all.shape[0]

    def batches():
      for first in range(0, total, B):
        count = min(B, total - first)
        if count < B and cfg.drop_remainder:
          return
        if listed is None:
          yield sets.materialize(*pair_entries(sets.num_images, sets.num_texts, first, count, shard, device=self.device))
        else:
          yield sets.materialize(ie_all[first:first + count], te_all[first:first + count])

    return self._maybe_packed(batches(), B)
