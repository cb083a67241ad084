"""The stages every loader on TFRecord shards shares ("Records"): files, interleave, record
shuffle, the upload of a group of records with its checksums, the field lookup, the example shuffle on the device, and
the word ids and side inputs of a batch.  `MmtPretrainDataLoader`, `MmtClassificationDataLoader` and
`MmtRetrievalDataLoader` derive from `RecordStages`; each adds its own decode and its own stage order.

The host does files, frames and field lookup; the device does checksums and everything behind them."""
from __future__ import annotations

import glob
import json
import os
import random
import time
from typing import Dict, Iterator, List, Optional, Tuple

import torch

from . import input_utils, records, text_frontend
from .ops import side_inputs


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


def _where(group, i: int) -> str:
  """A record of a group of (payload, stored crc, file, index), as the error texts name it."""
  return f'{group[i][2]}: record {group[i][3]}'


def one_bytes_field(group, i: int, f, what: str) -> Tuple[int, int]:
  """(offset, length) of a feature that must hold exactly one bytes value."""
  from . import _lib
  if f.kind != _lib.MMT_FIELD_BYTES or f.count != 1:
    raise ValueError(f'{_where(group, i)}: feature {what!r} must hold exactly one bytes value')
  return int(f.offset), int(f.length)


def text_field(group, i: int, f, name: str) -> Tuple[int, int]:
  """(offset, length) of a text feature; a missing or empty one is '' (FixedLenFeature(default_value=''))."""
  from . import _lib
  if f.kind == _lib.MMT_FIELD_MISSING or (f.kind == _lib.MMT_FIELD_BYTES and f.count == 0):
    return 0, 0
  if f.kind != _lib.MMT_FIELD_BYTES or f.count != 1:
    raise ValueError(f'{_where(group, i)}: text feature {name!r} must hold one bytes value')
  return int(f.offset), int(f.length)


def one_int64_field(group, i: int, f, what: str) -> int:
  """The value of a feature that must hold exactly one int64 value (FixedLenFeature([], tf.int64))."""
  from . import _lib
  if f.kind == _lib.MMT_FIELD_MISSING:
    raise ValueError(f'{_where(group, i)}: feature {what!r} is missing')
  if f.kind != _lib.MMT_FIELD_INT64 or f.count != 1:
    raise ValueError(f'{_where(group, i)}: feature {what!r} must hold exactly one int64 value')
  return int(f.int_value)


class RecordStages:
  """What the loaders on records have in common.  params: the data config.  device: where the batches live (a GPU: the
  side inputs are HIP only; the host stages and the field lookup also run with 'cpu').  shuffle_buffer: the record
  shuffle (host, payloads), 4096 in the reference."""

  def __init__(self, params, *, device=None, shuffle_buffer: int = 4096, entropy: str = 'auto',
               dense_side_inputs: bool = False, chunk_bytes: int = 1 << 22):
    self.params = params
    self.device = torch.device(device) if device is not None else torch.device('cuda')
    self.shuffle_buffer = int(shuffle_buffer)
    self.entropy, self.dense_side_inputs, self.chunk_bytes = entropy, bool(dense_side_inputs), int(chunk_bytes)
    self.field_dict = json.loads(params.text_special_token_field_dict)
    if not isinstance(self.field_dict, dict) or not self.field_dict:
      raise ValueError('text_special_token_field_dict must name at least one field')
    self._vocab = None
    self._key_ids: Dict[bytes, int] = {}
    if int(getattr(params, 'pack_rows', 0) or 0) < 0 or int(getattr(params, 'pack_row_len', 0) or 0) < 0:
      raise ValueError('pack_rows and pack_row_len must not be negative')
    if int(getattr(params, 'prefetch_buffer_size', 0) or 0) < 0:
      raise ValueError('prefetch_buffer_size must not be negative')
    if int(getattr(params, 'pack_rows', 0) or 0) and self.dense_side_inputs:
      raise ValueError('pack_rows takes the structured side inputs: dense_side_inputs must be off')
    # the packing stage's own cost: batches packed, and the seconds spent waiting for their `consumed` words
    self.pack_batches, self.pack_wait_seconds = 0, 0.0

  # ---- stage 1: files ------------------------------------------------------------------------------------------------
  def files(self, input_path: Optional[str] = None) -> List[str]:
    return check_input_patterns((self.params.input_path if input_path is None else input_path).split(','))

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

  # ---- stage 2: interleave, one record of each of cycle_length files in turn -------------------------------------------
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

  # ---- stage 3: record shuffle -------------------------------------------------------------------------------------------
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

  # ---- stage 4: a group of records on the device --------------------------------------------------------------------
  def vocab(self) -> text_frontend.WordpieceVocab:
    if self._vocab is None:
      self._vocab = text_frontend.WordpieceVocab(self.params.vocab_filename).to(self.device)
    return self._vocab

  def _special(self, token: str) -> int:
    try:
      return self.vocab().id(token)
    except KeyError:
      raise ValueError(f'the vocabulary {self.params.vocab_filename!r} has no token {token!r}') from None

  def _open_group(self, group, names):
    """One group of (payload, stored crc, file, index): the payloads packed into one blob, its one upload, the payload
    checksums verified on the blob's device, and every named feature's place.  Returns (blob, blob on the device,
    fields); fields[i][j] is the `ExampleField` of names[j] in record i."""
    n = len(group)
    try:
      blob, recs, fields = records.pack_records([g[0] for g in group], [g[1] for g in group], names)
    except ValueError as e:
      i = int(str(e).split()[1])
      raise ValueError(f'{_where(group, i)}: {e}') from None
    blob_d = blob.to(self.device, non_blocking=True)             # the one upload of the group's bytes
    bad = records.payload_checksums(blob_d, recs, n).cpu()
    if bool(bad.any()):
      i = int(torch.nonzero(bad)[0])
      raise ValueError(f'{_where(group, i)}: the payload checksum does not match (corrupt record)')
    return blob, blob_d, fields

  def _image_key_text_fields(self, group, view, fields):
    """The lookup of a record that carries image_data_field, image_key_field and the text fields, in this order in
    `fields`: (image byte views, their offsets in the blob, key ids, text offsets, text lengths)."""
    cfg = self.params
    images, image_at, keys, t_off, t_len = [], [], [], [], []
    for i, f in enumerate(fields):
      spans = [one_bytes_field(group, i, f[j], what) for j, what in ((0, cfg.image_data_field), (1, cfg.image_key_field))]
      images.append(view[spans[0][0]:spans[0][0] + spans[0][1]])
      image_at.append(spans[0][0])
      key = view[spans[1][0]:spans[1][0] + spans[1][1]].tobytes()
      keys.append(self._key_ids.setdefault(key, len(self._key_ids)))
      for j, name in enumerate(self.field_dict, start=2):
        off, length = text_field(group, i, f[j], name)
        t_off.append(off); t_len.append(length)
    return images, image_at, keys, t_off, t_len

  def _meta(self, values, dtype) -> torch.Tensor:
    return torch.tensor(values, dtype=dtype).to(self.device)

  def _decode_texts(self, blob_d, t_off, t_len) -> Dict[str, torch.Tensor]:
    return text_frontend.decode_text_features(self.params, self.vocab(),
                                              (blob_d, self._meta(t_off, torch.int64), self._meta(t_len, torch.int32)))

  def _patch_token_ids(self, n: int, P2: int) -> torch.Tensor:
    """[CLS] [PATCH] patch_1 .. patch_{P^2}, int32 [n, 2 + P^2] (data_utils.py:224-231)."""
    ptok = torch.empty(n, 2 + P2, dtype=torch.int32, device=self.device)
    ptok[:, 0], ptok[:, 1] = self._special('[CLS]'), self._special('[PATCH]')
    ptok[:, 2:] = input_utils.PATCH_START_UNUSED_INDEX + torch.arange(P2, dtype=torch.int32, device=self.device)
    return ptok

  # ---- the example shuffle, on the device --------------------------------------------------------------------------------
  def _example_shuffle(self, chunks, gen, N: int):
    """A shuffle buffer of N examples over a stream of chunks (dicts of tensors with a common leading dimension)."""
    dev = self.device
    if N <= 1:
      yield from chunks
      return
    held, count = None, 0
    for ex in chunks:
      m = next(iter(ex.values())).shape[0]
      while m:
        if count < N:                                            # filling
          take = min(N - count, m)
          head = {k: v[:take] for k, v in ex.items()}
          held = head if held is None else _cat([held, head])
          count += take
        else:                                                    # full: every newcomer takes a random place and frees its holder
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

  # ---- word ids and side inputs, as synthetic_batch builds them ---------------------------------------------------------
  def _encoder_inputs(self, ex) -> Dict:
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
      if dev.type == 'cuda':
        inputs['segment_ids'] = side_inputs(pattern, n_image, n_text, S, want_mask=False, want_ids=False)['segment_ids']
      else:     # `make_segment_ids` (data_utils.py:350-361) in torch, for the host stages: 1 image part, 2 text part, 0 boundary / pad
        pos = torch.arange(S, device=dev)[None]
        inputs['segment_ids'] = ((pos < W).to(torch.int32) + 2 * ((pos > W) & (pos < W + n_text[:, None])).to(torch.int32))
      inputs['attention_pattern'] = pattern
      inputs['valid_len'] = (n_image + n_text).to(torch.int32)
    return inputs

  # ---- the last stage when `pack_rows` is set: short examples into long rows -------------------------------------------------
  def _maybe_packed(self, batches, B: int):
    return self._packed(batches, B) if int(getattr(self.params, 'pack_rows', 0) or 0) else batches

  def _packed(self, batches, B: int):
    """Packs the stream of unpacked (inputs, labels) batches into batches of `pack_rows` rows of `pack_row_len` positions
    (`input_utils.pack_batch`).  The examples in hand form a pool on the device, in arrival order.  `max_examples` is the
    per-replica batch size times the examples a row can hold, capped at the kernel's limit.  As soon as the pool holds as
    many examples as a batch could take at the most (max_examples, or rows times the examples a row can hold) a batch
    packs a prefix of the pool, the one `consumed` word is read back -- the stage's only host wait -- and the
    rest stays at the front for the next batch: nothing is dropped, repeated or reordered.  When a finite pass ends
    (is_training off) the remainder goes out in as many last batches as it takes."""
    cfg = self.params
    rows = int(cfg.pack_rows)
    row_len = int(getattr(cfg, 'pack_row_len', 0) or 0) or int(cfg.max_seq_len)
    if row_len < int(cfg.max_seq_len):
      raise ValueError(f'pack_row_len {row_len} is shorter than max_seq_len {cfg.max_seq_len}')
    M = input_utils.pack_max_examples(cfg, B, row_len)
    need = min(M, rows * input_utils.pack_examples_per_row(cfg, row_len))     # more examples in hand cannot change the batch
    pool_in, pool_lab = _Pool(), _Pool()
    constants = {}

    def pack_one():
      n = min(pool_in.n, M)
      all_in, all_lab = _cat(pool_in.chunks), _cat(pool_lab.chunks)
      head_in = {k: v[:n] for k, v in all_in.items()}
      head_in.update(constants)
      packed_in, packed_lab, consumed = input_utils.pack_batch(head_in, {k: v[:n] for k, v in all_lab.items()}, rows, row_len, M)
      t0 = time.perf_counter()
      taken = int(consumed)                                      # the read-back: waits for the pack (and all before it)
      self.pack_wait_seconds += time.perf_counter() - t0
      self.pack_batches += 1
      for pool, everything in ((pool_in, all_in), (pool_lab, all_lab)):
        pool.n -= taken
        pool.chunks = [{k: v[taken:] for k, v in everything.items()}] if pool.n else []
      return packed_in, packed_lab

    for inputs, labels in batches:
      constants = {k: v for k, v in inputs.items() if not torch.is_tensor(v)}
      pool_in.push({k: v for k, v in inputs.items() if torch.is_tensor(v)})
      pool_lab.push(labels)
      while pool_in.n >= need:
        yield pack_one()
    while pool_in.n and not cfg.is_training:                     # a training stream that ends drops its remainder, as the unpacked loaders do
      yield pack_one()
