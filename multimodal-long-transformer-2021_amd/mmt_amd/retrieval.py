"""Retrieval evaluation: every image of a set scored against every text of a set, on the device.

The reference reads image records and text records separately and "enumerates all possible combinations on the fly"
(`src/data/retrieval_dataloader.py:139-195`), feeds every pair through the classification model
(`src/tasks/classification.py:256-334`) and turns the scores into recall@k (`src/prediction_helper.py:30-118`).  Here the
two sets stay resident in device memory (`RetrievalSets`), a batch of pairs is two int32 entries per row
(`pair_entries`), the embedding assembly gathers straight from the tables (`MmtEncoder.embed_pairs`,
`mmt_embed_fwd_pairs`), and the scores land in one [I, T] matrix (`PairScorer`) from which recall@k and the reference's
two result files are computed without one Python object per pair (`recall_at_k_from_scores`,
`write_results_from_scores`).  `RetrievalSets.materialize` builds the batch the reference's loader would emit for the
same pairs: the route that existed before, and the yardstick of this one.  `evaluate_from_records` fills the sets from
TFRecord files (`retrieval_dataloader.MmtRetrievalDataLoader`) and goes on to recall@k and the result files."""
from __future__ import annotations

import collections
import csv
import dataclasses
import json
import os
import warnings
from typing import Any, Optional, Sequence, Tuple

import numpy as np
import torch

from . import feature_pipeline, predict, prefetch
from .input_utils import attention_pattern_from_config

# `graph=None` with MMT_STEP_GRAPH unset, as for the train step: on.  Two measurements of this code show the replayed
# forward ahead of the eager one outside the eager route's own spread ("Retrieval: all pairs from
# separate sets"); a capture that raises falls back to eager batches.
GRAPH_DEFAULT = True


@dataclasses.dataclass
class RetrievalSets:
  """An image set and a text set, resident on one device.

    patch_embeddings     [I, P^2, 3 * patch^2]  patch features of every image
    image_index          int64 [I]              the images' ids (unique)
    prefix_ids           int32 [2 + P^2]        the image-side word ids every pair shares: [CLS] [PATCH] patch ids
    text_token_ids       int32 [T, Lt]          zero-padded text ids, Lt = max_seq_len - 2 - P^2 (data_utils.py:272-276)
    num_text_wordpieces  int32 [T]              text lengths, in [0, Lt]
    text_index           int64 [T]              the texts' ids (unique)
    gt_image_index       int64 [T]              id of every text's ground-truth image

  Validated once, on the host, at construction."""
  data_cfg: Any
  patch_embeddings: torch.Tensor
  image_index: torch.Tensor
  prefix_ids: torch.Tensor
  text_token_ids: torch.Tensor
  num_text_wordpieces: torch.Tensor
  text_index: torch.Tensor
  gt_image_index: torch.Tensor

  def __post_init__(self):
    c = self.data_cfg
    P = c.image_size // c.patch_size
    n_patch, F = P * P, c.patch_size ** 2 * 3
    Lt = c.max_seq_len - 2 - n_patch
    if Lt < 1:
      raise ValueError('max_seq_len leaves no room for text')
    pe = self.patch_embeddings
    if pe.dim() != 3 or tuple(pe.shape[1:]) != (n_patch, F) or not pe.is_floating_point():
      raise ValueError(f'patch_embeddings must be a floating [I, {n_patch}, {F}] tensor, got {tuple(pe.shape)}')
    I = pe.shape[0]
    tt = self.text_token_ids
    if tt.dim() != 2 or tt.shape[1] != Lt or tt.dtype != torch.int32:
      raise ValueError(f'text_token_ids must be int32 [T, {Lt}], got {tt.dtype} {tuple(tt.shape)}')
    T = tt.shape[0]
    if I < 1 or T < 1:
      raise ValueError('both sets must hold at least one record')
    for name, t, shape, dtype in (('image_index', self.image_index, (I,), torch.int64),
                                  ('prefix_ids', self.prefix_ids, (2 + n_patch,), torch.int32),
                                  ('num_text_wordpieces', self.num_text_wordpieces, (T,), torch.int32),
                                  ('text_index', self.text_index, (T,), torch.int64),
                                  ('gt_image_index', self.gt_image_index, (T,), torch.int64)):
      if tuple(t.shape) != shape or t.dtype != dtype:
        raise ValueError(f'{name} must be {dtype} {list(shape)}, got {t.dtype} {list(t.shape)}')
    dev = pe.device
    for f in dataclasses.fields(self)[1:]:
      t = getattr(self, f.name)
      if t.device != dev:
        raise ValueError(f'{f.name} is on {t.device}, patch_embeddings on {dev}')
      setattr(self, f.name, t.contiguous())
    for name in ('image_index', 'text_index'):
      v = getattr(self, name).cpu().numpy()
      if len(np.unique(v)) != len(v):
        raise ValueError(f'{name} holds duplicate ids')
    n = self.num_text_wordpieces.cpu().numpy()
    if len(n) and (n.min() < 0 or n.max() > Lt):
      raise ValueError(f'num_text_wordpieces must lie in [0, {Lt}]')

  @property
  def num_images(self) -> int:
    return self.patch_embeddings.shape[0]

  @property
  def num_texts(self) -> int:
    return self.text_token_ids.shape[0]

  @property
  def device(self):
    return self.patch_embeddings.device

  def materialize(self, image_entry, text_entry):
    """The (inputs, labels) the reference's loader emits for the pairs (image_entry[b], text_entry[b]): `word_ids`,
    `segment_ids`, `patch_embeddings`, `attention_pattern`, `valid_len` and the three index tensors; `label_ids` and
    `label_weights` from `feature_pipeline.make_retrieval_labels`.  An entry outside its table (the -1 padding of
    `pair_entries`) gives zero patches / an empty text and index -1."""
    dev = self.device
    ie = torch.as_tensor(image_entry, device=dev).long()
    te = torch.as_tensor(text_entry, device=dev).long()
    I, T = self.num_images, self.num_texts
    n_img, Lt = self.prefix_ids.shape[0], self.text_token_ids.shape[1]
    S, B = n_img + Lt, ie.shape[0]
    i_ok, t_ok = (ie >= 0) & (ie < I), (te >= 0) & (te < T)
    ic, tc = ie.clamp(0, I - 1), te.clamp(0, T - 1)
    text = torch.where(t_ok[:, None], self.text_token_ids[tc], torch.zeros_like(self.text_token_ids[:1]))
    n_text = torch.where(t_ok, self.num_text_wordpieces[tc].clamp(0, Lt), torch.zeros_like(self.num_text_wordpieces[:1]))
    pos = torch.arange(S, device=dev)[None]
    patches = self.patch_embeddings[ic]
    minus1 = torch.full_like(ie, -1)
    inputs = {
        'word_ids': torch.cat([self.prefix_ids[None].expand(B, n_img), text], 1).contiguous(),
        # `make_segment_ids` (data_utils.py:350-361): 1 image part, 2 text part, 0 boundary / pad
        'segment_ids': ((pos < n_img).to(torch.int32)
                        + 2 * ((pos > n_img) & (pos < n_img + n_text[:, None])).to(torch.int32)),
        'patch_embeddings': torch.where(i_ok[:, None, None], patches, torch.zeros_like(patches[:1, :1])),
        'attention_pattern': attention_pattern_from_config(self.data_cfg),
        'valid_len': (n_img + n_text).to(torch.int32),
        'image_index': torch.where(i_ok, self.image_index[ic], minus1),
        'text_index': torch.where(t_ok, self.text_index[tc], minus1),
        'gt_image_index': torch.where(t_ok, self.gt_image_index[tc], minus1),
    }
    lab = feature_pipeline.make_retrieval_labels(
        {'image_index': inputs['image_index'], 'gt_image_index': inputs['gt_image_index']},
        pos_weight=float(getattr(self.data_cfg, 'pos_weight', 1.0)))
    return inputs, {'label_ids': lab['label_ids'], 'label_weights': lab['label_weights']}


def num_shard_pairs(n_images: int, n_texts: int, shard=(0, 1)) -> int:
  sid, n = int(shard[0]), int(shard[1])
  if n < 1 or not 0 <= sid < n:
    raise ValueError(f'shard {shard}: want (id, n) with 0 <= id < n')
  return max(0, (n_images * n_texts - sid + n - 1) // n)


def pair_entries(n_images: int, n_texts: int, first: int, count: int, shard=(0, 1), device=None):
  """(image_entry, text_entry), int32 [count]: pairs `first .. first + count - 1` of a shard's list.  Pair p = i * T + t,
  image-major (the order of the loader's own comment; consecutive rows share the image's patch rows); shard (id, n) is
  `dataset.shard(n, id)`: the pairs with p % n == id, in rising order.  Past the end of the list the entries are -1."""
  total = num_shard_pairs(n_images, n_texts, shard)
  sid, n = int(shard[0]), int(shard[1])
  k = torch.arange(int(first), int(first) + int(count), dtype=torch.int64, device=device)
  p = sid + k * n
  ok = (k >= 0) & (k < total)
  minus1 = torch.full_like(p, -1)
  T = max(int(n_texts), 1)
  ie = torch.where(ok, torch.div(p, T, rounding_mode='floor'), minus1).to(torch.int32)
  te = torch.where(ok, p % T, minus1).to(torch.int32)
  return ie, te


def scores_from_logits(logits: torch.Tensor) -> torch.Tensor:
  """One score per pair, the rule of `predict.predict` (classification.py:256-334): 1 class sigmoid, 2 classes the
  softmax probability of class 1, more the argmax.  float32 [B]."""
  logits = logits.float()
  num_classes = logits.shape[-1] if logits.dim() > 1 else 1
  if num_classes == 1:
    return torch.sigmoid(logits.reshape(-1))
  if num_classes == 2:
    return torch.softmax(logits, dim=1)[:, 1]
  return torch.argmax(logits, dim=1).float()


class PairScorer:
  """Scores pairs of a `RetrievalSets` with a classification model.  One batch is a fixed [batch_size] pair of entry
  buffers; the forward reads them, so after one eager batch it can be captured once as a HIP graph and replayed for
  every following batch, the padded tail included.  `graph`: True / False, or None = the MMT_STEP_GRAPH switch as the
  train step reads it (0 / 1), `GRAPH_DEFAULT` when unset.  A capture that raises falls back to eager batches with one
  warning.  `close()` drops the graph.

  The scorer owns the projected image table: a buffer it allocates once and rewrites in place, with the model's current
  projection weights, at the start of every `score_all` / `score_pairs` (64 images against tens of thousands of
  forwards).  So weights written between two calls -- by an optimizer step, a checkpoint restore -- are seen, and the
  address a recorded graph reads stays valid for as long as the scorer lives."""

  def __init__(self, task, model, sets: RetrievalSets, batch_size: int, logits_key: str = 'itm_logits',
               graph: Optional[bool] = None):
    self.task, self.model, self.sets, self.logits_key = task, model, sets, logits_key
    self.batch_size = int(batch_size)
    if self.batch_size < 1:
      raise ValueError('batch_size must be positive')
    dev = sets.device
    if graph is None:
      env = os.environ.get('MMT_STEP_GRAPH')
      graph = GRAPH_DEFAULT if env is None else env != '0'
    self.use_graph = bool(graph) and dev.type == 'cuda'
    self.pattern = attention_pattern_from_config(sets.data_cfg)
    self.image_entry = torch.full((self.batch_size,), -1, dtype=torch.int32, device=dev)
    self.text_entry = torch.full((self.batch_size,), -1, dtype=torch.int32, device=dev)
    self.graph = None
    self.sync_words = None
    self.out = None
    self._eager_done = False
    from .encoder import MmtEncoder
    self.encoder = next(m for m in model.modules() if isinstance(m, MmtEncoder))
    self.patch_proj = None

  def _refresh_projection(self):
    self.patch_proj = self.encoder.project_image_table(self.sets, out=self.patch_proj)

  @torch.no_grad()
  def _forward(self, image_entry, text_entry) -> torch.Tensor:
    outputs = self.model(pairs=(self.sets, image_entry, text_entry, self.patch_proj), attention_pattern=self.pattern,
                         training=False)
    if self.logits_key not in outputs:
      raise KeyError(f'the model has no output {self.logits_key!r}; it has {sorted(k for k in outputs if k.endswith("_logits"))}')
    return scores_from_logits(outputs[self.logits_key])

  def _record(self):
    from . import ops
    dev = self.sets.device
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    # a capture stream of the scorer's own with arrival counters reserved on it before the capture; the scorer holds them
    # for as long as the graph lives (ops.reserve_sync_words)
    stream = torch.cuda.Stream(dev)
    self.sync_words = ops.reserve_sync_words(dev, stream, 4096)
    try:
      with prefetch.capture_gate, torch.cuda.graph(graph, stream=stream):     # (no loader thread allocates or waits inside the capture)
        self.out = self._forward(self.image_entry, self.text_entry)
    finally:
      ops.release_sync_words(dev, stream)
    self.graph = graph

  def _batch(self) -> torch.Tensor:
    """Scores of the pairs in the entry buffers.  With the graph: the graph's output buffer, read it before the next batch."""
    if self.graph is not None:
      self.graph.replay()
      return self.out
    if self.use_graph and self._eager_done:
      try:
        self._record()
        self.graph.replay()
        return self.out
      except Exception as e:       # something in this configuration cannot be captured: stay eager, say so once
        warnings.warn(f'pair scorer not recorded as a HIP graph ({type(e).__name__}: {e}); continuing with eager batches')
        self.close()
        self.use_graph = False
        torch.cuda.synchronize(self.sets.device)
    self._eager_done = True
    return self._forward(self.image_entry, self.text_entry)

  def score_all(self, shard=(0, 1)) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores float32 [I, T], scored bool [I, T]) on the device: the shard's pairs in batches of `batch_size`, the tail
    padded with entry -1 and dropped.  Pairs of other shards keep score -1 and `scored` False."""
    was_training = self.model.training
    self.model.eval()
    sets, bs = self.sets, self.batch_size
    I, T, dev = sets.num_images, sets.num_texts, sets.device
    total = num_shard_pairs(I, T, shard)
    n_batches = (total + bs - 1) // bs
    ie_all, te_all = pair_entries(I, T, 0, n_batches * bs, shard, device=dev)
    # one spare slot past the matrix takes the rows of padded entries
    flat = torch.where(ie_all >= 0, ie_all.long() * T + te_all.long(), torch.full_like(ie_all, I * T, dtype=torch.int64))
    scores = torch.full((I * T + 1,), -1.0, dtype=torch.float32, device=dev)
    scored = torch.zeros(I * T + 1, dtype=torch.bool, device=dev)
    try:
      self._refresh_projection()
      for k in range(n_batches):
        sl = slice(k * bs, (k + 1) * bs)
        self.image_entry.copy_(ie_all[sl])
        self.text_entry.copy_(te_all[sl])
        scores[flat[sl]] = self._batch()
        scored[flat[sl]] = True
    finally:
      self.model.train(was_training)
    scores[I * T], scored[I * T] = -1.0, False
    return scores[:I * T].view(I, T), scored[:I * T].view(I, T)

  @torch.no_grad()
  def score_pairs(self, image_entry, text_entry) -> torch.Tensor:
    """Scores of an explicit list of pairs (re-ranking a shortlist), float32 [n]; eager.  The list runs in batches of
    `batch_size`, the last one padded with entry -1 like the tail of `score_all`: every kernel sees the shapes it sees
    there, so a pair's score has the bits of its matrix entry."""
    dev = self.sets.device
    ie = torch.as_tensor(image_entry, device=dev).to(torch.int32).reshape(-1)
    te = torch.as_tensor(text_entry, device=dev).to(torch.int32).reshape(-1)
    if ie.shape != te.shape:
      raise ValueError('image_entry and text_entry must have the same length')
    n, bs = ie.shape[0], self.batch_size
    pad = (-n) % bs
    if pad:
      minus1 = torch.full((pad,), -1, dtype=torch.int32, device=dev)
      ie, te = torch.cat([ie, minus1]), torch.cat([te, minus1])
    was_training = self.model.training
    self.model.eval()
    try:
      self._refresh_projection()
      parts = [self._forward(ie[i:i + bs].contiguous(), te[i:i + bs].contiguous()) for i in range(0, n, bs)]
    finally:
      self.model.train(was_training)
    return torch.cat(parts)[:n] if parts else torch.empty(0, dtype=torch.float32, device=dev)

  def close(self):
    self.graph = None            # (first: its launches name the counters)
    self.sync_words = None
    self.out = None


# ---- recall@k and the result files from the score matrix -------------------------------------------------------------
def _host(x, dtype=None):
  a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
  return a if dtype is None else a.astype(dtype)


def results_from_scores(scores, scored, image_index, text_index, gt_image_index):
  """The `predict.RawResult` list of the scored pairs, image-major: what `predict.predict` returns for them."""
  s, m = _host(scores, np.float64), _host(scored, bool)
  img, txt, gt = _host(image_index).tolist(), _host(text_index).tolist(), _host(gt_image_index).tolist()
  return [predict.RawResult(img[i], txt[t], gt[t], float(s[i, t])) for i, t in zip(*np.nonzero(m))]


def _matrices(scores, scored, image_index, text_index, gt_image_index):
  """Score and ground-truth matrices as `predict.get_recall_at_k` pivots them: rows / columns that hold a scored pair,
  sorted by id; unscored pairs -1 / not ground truth."""
  s, m = _host(scores, np.float64), _host(scored, bool)
  img, txt, gt = _host(image_index), _host(text_index), _host(gt_image_index)
  rows, cols = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
  rows, cols = rows[np.argsort(img[rows], kind='stable')], cols[np.argsort(txt[cols], kind='stable')]
  m = m[np.ix_(rows, cols)]
  score = np.where(m, s[np.ix_(rows, cols)], -1.0)
  gt_matrix = np.where(m, (img[rows][:, None] == gt[cols][None, :]).astype(np.float64), 0.0)
  return score, gt_matrix


def recall_at_k_from_scores(scores, scored, image_index, text_index, gt_image_index, topks=(1, 3, 5, 10)):
  """`predict.get_recall_at_k(results_from_scores(...))`, string for string, straight from the [I, T] matrix: index
  arrays in any order, tied scores ranked as the stable double argsort ranks them, unscored pairs -1 / not ground truth."""
  score, gt_matrix = _matrices(scores, scored, image_index, text_index, gt_image_index)
  recall = collections.OrderedDict()
  if score.size == 0:
    for name in ('i2t', 't2i'):
      for k in topks:
        recall[f'{name} @ {k:>2}'] = f'{0.0:.4f}'
    return recall
  # the rank expression of predict.get_recall_at_k, restated (predict.py is the reference-shaped route and stays as it
  # is); tests/test_retrieval_pairs_host.py holds the two to the same strings, so a change to one that is not made to
  # the other fails there
  rank = lambda x, axis: np.argsort(np.argsort(x, axis=axis, kind='stable'), axis=axis, kind='stable')
  m, n = score.shape
  i2t_rank = (rank(score, 1) - n) * -1
  t2i_rank = (rank(score, 0) - m) * -1
  for name, rk, axis in (('i2t', i2t_rank, 1), ('t2i', t2i_rank, 0)):
    for k in topks:
      at_gt = rk * gt_matrix
      match = np.clip(((at_gt <= k) & (at_gt > 0)).sum(axis=axis).astype(float), 0, 1)
      valid = np.clip(gt_matrix.sum(axis=axis), 0, 1)
      r = match.sum() / valid.sum() if valid.sum() > 0 else 0.0
      recall[f'{name} @ {k:>2}'] = f'{r:.4f}'
  return recall


def write_results_from_scores(scores, scored, image_index, text_index, gt_image_index, output_dir: str,
                              topks: Sequence[int] = (1, 3, 5, 10)):
  """`predict.write_results(results_from_scores(...), output_dir, topks)`: the same results.csv (scores clipped to
  [0, 1], %.8f, image-major) and recall.json, byte for byte."""
  os.makedirs(output_dir, exist_ok=True)
  s, m = np.clip(_host(scores, np.float64), 0.0, 1.0), _host(scored, bool)
  img, txt, gt = _host(image_index).tolist(), _host(text_index).tolist(), _host(gt_image_index).tolist()
  with open(os.path.join(output_dir, 'results.csv'), 'w', newline='') as f:
    w = csv.writer(f)
    w.writerow(predict.RawResult._fields)
    w.writerows([img[i], txt[t], gt[t], f'{float(s[i, t]):.8f}'] for i, t in zip(*np.nonzero(m)))
  recall = recall_at_k_from_scores(s, m, image_index, text_index, gt_image_index, topks)
  with open(os.path.join(output_dir, 'recall.json'), 'w') as f:
    json.dump(recall, f, indent=4)
  return recall


# ---- from records to recall@k -------------------------------------------------------------------------------------------
def evaluate_from_records(task, model, data_cfg, batch_size: int, output_dir: Optional[str] = None,
                          topks: Sequence[int] = (1, 3, 5, 10), shard=(0, 1), prefetch: int = 0, **loader_args):
  """Retrieval evaluation on TFRecord files: `retrieval_dataloader.MmtRetrievalDataLoader(data_cfg, **loader_args)`
  fills the sets, a `PairScorer` scores this shard's pairs -- all of them (`score_all`) for separate sets, the listed
  ones (`score_pairs`, scattered into the [I, T] matrix and its `scored` mask) for pairs in records -- and
  `recall_at_k_from_scores` turns the matrix into the recall dictionary, which is returned.  With `output_dir` the
  reference's two result files are written too (`write_results_from_scores`).  shard (id, n) scores the pairs with
  p % n == id only; merging the shards of several ranks into one result is not built.  prefetch > 0: the set build -- all
  the reading and decoding of this evaluation -- runs on a `prefetch.Prefetcher`'s worker thread and side stream, under
  the capture gate, and reaches this thread's stream through its event (a negative value is a ValueError)."""
  from . import prefetch as prefetch_lib
  from .retrieval_dataloader import MmtRetrievalDataLoader
  loader = MmtRetrievalDataLoader(data_cfg, **loader_args)
  if prefetch_lib.check_buffer_size(prefetch) > 0:
    with prefetch_lib.Prefetcher(((loader.sets(), loader.pairs()) for _ in range(1)), device=loader.device, depth=1) as ahead:
      sets, listed = next(ahead)
  else:
    sets, listed = loader.sets(), loader.pairs()
  scorer = PairScorer(task, model, sets, batch_size)
  try:
    if listed is None:
      scores, scored = scorer.score_all(shard)
    else:
      num_shard_pairs(0, 0, shard)                               # the shard check
      ie = torch.from_numpy(listed[0][int(shard[0])::int(shard[1])].copy()).to(sets.device)
      te = torch.from_numpy(listed[1][int(shard[0])::int(shard[1])].copy()).to(sets.device)
      scores = torch.full((sets.num_images, sets.num_texts), -1.0, dtype=torch.float32, device=sets.device)
      scored = torch.zeros(sets.num_images, sets.num_texts, dtype=torch.bool, device=sets.device)
      scores[ie.long(), te.long()] = scorer.score_pairs(ie, te)
      scored[ie.long(), te.long()] = True
  finally:
    scorer.close()
  idx = (sets.image_index, sets.text_index, sets.gt_image_index)
  if output_dir:
    return write_results_from_scores(scores, scored, *idx, output_dir, topks)
  return recall_at_k_from_scores(scores, scored, *idx, topks)
