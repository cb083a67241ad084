"""The fine-tuning loader (mmt_amd/classification_dataloader.py) on shards written at test time from the committed JPEG
fixtures and the text corpus, at the smallest shapes of tests/test_gpu_records.py: image 32, patch 16, max_seq_len 32,
per-replica batch 8, so the matching step works on 16 examples.  Every comparison is bit for bit."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import _finetune_record_cases as F
from tests import _jpeg_cases as JC
from tests import _record_cases as R

pytestmark = pytest.mark.gpu

IMAGE, PATCH, SEQ, BATCH, N_PATCH, N_IMG = F.IMAGE, F.PATCH, F.SEQ, F.BATCH, F.N_PATCH, F.N_IMG
MIN_SHIFT, GROUP = 5, 16


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


@pytest.fixture(scope='module')
def vocab_path(tmp_path_factory):
  return R.write_vocab(tmp_path_factory.mktemp('vocab') / 'vocab.txt')


@pytest.fixture(scope='module')
def shards(tmp_path_factory):
  """32 records over 2 shards (validation order = record order), and the records."""
  recs = R.loader_records(32)
  d = tmp_path_factory.mktemp('plain')
  return R.write_shards(d, recs, 2), recs, str(d / '*.tfrecord')


def data_config(pattern, vocab_path, **kw):
  from mmt_amd import configs
  base = dict(input_path=pattern, vocab_filename=vocab_path, is_training=False, global_batch_size=BATCH, image_size=IMAGE,
              patch_size=PATCH, max_seq_len=SEQ, text_special_token_field_dict=json.dumps(R.FIELD_DICT), min_shift=MIN_SHIFT,
              seed=11)
  base.update(kw)
  return configs.MmtClassificationDataConfig(**base)


@functools.lru_cache(maxsize=None)
def expected_image(name):
  """images_to_patch_features of the committed Pillow decode, computed once per fixture: float32 [P^2, 3 * patch^2] on the CPU."""
  from mmt_amd import feature_pipeline as fp
  out = fp.images_to_patch_features([torch.from_numpy(JC.expected(name).copy()).cuda()], IMAGE, PATCH)
  return out['patch_embeddings'][0].cpu()


@functools.lru_cache(maxsize=None)
def cpu_vocab(path):
  from mmt_amd import text_frontend
  return text_frontend.WordpieceVocab(path)


@functools.lru_cache(maxsize=None)
def expected_text(vocab_path, caption, alt_text):
  from mmt_amd import text_frontend
  out = text_frontend.texts_to_token_features(cpu_vocab(vocab_path), [[caption], [alt_text]], list(R.FIELD_DICT.values()), SEQ, N_PATCH)
  return out['text_token_ids'][0], int(out['num_text_wordpieces'][0])


def images_of(inputs, b, group):
  got = inputs['patch_embeddings'][b].cpu()
  return [i for i, r in enumerate(group) if torch.equal(got, expected_image(r['image']))]


def texts_of(inputs, b, group, vocab_path):
  got, n = inputs['word_ids'][b, N_IMG:].cpu(), int(inputs['valid_len'][b]) - N_IMG
  hits = []
  for i, r in enumerate(group):
    want, count = expected_text(vocab_path, r['caption'], r['alt_text'])
    if count == n and torch.equal(got, want):
      hits.append(i)
  return hits


def matching_order(group, copies):
  """The matching step in plain Python: (image record, text record) of every example a group of records becomes.  Stable
  sort by the rank of the key's first appearance, image side tiled, text side of copy i rolled by min_shift + i."""
  first = {}
  for r in group:
    first.setdefault(r['key'], len(first))
  order = sorted(range(len(group)), key=lambda j: first[group[j]['key']])
  n = len(group)
  out = []
  for c in range(copies):
    shift = 0 if c == 0 else MIN_SHIFT + c
    out += [(order[j], order[(j - shift) % n]) for j in range(n)]
  return out


@pytest.mark.parametrize('ratio', [1, 2])
def test_validation_pass_matches_the_plain_python_matching(lib, shards, vocab_path, ratio):
  from mmt_amd import classification_dataloader as cd
  from mmt_amd import feature_pipeline as fp
  _, recs, pattern = shards
  copies = ratio + 1
  cfg = data_config(pattern, vocab_path, negative_positive_ratio=ratio)
  assert fp.matching_batch_size(cfg, BATCH) == GROUP
  groups = [recs[g:g + GROUP] for g in range(0, len(recs), GROUP)]
  want = [matching_order(group, copies) for group in groups]
  # not vacuous: 12 distinct images in a group of 16, and no roll brings a text to another record of its own image
  for group, pairs in zip(groups, want):
    assert len({r['image'] for r in group}) == 12 and len({r['caption'] for r in group}) == GROUP
    assert all(group[i]['key'] == group[t]['key'] for i, t in pairs[:GROUP])
    assert all(group[i]['key'] != group[t]['key'] for i, t in pairs[GROUP:])
  batches = list(cd.MmtClassificationDataLoader(cfg, device='cuda').load())
  assert [b[0]['word_ids'].shape[0] for b in batches] == [BATCH] * (len(groups) * GROUP * copies // BATCH)
  at = 0
  for inputs, labels in batches:
    assert torch.equal(labels['itm_label_weights'], torch.ones(BATCH, device='cuda'))
    assert torch.equal(labels['itm_pos_weights'], 1.0 + labels['itm_label_ids'].float() * (ratio - 1))
    for b in range(BATCH):
      g, e = divmod(at, GROUP * copies)
      at += 1
      group = groups[g]
      i, t = want[g][e]
      imgs, txts = images_of(inputs, b, group), texts_of(inputs, b, group, vocab_path)
      assert i in imgs and imgs == [k for k, r in enumerate(group) if torch.equal(expected_image(r['image']), expected_image(group[i]['image']))]
      assert all(group[k]['key'] == group[i]['key'] for k in imgs), (g, e, imgs)       # two fixtures never decode to the same patches
      assert txts == [t], (g, e, txts)
      assert int(labels['itm_label_ids'][b]) == int(e < GROUP), (g, e)
      assert int(labels['itm_label_ids'][b]) == int(group[i]['key'] == group[t]['key'])
  assert at == len(groups) * GROUP * copies


def test_records_short_of_a_matching_group_are_dropped(lib, tmp_path, vocab_path):
  from mmt_amd import classification_dataloader as cd
  R.write_shards(tmp_path, R.loader_records(21), 2)
  cfg = data_config(str(tmp_path / 'shard-*.tfrecord'), vocab_path)
  batches = list(cd.MmtClassificationDataLoader(cfg, device='cuda').load())
  assert [b[0]['word_ids'].shape[0] for b in batches] == [BATCH] * 4          # one group of 16 -> 32 examples; 5 records dropped
  R.write_shards(tmp_path, R.loader_records(15), 2, prefix='few')
  few = data_config(str(tmp_path / 'few-*.tfrecord'), vocab_path)
  assert list(cd.MmtClassificationDataLoader(few, device='cuda').load()) == []


@pytest.mark.parametrize('dense', [False, True], ids=['structured', 'dense'])
def test_keys_shapes_and_dtypes_are_those_of_the_synthetic_batch(lib, shards, vocab_path, dense):
  from mmt_amd import classification_dataloader as cd
  from mmt_amd import input_utils
  cfg = data_config(shards[2], vocab_path)
  got = next(cd.MmtClassificationDataLoader(cfg, device='cuda', dense_side_inputs=dense).load())
  want = input_utils.synthetic_batch(cfg, BATCH, 'cuda', vocab_size=len(cpu_vocab(vocab_path)), dense_side_inputs=dense,
                                     task='classification')
  sig = lambda d: {k: ((tuple(v.shape), v.dtype) if torch.is_tensor(v) else type(v)) for k, v in d.items()}
  assert sig(got[0]) == sig(want[0])
  assert sig(got[1]) == {'itm_label_ids': ((BATCH,), torch.int32), 'itm_label_weights': ((BATCH,), torch.float32),
                         'itm_pos_weights': ((BATCH,), torch.float32)}
  assert list(got[1]) == list(cd.LABEL_KEYS)


def test_training_same_seed_full_batches_repeats_mixes_labels_and_shards_files(lib, tmp_path, vocab_path):
  from mmt_amd import classification_dataloader as cd
  R.write_shards(tmp_path, R.loader_records(24), 4)
  cfg = data_config(str(tmp_path / '*.tfrecord'), vocab_path, is_training=True, cycle_length=2, use_rand_aug=True)

  def take(k, example_shuffle_buffer=32, **kw):
    it = cd.MmtClassificationDataLoader(cfg, device='cuda', shuffle_buffer=8, example_shuffle_buffer=example_shuffle_buffer).load(**kw)
    return [next(it) for _ in range(k)]
  a, b = take(12), take(12)             # 12 batches = 96 examples = 3 groups of 16 records = 48 records: two epochs of 24
  for (ia, la), (ib, lb) in zip(a, b):
    assert ia['word_ids'].shape[0] == BATCH and la['itm_label_ids'].shape[0] == BATCH
    for k in ia:
      assert torch.equal(ia[k], ib[k]) if torch.is_tensor(ia[k]) else ia[k] == ib[k], k
    for k in la:
      assert torch.equal(la[k], lb[k]), k
  # a buffer that holds a matched group (16 positives, then 16 negatives) mixes them; without it they come in runs
  mixed = [set(l['itm_label_ids'].tolist()) for _, l in a[:3]]
  print('labels of the first batches with the example shuffle:', [l['itm_label_ids'].tolist() for _, l in a[:3]])
  assert all(m == {0, 1} for m in mixed)
  runs = take(4, example_shuffle_buffer=1)
  assert [set(l['itm_label_ids'].tolist()) for _, l in runs] == [{1}, {1}, {0}, {0}]
  loader = cd.MmtClassificationDataLoader(cfg, device='cuda')
  for training in (False, True):
    cfg.is_training = training
    streams = [loader._file_stream(r, 2) for r in range(2)]
    first = [[next(s) for _ in range(2)] for s in streams]               # one epoch: 4 files over 2 pipelines
    assert not set(first[0]) & set(first[1]) and sorted(first[0] + first[1]) == loader.files()
  cfg.is_training = True
  r1 = take(1, rank=1, num_replicas=2, batch_size=BATCH)
  assert r1[0][0]['word_ids'].shape[0] == BATCH


def tiny_classification_experiment(**data):
  from mmt_amd import configs
  from tests._parity import tiny_experiment
  exp = tiny_experiment()
  cexp = configs.get_exp_config('mmt/classification')
  keep = {k: v for k, v in exp.task.train_data.as_dict().items() if hasattr(cexp.task.train_data, k)}
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(), 'num_classes': 2,
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': dict(keep, **data)}})
  return cexp


def test_classification_task_reads_records_and_trains_one_step(lib, shards, vocab_path):
  import mmt_amd
  from mmt_amd import optimization
  cexp = tiny_classification_experiment(
      input_path=shards[2], vocab_filename=vocab_path, text_special_token_field_dict=json.dumps(R.FIELD_DICT),
      label_field='itm_label_ids', label_weights_field='itm_label_weights', pos_weights_field='itm_pos_weights',
      negative_positive_ratio=2)
  d = cexp.task.train_data
  task = mmt_amd.tasks.get_task(cexp.task)
  torch.manual_seed(3)
  model = task.build_model().cuda()
  opt = optimization.create_optimizer(model, cexp.trainer.optimizer_config)
  it = task.build_inputs(d, device='cuda', batch_size=BATCH, loader_args=dict(shuffle_buffer=8, example_shuffle_buffer=48))
  assert task.input_source == 'records'
  inputs, labels = next(it)
  assert inputs['word_ids'].shape == (BATCH, d.max_seq_len) and set(labels) == {'itm_label_ids', 'itm_label_weights', 'itm_pos_weights'}
  out = task.train_step((inputs, labels), model, opt, clip_norm=1.0, step=1, micro_batch_size=BATCH)
  loss = float(out['loss'])
  print('loss of one fine-tuning step on a loader batch:', loss)
  assert np.isfinite(loss) and loss > 0
