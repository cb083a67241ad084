"""The fine-tuning and retrieval loaders on records, without a GPU: the index bookkeeping of the pair records, the
matching batch arithmetic, how `ClassificationTask.build_inputs` chooses its source, and the int64 field lookup's
errors.  The loaders run with device 'cpu' up to the point where they would decode."""
import json
import os

import numpy as np
import pytest

from tests import _finetune_record_cases as F
from tests import _record_cases as R


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


@pytest.fixture(scope='module')
def vocab_path(tmp_path_factory):
  return R.write_vocab(tmp_path_factory.mktemp('vocab') / 'vocab.txt')


# ---- index bookkeeping -----------------------------------------------------------------------------------------------
def test_first_appearance_on_unsorted_sparse_and_repeated_ids(lib):
  from mmt_amd.retrieval_dataloader import first_appearance
  ids = [40, 7, 40, 1000003, 7, 7, -2, 0, 40, 2 ** 40]
  unique, entry = first_appearance(ids)
  assert unique.dtype == np.int64 and entry.dtype == np.int32
  assert unique.tolist() == [40, 7, 1000003, -2, 0, 2 ** 40]
  assert entry.tolist() == [0, 1, 0, 2, 1, 1, 3, 4, 0, 5]
  assert unique[entry].tolist() == ids
  # plain Python of the same definition, on a longer list
  rng = np.random.default_rng(3)
  ids = rng.integers(-50, 50, size=500) * 1000003
  seen = {}
  want = [seen.setdefault(int(v), len(seen)) for v in ids]
  unique, entry = first_appearance(ids)
  assert entry.tolist() == want and unique.tolist() == list(seen)
  for single in ([5], [5, 5, 5]):
    unique, entry = first_appearance(single)
    assert unique.tolist() == [5] and entry.tolist() == [0] * len(single)
  unique, entry = first_appearance([])
  assert unique.shape == (0,) and entry.shape == (0,) and entry.dtype == np.int32


def test_matching_batch_size_as_the_loader_uses_it(lib):
  from mmt_amd import classification_dataloader as cd
  from mmt_amd import configs
  from mmt_amd import feature_pipeline as fp
  for per_replica, ratio, min_shift, want in ((8, 1, 5, 16), (8, 2, 5, 16), (8, 3, 5, 24), (4, 3, 5, 16), (64, 1, 5, 128),
                                              (1, 1, 5, 8), (7, 2, 5, 21), (8, 1, 0, 16)):
    cfg = configs.MmtClassificationDataConfig(negative_positive_ratio=ratio, min_shift=min_shift)
    Bm = cd.MmtClassificationDataLoader(cfg, device='cpu').group_size(per_replica)
    assert Bm == want == fp.matching_batch_size(cfg, per_replica), (per_replica, ratio, min_shift)
    assert Bm % per_replica == 0                               # the matched examples fall into whole per-replica batches
    assert Bm > ratio + 1 + min_shift or per_replica == 1      # what make_matching_features asks of its batch
    assert Bm > ratio + min_shift                              # the largest shift is shorter than the batch


# ---- build_inputs ------------------------------------------------------------------------------------------------------
def classification_task(**data):
  import mmt_amd
  from mmt_amd import configs
  exp = configs.get_exp_config('mmt/classification')
  exp.override({'task': {'model': {'num_classes': 2, 'cls_heads': [{'inner_dim': 16, 'num_classes': 2, 'name': 'itm'}]},
                         'train_data': dict(dict(image_size=F.IMAGE, patch_size=F.PATCH, max_seq_len=F.SEQ, global_batch_size=F.BATCH,
                                                 text_special_token_field_dict=json.dumps(R.FIELD_DICT)), **data)}})
  return mmt_amd.tasks.get_task(exp.task), exp.task.train_data


ITM_FIELDS = dict(label_field='itm_label_ids', label_weights_field='itm_label_weights', pos_weights_field='itm_pos_weights')


def test_build_inputs_of_the_classification_task_chooses_the_source(lib, tmp_path, vocab_path):
  for path in ('', 'gs://your_input_data_patterns'):
    task, d = classification_task(input_path=path, vocab_filename=vocab_path, **ITM_FIELDS)
    task.build_inputs(d, device='cpu')                         # the iterator is lazy: nothing is drawn
    assert task.input_source == 'synthetic'
  for vocab in (vocab_path, ''):                               # a local pattern must match, vocabulary or not
    task, d = classification_task(input_path=str(tmp_path / 'nothing-*.tfrecord'), vocab_filename=vocab, **ITM_FIELDS)
    with pytest.raises(ValueError, match='matches no file'):
      task.build_inputs(d, device='cpu')
  R.write_shards(tmp_path, R.loader_records(4), 1)
  pattern = str(tmp_path / '*.tfrecord')
  task, d = classification_task(input_path=pattern, vocab_filename=vocab_path)       # label_field unset: 'label_ids'
  with pytest.raises(ValueError, match=r"label_field is 'label_ids'.*itm_label_ids.*itm_label_weights.*itm_pos_weights"):
    task.build_inputs(d, device='cpu')
  for what in ('label_weights_field', 'pos_weights_field'):
    fields = dict(ITM_FIELDS)
    fields[what] = 'weights'
    task, d = classification_task(input_path=pattern, vocab_filename=vocab_path, **fields)
    with pytest.raises(ValueError, match=f"{what} is 'weights'"):
      task.build_inputs(d, device='cpu')
  task, d = classification_task(input_path=pattern, vocab_filename=vocab_path, **ITM_FIELDS)
  task.build_inputs(d, device='cpu')                           # lazy again: the loader is built, no record is read
  assert task.input_source == 'records'


def test_label_keys_are_the_references_names(lib):
  from mmt_amd import classification_dataloader as cd
  assert cd.LABEL_KEYS == ('itm_label_ids', 'itm_label_weights', 'itm_pos_weights')


# ---- int64 fields ------------------------------------------------------------------------------------------------------
def retrieval_config(vocab_path, **kw):
  from mmt_amd import configs
  base = dict(vocab_filename=vocab_path, is_training=False, global_batch_size=F.BATCH, image_size=F.IMAGE, patch_size=F.PATCH,
              max_seq_len=F.SEQ, text_special_token_field_dict=json.dumps(R.FIELD_DICT))
  base.update(kw)
  return configs.MmtRetrievalDataConfig(**base)


def test_int64_field_errors_name_file_record_and_feature(lib, tmp_path, vocab_path):
  from mmt_amd import retrieval_dataloader as rd
  im, texts = F.retrieval_images()[0], F.retrieval_texts()
  good = F.pair_payload(im, 4, texts[0])
  cases = {
      'missing': (R.example([('image_index', 'int64', [4]), ('gt_image_index', 'int64', [4]), ('image_data', 'bytes', [b'x'])]),
                  r"feature 'text_index' is missing"),
      'two': (R.example([('image_index', 'int64', [4]), ('text_index', 'int64', [1, 2]), ('gt_image_index', 'int64', [4])]),
              r"feature 'text_index' must hold exactly one int64 value"),
      'bytes': (R.example([('image_index', 'int64', [4]), ('text_index', 'int64', [1]), ('gt_image_index', 'bytes', [b'4'])]),
                r"feature 'gt_image_index' must hold exactly one int64 value"),
      'none': (R.example([('image_index', 'int64', []), ('text_index', 'int64', [1]), ('gt_image_index', 'int64', [4])]),
               r"feature 'image_index' must hold exactly one int64 value"),
      'noimage': (R.example([('text_index', 'int64', [1]), ('gt_image_index', 'int64', [4])]), r"feature 'image_index' is missing"),
      'alias': (R.example([('index', 'bytes', [b'1']), ('text_index', 'int64', [1]), ('gt_image_index', 'int64', [4])]),
                r"feature 'index' must hold exactly one int64 value"),
  }
  for name, (payload, text) in cases.items():
    d = tmp_path / name
    d.mkdir()
    F.write_file(d / 'pairs.tfrecord', [good, good, payload])
    loader = rd.MmtRetrievalDataLoader(retrieval_config(vocab_path, input_path=str(d / '*.tfrecord')), device='cpu')
    with pytest.raises(ValueError, match=r'pairs\.tfrecord: record 2: ' + text):
      loader.sets()


def test_group_lookup_reads_int64_values_on_the_host(lib, tmp_path, vocab_path):
  """The shared group stage with device 'cpu': pack, checksum (host mirror) and lookup; and a flipped bit is named."""
  from mmt_amd import record_stages, records
  texts = F.retrieval_texts()
  path = F.write_file(tmp_path / 't.tfrecord', [F.text_payload(r) for r in texts])
  stages = record_stages.RecordStages(retrieval_config(vocab_path), device='cpu')
  group = [(p, c, path, i) for i, (p, c) in enumerate(records.read_shard(path))]
  blob, blob_d, fields = stages._open_group(group, ['text_index', 'gt_image_index', 'caption', 'nothing'])
  assert blob_d.device.type == 'cpu'
  got = [(record_stages.one_int64_field(group, i, f[0], 'text_index'), record_stages.one_int64_field(group, i, f[1], 'gt_image_index'))
         for i, f in enumerate(fields)]
  assert got == [(r['text_index'], r['gt_image_index']) for r in texts]
  view = blob.numpy()
  for i, f in enumerate(fields):
    off, length = record_stages.one_bytes_field(group, i, f[2], 'caption')
    assert view[off:off + length].tobytes() == texts[i]['caption'].encode('utf-8')
    assert record_stages.text_field(group, i, f[3], 'nothing') == (0, 0)
    with pytest.raises(ValueError, match=rf"t\.tfrecord: record {i}: feature 'nothing' is missing"):
      record_stages.one_int64_field(group, i, f[3], 'nothing')
    with pytest.raises(ValueError, match=rf"t\.tfrecord: record {i}: feature 'text_index' must hold exactly one bytes value"):
      record_stages.one_bytes_field(group, i, f[0], 'text_index')
  bad = list(group)
  flipped = bytearray(bad[3][0])
  flipped[-1] ^= 1                                             # the last byte of the text_index varint: still an Example
  bad[3] = (bytes(flipped), *bad[3][1:])
  with pytest.raises(ValueError, match=r't\.tfrecord: record 3: the payload checksum does not match'):
    stages._open_group(bad, ['text_index'])


def test_retrieval_counts_are_checked_before_anything_is_decoded(lib, tmp_path, vocab_path):
  from mmt_amd import retrieval_dataloader as rd
  path, _ = F.write_pair_records(tmp_path)
  for kw, text in ((dict(num_image_examples=4), 'num_image_examples is 4, but 5 were read'),
                   (dict(num_text_examples=21), 'num_text_examples is 21, but 7 were read')):
    with pytest.raises(ValueError, match=text):
      rd.MmtRetrievalDataLoader(retrieval_config(vocab_path, input_path=path, **kw), device='cpu').sets()
  with pytest.raises(ValueError, match='matches no file'):
    rd.MmtRetrievalDataLoader(retrieval_config(vocab_path, image_input_path=path, text_input_path=str(tmp_path / 'no-*')),
                              device='cpu').sets()
  assert os.path.exists(path)
