"""The retrieval loader (mmt_amd/retrieval_dataloader.py) and `retrieval.evaluate_from_records` on files written at test
time from the committed JPEG and PNG fixtures and the text corpus: 5 images (one a PNG) and 7 texts with unsorted,
non-contiguous ids, as separate sets and as 21 pair records.  The tables are compared bit for bit at image 32, patch 16,
max_seq_len 32; the model tests use the tiny experiment's shapes, as tests/test_gpu_retrieval_pairs.py does."""
import functools
import json
import os

import pytest
import torch

from tests import _finetune_record_cases as F
from tests import _record_cases as R

pytestmark = pytest.mark.gpu

IMAGE, PATCH, SEQ, BATCH, N_PATCH, N_IMG = F.IMAGE, F.PATCH, F.SEQ, F.BATCH, F.N_PATCH, F.N_IMG


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
def separate(tmp_path_factory):
  return F.write_separate_sets(tmp_path_factory.mktemp('separate'))


@pytest.fixture(scope='module')
def paired(tmp_path_factory):
  return F.write_pair_records(tmp_path_factory.mktemp('paired'))


def data_config(vocab_path, **kw):
  from mmt_amd import configs
  base = dict(vocab_filename=vocab_path, is_training=False, global_batch_size=BATCH, image_size=IMAGE, patch_size=PATCH,
              max_seq_len=SEQ, text_special_token_field_dict=json.dumps(R.FIELD_DICT), drop_remainder=False)
  base.update(kw)
  return configs.MmtRetrievalDataConfig(**base)


@pytest.fixture(scope='module')
def separate_loader(lib, separate, vocab_path):
  from mmt_amd import retrieval_dataloader as rd
  loader = rd.MmtRetrievalDataLoader(data_config(vocab_path, image_input_path=separate[0], text_input_path=separate[1]), device='cuda', chunk=2)
  loader.sets()
  return loader


@pytest.fixture(scope='module')
def paired_loader(lib, paired, vocab_path):
  from mmt_amd import retrieval_dataloader as rd
  loader = rd.MmtRetrievalDataLoader(data_config(vocab_path, input_path=paired[0]), device='cuda', chunk=2)
  loader.sets()
  return loader


@functools.lru_cache(maxsize=None)
def expected_image(name, image=IMAGE):
  from mmt_amd import feature_pipeline as fp
  out = fp.images_to_patch_features([torch.from_numpy(F.image_pixels(name).copy()).cuda()], image, PATCH)
  return out['patch_embeddings'][0].cpu()


@functools.lru_cache(maxsize=None)
def cpu_vocab(path):
  from mmt_amd import text_frontend
  return text_frontend.WordpieceVocab(path)


def expected_text(vocab_path, rec):
  from mmt_amd import text_frontend
  out = text_frontend.texts_to_token_features(cpu_vocab(vocab_path), [[rec['caption']], [rec['alt_text']]], list(R.FIELD_DICT.values()),
                                              SEQ, N_PATCH)
  return out['text_token_ids'][0], int(out['num_text_wordpieces'][0])


def assert_tables(sets, images, texts, vocab_path):
  """images: (fixture, id) per table row; texts: the text records per table row."""
  assert sets.num_images == len(images) and sets.num_texts == len(texts)
  assert sets.image_index.tolist() == [i for _, i in images]
  assert sets.text_index.tolist() == [r['text_index'] for r in texts]
  assert sets.gt_image_index.tolist() == [r['gt_image_index'] for r in texts]
  assert sets.patch_embeddings.dtype == torch.float32
  for row, (name, _) in enumerate(images):
    assert torch.equal(sets.patch_embeddings[row].cpu(), expected_image(name)), name
  for row, rec in enumerate(texts):
    want, count = expected_text(vocab_path, rec)
    assert torch.equal(sets.text_token_ids[row].cpu(), want), row
    assert int(sets.num_text_wordpieces[row]) == count, row
  v = cpu_vocab(vocab_path)
  assert sets.prefix_ids.tolist() == [v.id('[CLS]'), v.id('[PATCH]')] + [104 + i for i in range(N_PATCH)]


def test_separate_sets_fill_the_tables_in_read_order(separate, separate_loader, vocab_path):
  _, _, images, texts = separate
  assert any(name.startswith('png:') for name, _ in images)
  assert [i for _, i in images] != sorted(i for _, i in images)
  assert_tables(separate_loader.sets(), images, texts, vocab_path)
  assert separate_loader.pairs() is None
  assert (separate_loader.images_decoded, separate_loader.texts_decoded) == (5, 7)
  assert separate_loader.sets() is separate_loader.sets()                    # built once


def test_pair_records_decode_every_index_once(paired, paired_loader, vocab_path):
  _, listed = paired
  assert len(listed) == 21 and len(set(listed)) == 21
  ims, texts = F.retrieval_images(), F.retrieval_texts()
  image_order = list(dict.fromkeys(i for i, _ in listed))                    # first appearance
  text_order = list(dict.fromkeys(t for _, t in listed))
  assert sorted(image_order) == list(range(5)) and image_order != sorted(image_order) and text_order == list(range(7))
  sets = paired_loader.sets()
  assert_tables(sets, [(ims[i], F.IMAGE_IDS[i]) for i in image_order], [texts[t] for t in text_order], vocab_path)
  assert (paired_loader.images_decoded, paired_loader.texts_decoded) == (5, 7)
  ie, te = paired_loader.pairs()
  assert ie.dtype == te.dtype == 'int32' and ie.shape == te.shape == (21,)
  assert sets.image_index.cpu()[ie.astype('int64')].tolist() == [F.IMAGE_IDS[i] for i, _ in listed]
  assert sets.text_index.cpu()[te.astype('int64')].tolist() == [F.TEXT_IDS[t] for _, t in listed]


def _same_batch(got, want):
  for part in (0, 1):
    assert list(got[part]) == list(want[part])
    for k, v in want[part].items():
      assert torch.equal(got[part][k], v) if torch.is_tensor(v) else got[part][k] == v, k


def test_load_gives_materialised_windows_of_the_sharded_pair_list(separate, paired, separate_loader, paired_loader, vocab_path):
  from mmt_amd import retrieval_dataloader as rd
  from mmt_amd.retrieval import pair_entries
  _, _, images, texts = separate
  sets = separate_loader.sets()
  batches = list(separate_loader.load(rank=1, num_replicas=2, batch_size=BATCH))          # 35 pairs, the odd ones: 17
  assert [b[0]['word_ids'].shape[0] for b in batches] == [8, 8, 1]
  ps = list(range(1, 35, 2))
  assert torch.cat([b[0]['image_index'] for b in batches]).tolist() == [images[p // 7][1] for p in ps]
  assert torch.cat([b[0]['text_index'] for b in batches]).tolist() == [texts[p % 7]['text_index'] for p in ps]
  assert torch.cat([b[1]['label_ids'] for b in batches]).tolist() == [int(images[p // 7][1] == texts[p % 7]['gt_image_index']) for p in ps]
  for k, first in enumerate((0, 8, 16)):
    _same_batch(batches[k], sets.materialize(*pair_entries(5, 7, first, min(8, 17 - first), (1, 2), device='cuda')))
  keep = separate_loader.params.drop_remainder
  separate_loader.params.drop_remainder = True
  try:
    dropped = list(separate_loader.load(rank=1, num_replicas=2, batch_size=BATCH))
  finally:
    separate_loader.params.drop_remainder = keep
  assert [b[0]['word_ids'].shape[0] for b in dropped] == [8, 8]
  # listed pairs: the even places of the list, 11 of 21
  _, listed = paired
  sets, (ie, te) = paired_loader.sets(), paired_loader.pairs()
  batches = list(paired_loader.load(rank=0, num_replicas=2, batch_size=BATCH))
  assert [b[0]['word_ids'].shape[0] for b in batches] == [8, 3]
  assert torch.cat([b[0]['image_index'] for b in batches]).tolist() == [F.IMAGE_IDS[i] for i, _ in listed[0::2]]
  assert torch.cat([b[0]['text_index'] for b in batches]).tolist() == [F.TEXT_IDS[t] for _, t in listed[0::2]]
  _same_batch(batches[0], sets.materialize(ie[0::2][:8].copy(), te[0::2][:8].copy()))
  _same_batch(batches[1], sets.materialize(ie[0::2][8:].copy(), te[0::2][8:].copy()))
  # counts and duplicates
  with pytest.raises(ValueError, match='num_image_examples is 6, but 5 were read'):
    rd.MmtRetrievalDataLoader(data_config(vocab_path, image_input_path=separate[0], text_input_path=separate[1], num_image_examples=6),
                              device='cuda').sets()


def test_a_duplicate_image_index_in_a_separate_set_is_refused(lib, tmp_path, separate, vocab_path):
  from mmt_amd import retrieval_dataloader as rd
  ims = F.retrieval_images()
  F.write_file(tmp_path / 'image.tfrecord', [F.image_payload(ims[0], 40), F.image_payload(ims[1], 7), F.image_payload(ims[3], 40)])
  cfg = data_config(vocab_path, image_input_path=str(tmp_path / 'image.tfrecord'), text_input_path=separate[1])
  with pytest.raises(ValueError, match='image_index holds duplicate ids'):
    rd.MmtRetrievalDataLoader(cfg, device='cuda').sets()


# ---- from records to recall@k ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model_setup(lib, vocab_path):
  """The tiny classification model at the tiny experiment's shapes (max_seq_len 256, image 224), and its data config."""
  import mmt_amd
  from mmt_amd import configs
  from tests._parity import tiny_experiment
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp = configs.get_exp_config('mmt/retrieval')
  keep = {k: v for k, v in exp.task.train_data.as_dict().items() if hasattr(cexp.task.train_data, k)}
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(),
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': dict(keep, vocab_filename=vocab_path, is_training=False, drop_remainder=False,
                                             text_special_token_field_dict=json.dumps(R.FIELD_DICT))}})
  task = mmt_amd.tasks.get_task(cexp.task)
  torch.manual_seed(0)
  model = task.build_model().cuda().eval()
  return task, model, cexp.task.train_data


def _predict_recall(task, model, sets, ie, te):
  """The route that existed before: `predict.predict` over materialised batches of the same pairs, 8 at a time."""
  from mmt_amd import predict
  ie, te = torch.as_tensor(ie, device='cuda'), torch.as_tensor(te, device='cuda')
  batches = [sets.materialize(ie[k:k + BATCH], te[k:k + BATCH]) for k in range(0, ie.shape[0], BATCH)]
  results = predict.predict(task, batches, model)
  assert len(results) == ie.shape[0]
  return predict.get_recall_at_k(results), results


@pytest.mark.parametrize('mode', ['separate', 'paired'])
def test_evaluate_from_records_gives_the_recall_of_the_predict_route(model_setup, separate, paired, tmp_path, mode):
  import dataclasses
  from mmt_amd import retrieval
  from mmt_amd import retrieval_dataloader as rd
  from mmt_amd.retrieval import pair_entries
  task, model, base = model_setup
  paths = dict(image_input_path=separate[0], text_input_path=separate[1]) if mode == 'separate' else dict(input_path=paired[0])
  cfg = dataclasses.replace(base, **paths)
  out = str(tmp_path / 'out')
  recall = retrieval.evaluate_from_records(task, model, cfg, BATCH, output_dir=out, device='cuda', chunk=2)
  loader = rd.MmtRetrievalDataLoader(cfg, device='cuda', chunk=4)
  sets = loader.sets()
  ie, te = pair_entries(5, 7, 0, 35, device='cuda') if mode == 'separate' else loader.pairs()
  want, results = _predict_recall(task, model, sets, ie, te)
  print(mode, 'recall from records:', dict(recall))
  print(mode, 'scores of the predict route: min %.6f max %.6f' % (min(r.output for r in results), max(r.output for r in results)))
  assert max(r.output for r in results) - min(r.output for r in results) > 1e-4        # the model tells the pairs apart
  assert list(recall) == [f'{d} @ {k:>2}' for d in ('i2t', 't2i') for k in (1, 3, 5, 10)]
  assert dict(recall) == dict(want)
  if mode == 'paired':                                         # no output_dir: the same dictionary, no file
    assert retrieval.evaluate_from_records(task, model, cfg, BATCH, device='cuda', chunk=2) == recall
  assert sorted(os.listdir(out)) == ['recall.json', 'results.csv']
  with open(os.path.join(out, 'recall.json')) as f:
    assert json.load(f) == dict(recall)
  with open(os.path.join(out, 'results.csv')) as f:
    assert len(f.read().splitlines()) == 1 + len(results)
