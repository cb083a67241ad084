"""Record container on the GPU: mmt_records_crc bit for bit against the pure-Python oracle of tests/_record_cases.py, and
the pretraining loader (mmt_amd/pretrain_dataloader.py) on shards written at test time from the committed JPEG fixtures
and the text corpus, at the smallest shapes: image 32, patch 16, max_seq_len 32, batch 8."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import _jpeg_cases as JC
from tests import _record_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


# ---------------------------------------------------------------------------------------------------
# mmt_records_crc
# ---------------------------------------------------------------------------------------------------
def device_crc(lib, blob, offsets, lengths, stored=None, bytes_len=None):
  """One mmt_records_crc call: (crc uint32 [n], bad int32 [n]) as numpy; outputs and workspace start poisoned."""
  L = lib.lib()
  n = len(offsets)
  recs = (lib.Record * max(n, 1))()
  for i in range(n):
    recs[i].offset, recs[i].length = int(offsets[i]), int(lengths[i])
    recs[i].crc = 0 if stored is None else int(stored[i])
  blob_d = torch.from_numpy(blob).cuda()
  recs_d = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).cuda()
  crc = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
  bad = torch.full((max(n, 1),), -7, dtype=torch.int32, device='cuda')
  need = L.mmt_records_crc_workspace_bytes(n)
  work = torch.full((need,), 0xA5, dtype=torch.uint8, device='cuda')
  lib.check(L.mmt_records_crc(blob_d.data_ptr(), blob.size if bytes_len is None else bytes_len, n, recs_d.data_ptr(), crc.data_ptr(),
                              bad.data_ptr(), work.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()
  return crc.cpu().numpy().view(np.uint32)[:n], bad.cpu().numpy()[:n]


def test_crc_on_the_length_and_alignment_grid(lib):
  assert lib.MMT_RECORDS_PART == 256 * lib.MMT_RECORDS_PIECE
  blob, offs, lens, want = R.crc_grid(lib.MMT_RECORDS_PIECE, lib.MMT_RECORDS_PART)
  stored = np.asarray([R.mask(int(w)) for w in want], dtype=np.uint32)
  crc, bad = device_crc(lib, blob, offs, lens, stored)
  wrong = np.nonzero(crc != want)[0]
  print('records', len(want), 'wrong', [(int(lens[i]), int(offs[i]) % 16) for i in wrong[:20]])
  assert np.array_equal(crc, want)
  assert not bad.any()
  again, _ = device_crc(lib, blob, offs, lens, stored)     # the same bytes give the same words
  assert np.array_equal(again, crc)


def test_crc_of_a_thousand_short_records_and_the_rfc_vectors(lib):
  rng = np.random.default_rng(5)
  datas = [d for d, _ in R.CRC_VECTORS] + [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 41, size=1000)]
  lens = [len(d) for d in datas]
  offs = np.cumsum([0] + lens[:-1])
  blob = np.frombuffer(b''.join(datas), dtype=np.uint8).copy()
  want = np.asarray([R.crc32c(d) for d in datas], dtype=np.uint32)
  crc, bad = device_crc(lib, blob, offs, lens, [R.mask(int(w)) for w in want])
  assert [int(c) for c in crc[:5]] == [w for _, w in R.CRC_VECTORS]
  assert np.array_equal(crc, want) and not bad.any()


def test_crc_of_a_record_that_ends_at_the_last_byte(lib):
  rng = np.random.default_rng(6)
  piece, part = lib.MMT_RECORDS_PIECE, lib.MMT_RECORDS_PART
  for total, last in ((part + 77, part + 30), (1001, 1001), (piece + 3, 2), (5, 5)):
    blob = rng.integers(0, 256, size=total, dtype=np.uint8)           # an allocation of exactly `total` bytes
    offs, lens = [0, total - last], [total - last, last]
    crc, _ = device_crc(lib, blob, offs, lens)
    data = blob.tobytes()
    assert [int(c) for c in crc] == [R.crc32c(data[:total - last]), R.crc32c(data[total - last:])], (total, last)


def test_a_flipped_bit_marks_its_record_only(lib):
  rng = np.random.default_rng(7)
  part = lib.MMT_RECORDS_PART
  lens = [300, part + 37, 0, 129, 4000]
  datas = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]
  stored = [R.mask(R.crc32c(d)) for d in datas]
  offs = np.cumsum([0] + lens[:-1])
  clean = np.frombuffer(b''.join(datas), dtype=np.uint8)
  for victim in (1, 0, 4):
    for where in (0, lens[victim] // 2, lens[victim] - 1):
      blob = clean.copy()
      blob[offs[victim] + where] ^= 1 << (where % 8)
      _, bad = device_crc(lib, blob, offs, lens, stored)
      assert bad.tolist() == [int(i == victim) for i in range(len(lens))], (victim, where)


# ---------------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------------
IMAGE, PATCH, SEQ, BATCH = 32, 16, 32, 8
N_PATCH = (IMAGE // PATCH) ** 2
N_IMG = 2 + N_PATCH


@pytest.fixture(scope='module')
def vocab_path(tmp_path_factory):
  return R.write_vocab(tmp_path_factory.mktemp('vocab') / 'vocab.txt')


@pytest.fixture(scope='module')
def shards(tmp_path_factory):
  """20 records over 2 shards (validation order = record order), and the records."""
  recs = R.loader_records(20)
  d = tmp_path_factory.mktemp('plain')
  return R.write_shards(d, recs, 2), recs, str(d / '*.tfrecord')


def data_config(pattern, vocab_path, **kw):
  from mmt_amd import configs
  base = dict(input_path=pattern, vocab_filename=vocab_path, is_training=False, global_batch_size=BATCH, image_size=IMAGE,
              patch_size=PATCH, max_seq_len=SEQ, tasks='mlm', text_special_token_field_dict=json.dumps(R.FIELD_DICT),
              mlm_max_selections_per_seq=SEQ - N_IMG, mpp_max_selections_per_seq=N_PATCH, seed=11)
  base.update(kw)
  return configs.MmtPretrainDataConfig(**base)


@functools.lru_cache(maxsize=None)
def expected_image(name):
  """images_to_patch_features of the committed Pillow decode (the same call on the decoded pixels, so the comparison is
  bit for bit): (normalised, unnormalised, MPP ids) as CPU tensors."""
  from mmt_amd import feature_pipeline as fp
  out = fp.images_to_patch_features([torch.from_numpy(JC.expected(name).copy()).cuda()], IMAGE, PATCH, keep_unnormalized=True,
                                    output_channel_bits=3)
  return out['patch_embeddings'][0].cpu(), out['unnormalized_patch_embeddings'][0].cpu(), out['mpp_label_ids'][0].cpu()


@functools.lru_cache(maxsize=None)
def cpu_vocab(path):
  from mmt_amd import text_frontend
  return text_frontend.WordpieceVocab(path)


def expected_text(vocab_path, rec):
  from mmt_amd import text_frontend
  out = text_frontend.texts_to_token_features(cpu_vocab(vocab_path), [[rec['caption']], [rec['alt_text']]], list(R.FIELD_DICT.values()),
                                              SEQ, N_PATCH)
  return out['text_token_ids'][0], int(out['num_text_wordpieces'][0])


def masked_positions(positions_row):
  return {int(p) for p in positions_row.tolist() if p > 0}


def image_matches(inputs, b, name, mask_id):
  """The unmasked rows of example b's patch_embeddings equal the expected ones of `name`, the masked rows are zero."""
  norm, _, _ = expected_image(name)
  got = inputs['patch_embeddings'][b].cpu()
  tok = inputs['word_ids'][b, 2:N_IMG].cpu()
  for i in range(N_PATCH):
    if int(tok[i]) == mask_id:
      if bool(got[i].abs().max() != 0):
        return False
    elif not torch.equal(got[i], norm[i]):
      return False
  return True


def text_matches(inputs, b, vocab_path, rec):
  want, count = expected_text(vocab_path, rec)
  if int(inputs['valid_len'][b]) != N_IMG + count:
    return False
  got = inputs['word_ids'][b, N_IMG:].cpu()
  hidden = masked_positions(inputs['mlm_positions'][b])
  return all(int(got[t]) == int(want[t]) for t in range(SEQ - N_IMG) if t + N_IMG not in hidden)


def test_validation_pass_covers_every_record_in_order(lib, shards, vocab_path):
  from mmt_amd import pretrain_dataloader as pd
  _, recs, pattern = shards
  cfg = data_config(pattern, vocab_path)
  loader = pd.MmtPretrainDataLoader(cfg, device='cuda')
  mask_id = cpu_vocab(vocab_path).id('[MASK]')
  batches = list(loader.load())
  assert [b[0]['word_ids'].shape[0] for b in batches] == [8, 8, 4]          # one pass, the final short batch kept
  at = 0
  for inputs, labels in batches:
    for b in range(inputs['word_ids'].shape[0]):
      rec = recs[at]
      at += 1
      want_text, count = expected_text(vocab_path, rec)
      assert text_matches(inputs, b, vocab_path, rec), (at, rec)
      full = torch.cat([torch.tensor([cpu_vocab(vocab_path).id('[CLS]'), cpu_vocab(vocab_path).id('[PATCH]')] +
                                     [104 + i for i in range(N_PATCH)], dtype=torch.int32), want_text])
      pos, lab = inputs['mlm_positions'][b].cpu(), labels['mlm_label_ids'][b].cpu()
      for j in range(pos.numel()):
        if pos[j] > 0:
          assert int(lab[j]) == int(full[int(pos[j])]), (at, j)
      norm, unnorm, ids = expected_image(rec['image'])
      diff = (inputs['patch_embeddings'][b].cpu() - norm).abs().max()
      print(rec['image'], 'max |patch - expected| over all rows (masked rows are zeroed):', float(diff))
      assert image_matches(inputs, b, rec['image'], mask_id), (at, rec['image'])
      ppos, plab = inputs['mpp_positions'][b].cpu(), labels['mpp_label_ids'][b].cpu()
      for j in range(ppos.numel()):
        if ppos[j] > 0:
          assert int(plab[j]) == int(ids[int(ppos[j]) - 2]), (at, j)
  assert at == len(recs)


def test_itm_labels_say_where_the_text_belongs_to_the_image(lib, tmp_path, vocab_path):
  from mmt_amd import pretrain_dataloader as pd
  recs = R.loader_records(16, unique_texts=True)[:12] + R.loader_records(16)[12:16]     # 12 distinct images, then 4 again with other texts
  R.write_shards(tmp_path, recs, 2)
  cfg = data_config(str(tmp_path / '*.tfrecord'), vocab_path, tasks='mlm,itm')
  mask_id = cpu_vocab(vocab_path).id('[MASK]')
  batches = list(pd.MmtPretrainDataLoader(cfg, device='cuda').load())
  assert [b[0]['word_ids'].shape[0] for b in batches] == [8, 8, 8, 8]        # 2 matching batches of 8 -> 16 examples each
  ones = 0
  for k, (inputs, labels) in enumerate(batches):
    group = recs[(k // 2) * 8:(k // 2) * 8 + 8]
    for b in range(8):
      imgs = [i for i, r in enumerate(group) if image_matches(inputs, b, r['image'], mask_id)]
      txts = [i for i, r in enumerate(group) if text_matches(inputs, b, vocab_path, r)]
      assert len(imgs) == 1 and len(txts) == 1, (k, b, imgs, txts)
      assert int(labels['itm_label_ids'][b]) == int(imgs[0] == txts[0]), (k, b)
      ones += int(labels['itm_label_ids'][b])
    assert labels['itm_label_weights'].dtype == torch.float32 and bool((labels['itm_label_weights'] == 1).all())
  assert ones == 16


@pytest.mark.parametrize('dense', [False, True], ids=['structured', 'dense'])
def test_keys_shapes_and_dtypes_are_those_of_the_synthetic_batch(lib, shards, vocab_path, dense):
  from mmt_amd import input_utils
  from mmt_amd import pretrain_dataloader as pd
  cfg = data_config(shards[2], vocab_path, tasks='mlm,itm')
  got = next(pd.MmtPretrainDataLoader(cfg, device='cuda', dense_side_inputs=dense).load())
  want = input_utils.synthetic_batch(cfg, BATCH, 'cuda', vocab_size=len(cpu_vocab(vocab_path)), dense_side_inputs=dense)
  sig = lambda d: {k: ((tuple(v.shape), v.dtype) if torch.is_tensor(v) else type(v)) for k, v in d.items()}
  assert sig(got[0]) == sig(want[0])
  assert sig(got[1]) == sig(want[1])


def test_same_seed_same_batches_and_disjoint_files_per_rank(lib, tmp_path, vocab_path):
  from mmt_amd import pretrain_dataloader as pd
  R.write_shards(tmp_path, R.loader_records(24), 4)
  cfg = data_config(str(tmp_path / '*.tfrecord'), vocab_path, is_training=True, tasks='mlm,itm', cycle_length=2)

  def take(k, **kw):
    it = pd.MmtPretrainDataLoader(cfg, device='cuda', shuffle_buffer=8, example_shuffle_buffer=8).load(**kw)
    return [next(it) for _ in range(k)]
  a, b = take(3), take(3)
  for (ia, la), (ib, lb) in zip(a, b):
    for k in ia:
      assert torch.equal(ia[k], ib[k]) if torch.is_tensor(ia[k]) else ia[k] == ib[k], k
    for k in la:
      assert torch.equal(la[k], lb[k]), k
  loader = pd.MmtPretrainDataLoader(cfg, device='cuda')
  for training in (False, True):
    cfg.is_training = training
    streams = [loader._file_stream(r, 2) for r in range(2)]
    first = [[next(s) for _ in range(2)] for s in streams]               # one epoch: 4 files over 2 pipelines
    assert not set(first[0]) & set(first[1]) and sorted(first[0] + first[1]) == loader.files()
  cfg.is_training = True
  r1 = take(1, rank=1, num_replicas=2, batch_size=BATCH)                # the matching step needs more than 7 examples
  assert r1[0][0]['word_ids'].shape[0] == BATCH


def test_training_drops_short_texts_fills_every_batch_and_repeats(lib, tmp_path, vocab_path):
  from mmt_amd import pretrain_dataloader as pd
  recs = R.loader_records(24, short_every=4)                             # 18 records survive the filter per epoch
  R.write_shards(tmp_path, recs, 3)
  cfg = data_config(str(tmp_path / '*.tfrecord'), vocab_path, is_training=True, tasks='mlm,itm')
  it = pd.MmtPretrainDataLoader(cfg, device='cuda', shuffle_buffer=8, example_shuffle_buffer=8).load()
  seen = 0
  for _ in range(6):                                                     # 48 examples = 24 records behind the filter: more than one epoch
    inputs, labels = next(it)
    assert inputs['word_ids'].shape[0] == BATCH and labels['itm_label_ids'].shape[0] == BATCH
    assert int((inputs['valid_len'] - N_IMG).min()) >= 6
    seen += BATCH // 2
  assert seen > 18


def test_a_corrupt_payload_raises_naming_file_and_record(lib, tmp_path, vocab_path):
  from mmt_amd import pretrain_dataloader as pd
  recs = R.loader_records(5)
  path = R.write_shards(tmp_path, recs, 1)[0]
  data = bytearray(open(path, 'rb').read())
  at = sum(16 + len(R.record_payload(r)) for r in recs[:2]) + 12 + 40    # inside the third record's payload
  data[at] ^= 0x20
  open(path, 'wb').write(bytes(data))
  cfg = data_config(str(tmp_path / '*.tfrecord'), vocab_path)
  with pytest.raises(ValueError, match=r'shard-00000-of-00001\.tfrecord: record 2\b'):
    list(pd.MmtPretrainDataLoader(cfg, device='cuda').load())


def test_build_inputs_chooses_the_source(lib, shards, tmp_path, vocab_path):
  import mmt_amd
  from tests._parity import tiny_experiment
  exp = tiny_experiment()
  assert exp.task.train_data.input_path.startswith('gs://') or exp.task.train_data.input_path == ''
  task = mmt_amd.tasks.get_task(exp.task)
  inputs, _ = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2))
  assert task.input_source == 'synthetic' and inputs['word_ids'].shape == (2, 256)
  exp.task.train_data.vocab_filename = vocab_path
  exp.task.train_data.input_path = str(tmp_path / 'nothing-*.tfrecord')
  with pytest.raises(ValueError, match='matches no file'):
    task.build_inputs(exp.task.train_data, device='cuda', batch_size=2)
  exp.task.train_data.input_path = shards[2]
  exp.task.train_data.text_special_token_field_dict = json.dumps(R.FIELD_DICT)
  exp.task.train_data.tasks = 'mlm'
  exp.task.train_data.mlm_max_selections_per_seq = 58                    # every text position: whole words may exceed the tiny config's 8
  it = task.build_inputs(exp.task.train_data, device='cuda', batch_size=8, loader_args=dict(shuffle_buffer=8))
  inputs, labels = next(it)
  assert task.input_source == 'records' and inputs['word_ids'].shape == (8, 256) and 'itm_label_ids' not in labels


def test_one_train_step_on_a_loader_batch(lib, shards, vocab_path):
  import mmt_amd
  from mmt_amd import optimization
  from tests._parity import tiny_experiment
  exp = tiny_experiment()
  d = exp.task.train_data
  d.input_path, d.vocab_filename, d.text_special_token_field_dict = shards[2], vocab_path, json.dumps(R.FIELD_DICT)
  d.mlm_max_selections_per_seq = 58                                      # every text position: whole words may exceed the tiny config's 8
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(3)
  model = task.build_model().cuda()
  opt = optimization.create_optimizer(model, exp.trainer.optimizer_config)
  it = task.build_inputs(d, device='cuda', batch_size=8, loader_args=dict(shuffle_buffer=8, example_shuffle_buffer=8))
  out = task.train_step(next(it), model, opt, clip_norm=1.0, step=1, micro_batch_size=8)
  assert task.input_source == 'records' and np.isfinite(float(out['loss'])) and float(out['loss']) > 0
