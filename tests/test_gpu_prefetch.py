"""`prefetch_buffer_size` on the GPU: the loaders on records behind a `prefetch.Prefetcher` (worker thread, side stream,
event hand-over) against the plain loaders of the same seed, bit for bit; the train step -- recorded as a HIP graph while
the worker is producing, and eager -- fed either way; an evaluation that ends early; a corrupt record.  The shards are
those tests/_record_cases.py writes from the committed JPEG fixtures.  Every prefetcher has `timeout = 60`, so a wrong
gate fails a test instead of hanging the run."""
import copy
import json
import threading

import pytest
import torch

import __graft_entry__  # noqa: F401
from tests import _record_cases as R
from tests._parity import tiny_experiment

pytestmark = pytest.mark.gpu

BATCH = 8
LOADER_ARGS = dict(shuffle_buffer=8, example_shuffle_buffer=8)


@pytest.fixture(scope='module')
def shards(tmp_path_factory):
  """24 records over 4 shards, and the vocabulary: (pattern, vocab path)."""
  d = tmp_path_factory.mktemp('prefetch')
  R.write_shards(d, R.loader_records(24), 4)
  return str(d / '*.tfrecord'), R.write_vocab(tmp_path_factory.mktemp('vocab') / 'vocab.txt')


def on_records(data_cfg, pattern, vocab, **kw):
  v = copy.deepcopy(data_cfg)
  v.input_path, v.vocab_filename, v.text_special_token_field_dict = pattern, vocab, json.dumps(R.FIELD_DICT)
  v.global_batch_size, v.min_shift, v.cycle_length = BATCH, 1, 2
  if hasattr(v, 'mlm_max_selections_per_seq'):
    v.mlm_max_selections_per_seq = 58                            # every text position: whole words may exceed the tiny config's 8
  for k, val in kw.items():
    setattr(v, k, val)
  return v


def pretraining(shards, dropout=0.0, **kw):
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  if dropout:
    exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': dropout, 'attention_probs_dropout_prob': dropout}}}}})
  exp.task.train_data = on_records(exp.task.train_data, *shards, **kw)
  return exp


def classification(shards, **kw):
  from mmt_amd import configs
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp = configs.get_exp_config('mmt/classification')
  keep = {k: v for k, v in exp.task.train_data.as_dict().items() if hasattr(cexp.task.train_data, k)}
  keep.update(label_field='itm_label_ids', label_weights_field='itm_label_weights', pos_weights_field='itm_pos_weights',
              negative_positive_ratio=1)
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(), 'num_classes': 2,
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': keep}}, strict=False)
  cexp.task.train_data = on_records(cexp.task.train_data, *shards, **kw)
  return cexp


def workers():
  from mmt_amd import prefetch
  return [t for t in threading.enumerate() if t.name.startswith(prefetch.THREAD_PREFIX)]


def inputs_of(exp, depth, **build):
  """(task, iterator) of the experiment's train data with `prefetch_buffer_size = depth`."""
  import mmt_amd
  from mmt_amd import prefetch
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  cfg = copy.deepcopy(exp.task.train_data)
  cfg.prefetch_buffer_size = depth
  data = task.build_inputs(cfg, device='cuda', batch_size=BATCH, loader_args=LOADER_ARGS, **build)
  assert isinstance(data, prefetch.Prefetcher) == bool(depth) and task.input_source == 'records'
  if depth:
    assert task.input_prefetch is data and data.depth == depth
    data.timeout = 60
  return task, data


def assert_same_batches(exp, depth, n=12):
  _, plain = inputs_of(exp, 0)
  _, ahead = inputs_of(exp, depth)
  try:
    for i in range(n):
      want = next(plain)
      got = next(ahead)
      for w_tree, g_tree in zip(want, got):                        # compared at once: the event alone orders the two streams
        assert w_tree.keys() == g_tree.keys()
        for k, w in w_tree.items():
          if torch.is_tensor(w):
            assert g_tree[k].dtype == w.dtype and torch.equal(g_tree[k], w), (i, k)
          else:
            assert g_tree[k] == w, (i, k)
  finally:
    ahead.close()
  assert not workers()


# ---- (a), (b): the loaders ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 3])
def test_pretraining_loader_in_training_mode_gives_the_plain_loaders_batches(shards, depth):
  assert_same_batches(pretraining(shards, tasks='mlm,itm'), depth)


def test_classification_loader_gives_the_plain_loaders_batches(shards):
  assert_same_batches(classification(shards), 2)


def test_packed_rows_give_the_plain_loaders_batches(shards):
  assert_same_batches(pretraining(shards, tasks='mlm', pack_rows=2, pack_row_len=512), 2)


# ---- (c), (d): the train step ---------------------------------------------------------------------------------------------------
def run_steps(shards, depth, eager_only, n=4):
  from mmt_amd import distribute, graphed, optimization, tasks
  exp = pretraining(shards, dropout=0.1, tasks='mlm,itm')
  exp.task.micro_batch_size = BATCH                            # one micro-step per call
  task, data = inputs_of(exp, depth)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt_cfg = exp.trainer.optimizer_config
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()), reduce=tasks.gradient_reduce_mode(exp.task))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  step = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, clip_norm=opt_cfg.gradient_clip_norm, eager_steps=1)
  if eager_only:
    step.eager_left = 1 << 62
  try:
    losses = [float(step(next(data), i)['loss']) for i in range(1, n + 1)]
    assert (step.graph is None) == eager_only
    if depth:
      assert data.alive                                          # the worker was producing all along (the loader repeats)
    params = torch.cat([s['param'] for s in optimizer.slabs]).clone()
  finally:
    step.close()
    if depth:
      data.close()
  assert not workers()
  return losses, params


@pytest.mark.parametrize('eager_only', [False, True], ids=['recorded', 'eager'])
def test_four_steps_fed_from_the_prefetched_loader_equal_the_plain_run(shards, eager_only):
  """The dropout seeds are a function of the step and the batches are the loader's, so losses and weights must be equal
  bit for bit.  Recorded: the first call runs eagerly, the second records -- under the capture gate, while the worker
  is producing -- and replays, the others replay."""
  want = run_steps(shards, 0, eager_only)
  got = run_steps(shards, 2, eager_only)
  print('losses plain', want[0], 'prefetched', got[0])
  assert want[0] == got[0] and len(set(got[0])) == 4
  assert torch.equal(want[1], got[1])


# ---- (e): an evaluation that ends early -----------------------------------------------------------------------------------------
def test_an_early_ended_evaluation_leaves_no_worker(shards):
  import mmt_amd
  from mmt_amd import evaluation
  exp = pretraining(shards, tasks='mlm')
  vcfg = on_records(exp.task.train_data, *shards, tasks='mlm', is_training=False, global_batch_size=4)
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(3)
  model = task.build_model().cuda()
  want = evaluation.evaluate(task, model, vcfg, device='cuda', steps=2)
  vcfg.prefetch_buffer_size = 2
  got = evaluation.evaluate(task, model, vcfg, device='cuda', steps=2)          # 24 records: four more batches are there
  assert got == want and got['validation_batches'] == 2
  assert task.input_prefetch is not None and not task.input_prefetch.alive and not workers()
  whole = evaluation.evaluate(task, model, vcfg, device='cuda', steps=-1)
  assert whole['validation_batches'] == 6 and not workers()


# ---- (f): a corrupt record ------------------------------------------------------------------------------------------------------
def test_a_corrupt_record_raises_from_next_behind_the_batches_before_it(tmp_path):
  import mmt_amd
  recs = R.loader_records(12)
  path = R.write_shards(tmp_path, recs, 1)[0]
  data = bytearray(open(path, 'rb').read())
  at = sum(16 + len(R.record_payload(r)) for r in recs[:9]) + 12 + 40      # inside the tenth record's payload
  data[at] ^= 0x20
  open(path, 'wb').write(bytes(data))
  shards = (str(tmp_path / '*.tfrecord'), R.write_vocab(tmp_path / 'vocab.txt'))
  exp = pretraining(shards, tasks='mlm', is_training=False)

  def drain(depth):
    task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
    cfg = copy.deepcopy(exp.task.train_data)
    cfg.prefetch_buffer_size = depth
    it = task.build_inputs(cfg, device='cuda', batch_size=2)
    if depth:
      it.timeout = 60
    seen = []
    try:
      with pytest.raises(ValueError) as e:
        while True:
          seen.append(next(it)[0]['word_ids'].clone())
    finally:
      if depth:
        it.close()
    return seen, str(e.value)

  want, message = drain(0)
  assert 'shard-00000-of-00001.tfrecord: record 9' in message
  got, again = drain(2)
  assert again == message and len(got) == len(want)
  for w, g in zip(want, got):
    assert torch.equal(w, g)
  assert not workers()
