"""The validation loop on the GPU (mmt_amd/evaluation.py, mmt_amd/train.py): `evaluate` against a hand-written loop and
the numpy metrics of oracle/metrics.py, the recorded step against the eager one, evaluations between train steps, the
best checkpoint and `eval` mode through `run_experiment`, packed validation batches and two ranks on one GPU.

Shapes: `tiny_experiment(S=256, radius=32, n_global=8)` (2 layers, hidden 128, 2 heads) and its classification twin, bf16,
per-replica batch 4; validation shards of 18 records written at test time from the committed JPEG fixtures.  Every
comparison between two runs of the same kernels is bitwise.

What 18 records become.  The pretraining loader without the matching step (`tasks: mlm`) emits them as four batches of 4
and one of 2: the case with the short last batch.  With the matching step (`tasks: mlm,itm`, and the classification
loader) every whole group of records becomes positives plus as many negatives and the records short of a group are
dropped (pretrain_dataloader.py `matched`, classification_dataloader.py `matched`), so 18 records are 32 examples,
eight full batches and no short one: those two configurations assert 8, the number the loaders' rule gives, and the
short batch is asserted where it exists."""
import copy
import json
import os
import shutil
import socket
import time
import warnings

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from oracle import metrics as om
from tests import _record_cases as R
from tests._parity import tiny_experiment

pytestmark = pytest.mark.gpu

BATCH = 4
N_RECORDS = 18


# ---- configurations and shards --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shards(tmp_path_factory):
  """18 records over 2 shards, and the vocabulary: (pattern, vocab path)."""
  d = tmp_path_factory.mktemp('validation')
  R.write_shards(d, R.loader_records(N_RECORDS), 2)
  return str(d / '*.tfrecord'), R.write_vocab(tmp_path_factory.mktemp('vocab') / 'vocab.txt')


def _on_records(data_cfg, pattern, vocab, **kw):
  """A copy of a data config that reads the shards as validation data, per-replica batch 4."""
  v = copy.deepcopy(data_cfg)
  v.input_path, v.vocab_filename, v.text_special_token_field_dict = pattern, vocab, json.dumps(R.FIELD_DICT)
  v.is_training, v.global_batch_size, v.min_shift = False, BATCH, 1          # the matching step needs batch > ratio + 1 + min_shift
  if hasattr(v, 'mlm_max_selections_per_seq'):
    v.mlm_max_selections_per_seq = 58                            # every text position: whole words may exceed the tiny config's 8
  for k, val in kw.items():
    setattr(v, k, val)
  return v


def pretraining(shards, **kw):
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.task.train_data.global_batch_size = BATCH
  exp.task.validation_data = _on_records(exp.task.train_data, *shards, **kw)
  return exp


def classification(shards, **kw):
  """The classification twin of the tiny experiment (tests/test_checkpoint.py:48-52), two classes: accuracy and AUC."""
  from mmt_amd import configs
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp = configs.get_exp_config('mmt/classification')
  keep = {k: v for k, v in exp.task.train_data.as_dict().items() if hasattr(cexp.task.train_data, k)}
  keep.update(global_batch_size=BATCH, label_field='itm_label_ids', label_weights_field='itm_label_weights',
              pos_weights_field='itm_pos_weights', negative_positive_ratio=1)
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(), 'num_classes': 2,
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': keep}}, strict=False)
  cexp.task.validation_data = _on_records(cexp.task.train_data, *shards, **kw)
  return cexp


def build(exp, seed=3):
  import mmt_amd
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(seed)
  return task, task.build_model().cuda()


CASES = {
    # name: (experiment, validation data overrides, batch sizes the loader emits for 18 records)
    'pretrain-mlm': (pretraining, dict(tasks='mlm'), [4, 4, 4, 4, 2]),
    'pretrain-mlm-itm': (pretraining, dict(tasks='mlm,itm'), [4] * 8),
    'classification': (classification, {}, [4] * 8),
    'pretrain-mlm-packed': (pretraining, dict(tasks='mlm', pack_rows=2, pack_row_len=512), None),
}


# ---- the hand-written loop and the oracle ----------------------------------------------------------------------------------
def manual_loop(task, model, vcfg):
  """`validation_step` over a fresh iterator under no_grad with fresh metrics, read with `metrics.results`; and, from a
  second forward of every batch (the kernels are deterministic), what the numpy metrics of oracle/metrics.py need."""
  from mmt_amd import metrics as M
  metrics, loss_mean = task.build_metrics(training=False), M.Mean('validation_loss')
  seen = []
  with torch.no_grad():
    for inputs, labels in task.build_inputs(vcfg, device='cuda', rank=0):
      out = task.validation_step((inputs, labels), model, metrics=metrics)
      loss_mean.update_state(out[task.loss])
      fwd = dict(inputs, flat_positions=True) if inputs.get('example_starts') is not None else inputs
      outputs = model(**fwd, training=False)
      seen.append(dict(size=int(inputs['word_ids'].shape[0]), loss=float(out[task.loss]),
                       labels={k: v.float().cpu().numpy() for k, v in labels.items()},
                       logits={k: v.float().cpu().numpy() for k, v in outputs.items() if k.endswith('_logits')}))
  want = {'validation_loss': float(loss_mean.result()), **{f'validation_{k}': v for k, v in M.results(metrics).items()},
          'validation_batches': len(seen)}
  return want, seen


def oracle_metrics(task, seen):
  """name -> (value, tolerance of tests/test_metrics.py) from the per-batch outputs."""
  from mmt_amd import tasks
  out = {}
  st = np.zeros(2, np.float32)
  for b in seen:
    st = om.mean_update(st, np.float32(b['loss']))
  out['validation_loss'] = (float(om.divide_no_nan(st[0], st[1])), 1e-5)
  if isinstance(task, tasks.PretrainingTask):
    heads = [('mlm', 'mlm_label_weights', True)] + ([('itm', 'itm_label_weights', False)] if 'itm_label_ids' in seen[0]['labels'] else [])
    for head, wkey, masked in heads:
      st = np.zeros(2, np.float32)
      for b in seen:
        w = b['labels'][wkey]
        if masked and 'itm_label_ids' in b['labels']:
          w = w * b['labels']['itm_label_ids'][:, None]
        st = om.sparse_categorical_accuracy_update(st, b['labels'][f'{head}_label_ids'], b['logits'][f'{head}_logits'], w)
      out[f'validation_{head}_accuracy'] = (float(om.divide_no_nan(st[0], st[1])), 1e-6)
  else:
    acc, auc = np.zeros(2, np.float32), np.zeros((4, 200), np.float32)
    for b in seen:
      y, w, lg = b['labels']['itm_label_ids'], b['labels']['itm_label_weights'], b['logits']['itm_logits']
      acc = om.sparse_categorical_accuracy_update(acc, y, lg, w)
      e = np.exp(lg - lg.max(1, keepdims=True))
      auc = om.auc_update(auc, y, (e / e.sum(1, keepdims=True))[:, 1], w)
    out['validation_cls_accuracy'] = (float(om.divide_no_nan(acc[0], acc[1])), 1e-6)
    out['validation_auc'] = (float(om.auc_pr_result(auc)), 2e-5)
  return out


@pytest.fixture(scope='module')
def references(shards):
  """Per case, computed once and left unchanged: the task, the model, the validation config, the hand-written loop's
  result and the per-batch outputs."""
  cache = {}

  def get(name):
    if name not in cache:
      make, kw, sizes = CASES[name]
      exp = make(shards, **kw)
      task, model = build(exp)
      want, seen = manual_loop(task, model, exp.task.validation_data)
      cache[name] = dict(exp=exp, task=task, model=model, vcfg=exp.task.validation_data, want=want, seen=seen, sizes=sizes)
    return cache[name]
  return get


# ---- 1. equals the manual loop; 6. packed validation batches -------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_evaluate_equals_the_manual_loop_eager_and_recorded(references, name):
  from mmt_amd import evaluation
  ref = references(name)
  task, model, vcfg, want, seen = ref['task'], ref['model'], ref['vcfg'], ref['want'], ref['seen']
  sizes = [b['size'] for b in seen]
  print(name, 'batches', sizes, json.dumps(want))
  if ref['sizes'] is not None:
    assert sizes == ref['sizes']
  else:                                                          # packed: rows, not examples, lead; every batch has the static shape
    assert sizes == [2] * len(sizes) and len(sizes) >= 3
  if name == 'pretrain-mlm':
    assert want['validation_batches'] == 5
  assert want['validation_loss'] > 0 and np.isfinite(want['validation_loss'])
  was_training = model.training
  with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter('always')
    eager = evaluation.evaluate(task, model, vcfg, device='cuda', rank=0, steps=-1)
    step = evaluation.GraphedEvalStep(task, model, graph=True)
    recorded = evaluation.evaluate(task, model, vcfg, device='cuda', rank=0, steps=-1, step_fn=step)
    again = evaluation.evaluate(task, model, vcfg, device='cuda', rank=0, steps=-1, step_fn=step)      # the graph outlives an evaluation
  ours = [str(w.message) for w in caught if 'mmt_amd' in w.filename]
  assert not ours, ours                                          # no warning: not for the short batch, not for a failed capture
  assert model.training == was_training
  assert eager == want
  assert recorded == want and again == want
  assert list(eager) == list(want) and type(eager['validation_batches']) is int
  # the first batch ran eagerly, the second recorded, the full batches behind it replayed, the short one ran eagerly
  full = sum(1 for s in sizes if s == sizes[0])
  assert step.graph is not None and step.replays == (full - 1) + full
  step.close()
  # against the numpy metrics, fed the per-batch outputs
  for key, (value, tol) in oracle_metrics(task, seen).items():
    print(f'  {key}: {eager[key]:.7f} oracle {value:.7f}')
    assert abs(eager[key] - value) < tol, key
  if name == 'classification':
    assert 0 < eager['validation_auc'] <= 1 and 0 <= eager['validation_cls_accuracy'] <= 1
  # a count of batches stops the pass early
  assert evaluation.evaluate(task, model, vcfg, device='cuda', rank=0, steps=2)['validation_batches'] == 2


def test_switch_and_fallback(references, monkeypatch):
  """MMT_STEP_GRAPH=0 keeps the step eager; a capture that raises falls back to eager steps with one warning and the
  same result."""
  from mmt_amd import evaluation
  ref = references('pretrain-mlm')
  task, model, vcfg, want = ref['task'], ref['model'], ref['vcfg'], ref['want']
  monkeypatch.setenv('MMT_STEP_GRAPH', '0')
  off = evaluation.make_eval_step(task, model, 'cuda')
  assert evaluation.evaluate(task, model, vcfg, device='cuda', steps=-1, step_fn=off) == want and off.graph is None
  monkeypatch.delenv('MMT_STEP_GRAPH')
  assert evaluation.make_eval_step(task, model, 'cuda').use_graph == evaluation.GRAPH_DEFAULT
  step = evaluation.GraphedEvalStep(task, model, graph=True)

  def refuse(batch):
    raise RuntimeError('this configuration cannot be captured')
  monkeypatch.setattr(step, '_record', refuse)
  with pytest.warns(UserWarning, match='not recorded as a HIP graph') as caught:
    got = evaluation.evaluate(task, model, vcfg, device='cuda', steps=-1, step_fn=step)
  assert len([w for w in caught if 'not recorded' in str(w.message)]) == 1
  assert got == want and step.graph is None and step.replays == 0


# ---- 2. sees current weights ------------------------------------------------------------------------------------------------
def test_recorded_step_sees_the_weights_the_optimizer_wrote(shards):
  from mmt_amd import distribute, evaluation, optimization
  exp = pretraining(shards, tasks='mlm,itm')
  task, model = build(exp, seed=4)
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()))
  opt = optimization.create_optimizer(model, exp.trainer.optimizer_config, reducer=reducer)
  assert hasattr(opt, 'slabs')                                   # the fused optimizer: masters and bf16 shadows written in place
  optimization.set_learning_rate(opt, 1e-3)
  vcfg = exp.task.validation_data
  step = evaluation.GraphedEvalStep(task, model, graph=True)
  first = evaluation.evaluate(task, model, vcfg, device='cuda', steps=-1, step_fn=step)
  assert step.graph is not None
  batch = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=BATCH))
  for s in (1, 2):
    task.train_step(batch, model, opt, reducer=reducer, clip_norm=1.0, step=s, micro_batch_size=BATCH)
  replays = step.replays
  second = evaluation.evaluate(task, model, vcfg, device='cuda', steps=-1, step_fn=step)
  assert step.replays == replays + 8                             # every batch of the second evaluation was a replay
  eager = evaluation.evaluate(task, model, vcfg, device='cuda', steps=-1)
  print('before', first['validation_loss'], 'after two train steps', second['validation_loss'])
  assert second == eager
  assert second['validation_loss'] != first['validation_loss']
  step.close()


# ---- 3. the training trajectory; 4. best checkpoint; 5. eval mode ------------------------------------------------------------
def trainer_experiment(train_steps=4, **trainer):
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': 0.1, 'attention_probs_dropout_prob': 0.1}}},
                         'train_data': {'global_batch_size': BATCH}, 'micro_batch_size': BATCH},
                'runtime': {'mixed_precision_dtype': 'bfloat16'},
                'trainer': dict(train_steps=train_steps, checkpoint_interval=0, validation_interval=2, validation_steps=3, **trainer)})
  exp.task.validation_data = copy.deepcopy(exp.task.train_data)              # synthetic, like the train data
  exp.task.validation_data.is_training = False
  return exp


BEST = dict(best_checkpoint_export_subdir='best_ckpt', best_checkpoint_eval_metric='validation_loss', best_checkpoint_metric_comp='lower')


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
  """One run with validation (and the best checkpoint) and the same run without, MMT_STEP_GRAPH at its default (the
  train step recorded, the validation step as `evaluation.GRAPH_DEFAULT` says); and the run with validation once more
  with MMT_STEP_GRAPH=1, which records the validation step too."""
  from mmt_amd import train
  out = {}
  with pytest.MonkeyPatch.context() as mp:
    for name, mode, trainer, env in (('with', 'train_and_eval', BEST, None), ('without', 'train', {}, None),
                                     ('recorded', 'train_and_eval', BEST, '1')):
      mp.delenv('MMT_STEP_GRAPH', raising=False)
      if env is not None:
        mp.setenv('MMT_STEP_GRAPH', env)
      d = tmp_path_factory.mktemp(name)
      model, logs = train.run_experiment(trainer_experiment(**trainer), mode, str(d), log_every=1)
      assert train.run_experiment.last_step_launch == 'graph'
      out[name] = dict(dir=str(d), model=model, logs=logs)
  return out


def _validation_entries(logs):
  return [e for e in logs if 'validation_loss' in e]


def _same(a, b, where=''):
  if torch.is_tensor(a):
    assert torch.is_tensor(b) and torch.equal(a, b), where
  elif isinstance(a, dict):
    assert a.keys() == b.keys(), where
    for k in a:
      _same(a[k], b[k], f'{where}.{k}')
  elif isinstance(a, (list, tuple)):
    assert len(a) == len(b), where
    for i, (x, y) in enumerate(zip(a, b)):
      _same(x, y, f'{where}[{i}]')
  else:
    assert a == b, where


def test_validation_leaves_the_training_trajectory_untouched(runs):
  from mmt_amd import checkpoint
  a, b = runs['with'], runs['without']
  for (n, p), q in zip(a['model'].named_parameters(), b['model'].parameters()):
    assert torch.equal(p, q), n
  ca, cb = (torch.load(checkpoint.latest_checkpoint(r['dir']), map_location='cpu', weights_only=True) for r in (a, b))
  assert ca['step'] == cb['step'] == 4 and ca['optimizer'] is not None
  _same(ca['optimizer'], cb['optimizer'], 'optimizer')             # optimizer.state_dict() of both runs, as their last checkpoint holds it
  _same(ca['items'], cb['items'], 'items')
  train_a = [{k: v for k, v in e.items() if k != 'elapsed_s'} for e in a['logs'] if 'loss' in e]
  train_b = [{k: v for k, v in e.items() if k != 'elapsed_s'} for e in b['logs'] if 'loss' in e]
  assert train_a == train_b and len(train_a) == 4
  entries = _validation_entries(a['logs'])
  print(json.dumps(entries))
  assert [e['step'] for e in entries] == [2, 4] and all(e['validation_batches'] == 3 for e in entries)
  assert entries[0]['validation_loss'] != entries[1]['validation_loss']
  assert {k: v for k, v in entries[0].items() if k != 'step'} != {k: v for k, v in entries[1].items() if k != 'step'}
  assert not _validation_entries(b['logs'])                       # `train` mode runs no validation
  # the validation step recorded as well (MMT_STEP_GRAPH=1): the same trajectory and the same validation entries
  c = runs['recorded']
  for (n, p), q in zip(c['model'].named_parameters(), b['model'].parameters()):
    assert torch.equal(p, q), n
  cc = torch.load(checkpoint.latest_checkpoint(c['dir']), map_location='cpu', weights_only=True)
  _same(cc['optimizer'], cb['optimizer'], 'optimizer, validation step recorded')
  assert _validation_entries(c['logs']) == entries


def _best_dir(model_dir):
  d = os.path.join(model_dir, 'best_ckpt')
  files = sorted(os.listdir(d))
  info = json.load(open(os.path.join(d, 'info.json')))
  return d, files, info


def test_best_checkpoint_through_run_experiment(runs, tmp_path):
  import mmt_amd
  from mmt_amd import checkpoint, evaluation, train
  a = runs['with']
  entries = _validation_entries(a['logs'])
  losses = [e['validation_loss'] for e in entries]
  best = entries[int(np.argmin(losses))]
  d, files, info = _best_dir(a['dir'])
  assert files == [f'ckpt-{best["step"]}.pt', 'info.json']
  assert info['step'] == best['step'] and info['metric_name'] == 'validation_loss' and info['metric_comp'] == 'lower'
  assert info['metric_value'] == best['validation_loss']
  assert info['eval_logs'] == {k: v for k, v in best.items() if k != 'step'}
  # the best file restored into a fresh model reproduces the stored metric
  exp = trainer_experiment(**BEST)
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(99)
  fresh = task.build_model().cuda()
  assert checkpoint.restore(os.path.join(d, files[0]), fresh) == best['step']
  again = evaluation.evaluate(task, fresh, exp.task.validation_data, device='cuda', steps=3)
  assert again == info['eval_logs']
  # a resumed run whose results are worse leaves the better checkpoint alone: the stored best is made unbeatable (no
  # cross-entropy is below zero) and two more steps run on a copy of the directory
  model_dir = str(tmp_path / 'resumed')
  shutil.copytree(a['dir'], model_dir)
  d2 = os.path.join(model_dir, 'best_ckpt')
  info2 = dict(info, metric_value=-1.0)
  json.dump(info2, open(os.path.join(d2, 'info.json'), 'w'))
  before = open(os.path.join(d2, files[0]), 'rb').read()
  _, logs = train.run_experiment(trainer_experiment(train_steps=6, **BEST), 'train_and_eval', model_dir, log_every=1)
  assert [e['step'] for e in logs if 'loss' in e] == [4, 5]      # resumed after step 4 (train entries count from 0)
  assert [e['step'] for e in _validation_entries(logs)] == [6]   # 6 is a multiple of the interval and the end
  _, files2, after = _best_dir(model_dir)
  assert files2 == files and after == info2 and open(os.path.join(d2, files[0]), 'rb').read() == before
  # ... and one that is better replaces it
  json.dump(dict(info, metric_value=1e9), open(os.path.join(d2, 'info.json'), 'w'))
  _, logs = train.run_experiment(trainer_experiment(train_steps=7, **BEST), 'train_and_eval', model_dir, log_every=1)
  _, files3, info3 = _best_dir(model_dir)
  assert files3 == ['ckpt-7.pt', 'info.json'] and info3['step'] == 7
  assert info3['metric_value'] == _validation_entries(logs)[-1]['validation_loss']


def test_eval_mode_restores_evaluates_and_trains_nothing(runs, tmp_path, capsys):
  from mmt_amd import checkpoint, train
  a = runs['with']
  latest = checkpoint.latest_checkpoint(a['dir'])
  saved = torch.load(latest, map_location='cpu', weights_only=True)
  model, logs = train.run_experiment(trainer_experiment(**BEST), 'eval', a['dir'], log_every=1)
  assert len(logs) == 1 and logs[0]['step'] == 4 and logs[0]['restored_from'] == latest
  final = _validation_entries(a['logs'])[-1]
  assert {k: v for k, v in logs[0].items() if k != 'restored_from'} == final
  for (n, p), q in zip(model.named_parameters(), a['model'].parameters()):
    assert torch.equal(p, q), n                                  # the restored weights, unchanged
  assert checkpoint.latest_checkpoint(a['dir']) == latest
  _same(torch.load(latest, map_location='cpu', weights_only=True), saved, 'checkpoint')     # nothing was written
  # without a checkpoint the JSON line says so, and the initial weights are evaluated
  capsys.readouterr()
  _, logs = train.run_experiment(trainer_experiment(), 'eval', str(tmp_path / 'empty'), log_every=1)
  line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
  assert line['restored_from'] is None and line['step'] == 0 and line['validation_batches'] == 3
  assert logs[-1] == line


def test_run_experiment_checks_before_the_first_train_step(tmp_path):
  from mmt_amd import train
  exp = trainer_experiment(best_checkpoint_export_subdir='best_ckpt', best_checkpoint_eval_metric='acu')
  with pytest.raises(ValueError, match="'acu'"):
    train.run_experiment(exp, 'train_and_eval', str(tmp_path / 'a'), log_every=1)
  exp = trainer_experiment()
  exp.trainer.validation_steps = -1
  with pytest.raises(ValueError, match='endless synthetic'):
    train.run_experiment(exp, 'train_and_eval', str(tmp_path / 'b'), log_every=1)
  assert not os.path.exists(tmp_path / 'a') and not os.path.exists(tmp_path / 'b')       # nothing trained, nothing saved


# ---- 7. two ranks on one GPU ---------------------------------------------------------------------------------------------
def _free_port():
  s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_worker(rank, world, port, out, pattern, vocab, export_root):
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                    HSA_ENABLE_IPC_MODE_LEGACY='0', MMT_DIST_BACKEND='gloo', MMT_ONE_GPU='1')
  import torch.distributed as dist
  import mmt_amd
  from mmt_amd import evaluation
  dist.init_process_group('gloo')
  torch.cuda.set_device(0)
  exp = pretraining((pattern, vocab), tasks='mlm', global_batch_size=BATCH * world)
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16, num_replicas=world)
  torch.manual_seed(5)                                   # identical replicas
  model = task.build_model().cuda()
  vcfg = exp.task.validation_data
  logs = evaluation.evaluate(task, model, vcfg, device='cuda', rank=rank, steps=-1)
  # the same evaluation in its two halves, with the local sums dumped before the read
  step = evaluation.make_eval_step(task, model, 'cuda')
  n = evaluation.run_batches(task, step, vcfg, device='cuda', rank=rank, steps=-1)
  local = {m.name: m.ensure('cuda').state.clone().cpu() for m in step.all_metrics()}
  synced = {m.name: m.synced_state().cpu() for m in step.all_metrics()}
  halves = evaluation.read_results(step, 'cuda')
  step.close()
  exporter = evaluation.BestCheckpointExporter(os.path.join(export_root, f'best_ckpt_of_rank{rank}'), 'validation_loss', 'lower', rank=rank)
  exported = exporter.maybe_export(1, logs, model, None)
  out[rank] = dict(logs=logs, halves=halves, n=n, local=local, synced=synced, exported=exported)
  dist.destroy_process_group()


def test_two_ranks_on_one_gpu_read_the_same_sums(tmp_path):
  """Rank 0's file holds 8 records (two batches of 4), rank 1's holds 4 (one batch)."""
  import torch.multiprocessing as mp
  recs = R.loader_records(12)
  for name, part in (('part-0.tfrecord', recs[:8]), ('part-1.tfrecord', recs[8:])):
    with open(tmp_path / name, 'wb') as f:
      for rec in part:
        f.write(R.frame(R.record_payload(rec)))
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  world = 2
  with mp.Manager() as mgr:
    out = mgr.dict()
    ctx = mp.spawn(_rank_worker, args=(world, _free_port(), out, str(tmp_path / 'part-*.tfrecord'), vocab, str(tmp_path)),
                   nprocs=world, join=False)
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=1):                               # raises when a rank failed
      if time.monotonic() > deadline:
        for p in ctx.processes:
          p.kill()
        pytest.fail('the ranks did not finish in time')
    r0, r1 = out[0], out[1]
  assert (r0['n'], r1['n']) == (2, 1)
  print(json.dumps(r0['logs']))
  assert r0['logs'] == r1['logs'] == r0['halves'] == r1['halves']
  assert r0['logs']['validation_batches'] == 3 and r0['logs']['validation_loss'] > 0
  assert r0['local'].keys() == r0['synced'].keys() and 'validation_loss' in r0['local']
  for name in r0['local']:
    assert torch.equal(r0['synced'][name], r1['synced'][name]), name
    assert torch.equal(r0['synced'][name], r0['local'][name] + r1['local'][name]), name      # an fp32 sum of two operands has one order
  assert not torch.equal(r0['local']['validation_loss'], r1['local']['validation_loss'])
  assert r0['exported'] and r1['exported']                       # the same decision on both ranks ...
  assert sorted(os.listdir(tmp_path / 'best_ckpt_of_rank0')) == ['ckpt-1.pt', 'info.json']
  assert not os.path.exists(tmp_path / 'best_ckpt_of_rank1')     # ... and rank 0 alone writes
