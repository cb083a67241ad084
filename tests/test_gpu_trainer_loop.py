"""The trainer's loop mode on the GPU (mmt_amd/train.py, mmt_amd/summaries.py): loops of `steps_per_loop` steps with one
host read each, TensorBoard scalars under `model_dir/train` and `model_dir/<validation_summary_subdir>`, recovery from
the latest checkpoint.  DESIGN.md section 4, "Trainer loop, summaries, recovery".

Shapes: `tiny_experiment(S=256, radius=32, n_global=8)` (2 layers, hidden 128, 2 heads), bf16, dropout 0.1, per-replica
batch 4, synthetic data, at most 7 train steps per run.  Every comparison between two runs of the same kernels is bitwise."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from tests._parity import tiny_experiment

pytestmark = pytest.mark.gpu

BATCH = 4
LINE_HEAD = ['step', 'training_loss', 'learning_rate', 'steps_per_second']


def experiment(train_steps, **trainer):
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': 0.1, 'attention_probs_dropout_prob': 0.1}}},
                         'train_data': {'global_batch_size': BATCH}, 'micro_batch_size': BATCH},
                'runtime': {'mixed_precision_dtype': 'bfloat16'},
                'trainer': dict(dict(train_steps=train_steps, checkpoint_interval=0, validation_interval=3, validation_steps=2),
                                **trainer)}, strict=True)
  exp.task.validation_data = copy.deepcopy(exp.task.train_data)              # synthetic, like the train data
  exp.task.validation_data.is_training = False
  return exp


def set_graph(monkeypatch, value):
  monkeypatch.delenv('MMT_STEP_GRAPH', raising=False)
  if value is not None:
    monkeypatch.setenv('MMT_STEP_GRAPH', value)


def count_reads(monkeypatch):
  """Counts the calls of the loop's one host read."""
  from mmt_amd import train
  calls = []
  real = train.read_loop_results

  def counted(*a, **kw):
    calls.append(1)
    return real(*a, **kw)
  monkeypatch.setattr(train, 'read_loop_results', counted)
  return calls


def loop_lines(logs):
  return [e for e in logs if 'training_loss' in e]


def recovery_lines(logs):
  return [e for e in logs if 'recovered_from' in e]


def f32(v):
  return float(np.float32(v))


def same_number(a, b):
  return (math.isnan(a) and math.isnan(b)) or a == b


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


def event_files(d):
  return sorted(f for f in os.listdir(d) if f.startswith('events.out.tfevents.'))


def assert_events_are_lines(logdir, lines):
  """`logdir` holds exactly the steps of `lines`, every number of a line but `step` under its key, rounded to float32."""
  from mmt_amd import summaries
  got = summaries.read_scalars(logdir)
  tags = [k for k, v in lines[0].items() if k != 'step' and isinstance(v, (int, float))]
  assert list(got) == tags
  for tag in tags:
    assert [s for s, _ in got[tag]] == [e['step'] for e in lines], tag
    for (_, value), e in zip(got[tag], lines):
      assert same_number(value, f32(e[tag])), (tag, e['step'], value, e[tag])


# ---- 1. loop mode does not perturb the run; 6. off means off ----------------------------------------------------------------
@pytest.mark.parametrize('graph', [None, '0'], ids=['recorded', 'eager'])
def test_loop_mode_does_not_perturb_the_run(graph, tmp_path, monkeypatch):
  from mmt_amd import checkpoint, optimization, train
  set_graph(monkeypatch, graph)
  reads = count_reads(monkeypatch)
  exp = experiment(7, steps_per_loop=3, summary_interval=3)
  a_dir, b_dir = str(tmp_path / 'loops'), str(tmp_path / 'plain')
  model_a, logs_a = train.run_experiment(exp, 'train', a_dir, summaries=True)
  assert train.run_experiment.last_step_launch == ('graph' if graph is None else 'eager')
  assert train.run_experiment.last_logs is logs_a
  assert len(reads) == 3                                         # one host read per loop
  model_b, logs_b = train.run_experiment(experiment(7, steps_per_loop=3, summary_interval=3), 'train', b_dir, summaries=None, log_every=1)
  assert len(reads) == 3                                         # ... and none with loop mode off
  # the same weights and optimizer state, bit for bit
  for (n, p), q in zip(model_a.named_parameters(), model_b.parameters()):
    assert torch.equal(p, q), n
  ca, cb = (torch.load(checkpoint.latest_checkpoint(d), map_location='cpu', weights_only=True) for d in (a_dir, b_dir))
  assert ca['step'] == cb['step'] == 7 and ca['optimizer'] is not None
  _same(ca['optimizer'], cb['optimizer'], 'optimizer')
  _same(ca['items'], cb['items'], 'items')
  # the loop lines
  lines = loop_lines(logs_a)
  print(json.dumps(lines))
  assert lines == logs_a and [e['step'] for e in lines] == [3, 6, 7]
  per_step = [e for e in logs_b if 'loss' in e]
  assert [e['step'] for e in per_step] == list(range(7))         # the plain loop counts from 0
  names = [k for k in per_step[0] if k not in ('step', 'loss', 'elapsed_s')]
  assert names                                                   # the task's train metrics
  first = 0
  for line in lines:
    assert list(line) == LINE_HEAD + names
    total, count = np.float32(0), np.float32(0)                  # metrics.Mean: fp32 sums in step order, then one fp32 division
    for e in per_step[first:line['step']]:
      total = np.float32(total + np.float32(e['loss']))
      count = np.float32(count + np.float32(1))
    print('step', line['step'], 'training_loss', line['training_loss'], 'recomputed', float(total / count))
    assert line['training_loss'] == float(np.float32(total / count))
    assert line['learning_rate'] == optimization.learning_rate_at(exp.trainer.optimizer_config, line['step'] - 1)
    assert line['steps_per_second'] > 0 and all(math.isfinite(line[k]) for k in names)
    first = line['step']
  # the last loop is one step long: its metrics are that step's (which the plain loop rounds to 6 decimals)
  for k in names:
    assert abs(lines[-1][k] - per_step[-1][k]) <= 1e-6, k
  # the event file: exactly those three steps
  assert sorted(os.listdir(a_dir)) == ['ckpt-7.pt', 'train'] and len(event_files(os.path.join(a_dir, 'train'))) == 1
  assert_events_are_lines(os.path.join(a_dir, 'train'), lines)
  # off means off
  assert os.listdir(b_dir) == ['ckpt-7.pt']


def test_summary_interval_picks_among_the_loop_ends(tmp_path, monkeypatch):
  """Loops of 2 and summaries every 4 over 7 steps: lines at 2, 4, 6, 7, events at 4 and 7 (the last step)."""
  from mmt_amd import summaries, train
  set_graph(monkeypatch, None)
  reads = count_reads(monkeypatch)
  d = str(tmp_path / 'm')
  _, logs = train.run_experiment(experiment(7, steps_per_loop=2, summary_interval=4), 'train', d, summaries=True)
  assert [e['step'] for e in loop_lines(logs)] == [2, 4, 6, 7] and len(reads) == 4
  assert [s for s, _ in summaries.read_scalars(os.path.join(d, 'train'))['training_loss']] == [4, 7]
  with pytest.raises(ValueError, match='summary_interval'):     # checked before anything is built in model_dir
    train.run_experiment(experiment(7, steps_per_loop=2, summary_interval=5), 'train', str(tmp_path / 'n'), summaries=True)
  assert not os.path.exists(tmp_path / 'n')


# ---- 2. validation summaries --------------------------------------------------------------------------------------------------
def test_validation_summaries(tmp_path, monkeypatch):
  from mmt_amd import summaries, train
  set_graph(monkeypatch, None)
  d = str(tmp_path / 'm')
  _, logs = train.run_experiment(experiment(4, steps_per_loop=2, summary_interval=2), 'train_and_eval', d, summaries=True)
  entries = [e for e in logs if 'validation_loss' in e]
  print(json.dumps(entries))
  assert [e['step'] for e in entries] == [3, 4]                  # the interval, and the last step
  vdir = os.path.join(d, 'validation')
  assert len(event_files(vdir)) == 1
  assert_events_are_lines(vdir, entries)
  assert 'validation_batches' in summaries.read_scalars(vdir)
  assert_events_are_lines(os.path.join(d, 'train'), loop_lines(logs))
  assert [e['step'] for e in loop_lines(logs)] == [2, 4]
  # `eval` mode writes its one evaluation too, into a file of its own; the non-numeric `restored_from` stays out
  _, eval_logs = train.run_experiment(experiment(4), 'eval', d, summaries=True)
  assert len(eval_logs) == 1 and eval_logs[0]['step'] == 4 and eval_logs[0]['restored_from'].endswith('ckpt-4.pt')
  assert len(event_files(vdir)) == 2
  assert_events_are_lines(vdir, entries + [{k: v for k, v in eval_logs[0].items() if k != 'restored_from'}])
  assert {k: v for k, v in eval_logs[0].items() if k != 'restored_from'} == entries[-1]
  assert len(event_files(os.path.join(d, 'train'))) == 1        # `eval` trains nothing and opens no train file


# ---- 3. resume; `validation_summary_subdir` moves the validation events ---------------------------------------------------------
def test_a_resumed_run_adds_a_file_and_the_subdir_key_moves_the_events(tmp_path, monkeypatch):
  from mmt_amd import summaries, train
  set_graph(monkeypatch, None)
  d = str(tmp_path / 'm')
  keys = dict(steps_per_loop=2, summary_interval=2, validation_summary_subdir='ev')
  _, first = train.run_experiment(experiment(4, **keys), 'train_and_eval', d, summaries=True)
  assert len(event_files(os.path.join(d, 'train'))) == 1
  _, second = train.run_experiment(experiment(7, **keys), 'train_and_eval', d, summaries=True)
  assert [e['step'] for e in loop_lines(second)] == [6, 7]       # resumed after step 4: loops are counted from step 1
  tdir = os.path.join(d, 'train')
  assert len(event_files(tdir)) == 2
  got = summaries.read_scalars(tdir)
  assert [s for s, _ in got['training_loss']] == [2, 4, 6, 7]
  assert_events_are_lines(tdir, loop_lines(first) + loop_lines(second))
  assert not os.path.exists(os.path.join(d, 'validation'))
  entries = [e for e in first + second if 'validation_loss' in e]
  assert [e['step'] for e in entries] == [3, 4, 6, 7]
  assert len(event_files(os.path.join(d, 'ev'))) == 2
  assert_events_are_lines(os.path.join(d, 'ev'), entries)


# ---- 4. recovery by the bound, exhausted ------------------------------------------------------------------------------------
def test_recovery_by_the_bound_until_the_trials_run_out(tmp_path, monkeypatch):
  from mmt_amd import train
  set_graph(monkeypatch, None)                                   # steps 1-3 eager, then the recorded step, kept over the restore
  d = str(tmp_path / 'm')
  exp = experiment(6, steps_per_loop=2, checkpoint_interval=2, recovery_begin_steps=4, loss_upper_bound=1e-9, recovery_max_trials=1)
  with pytest.raises(RuntimeError, match='trial 2 of 1') as e:
    train.run_experiment(exp, 'train', d)                        # no `summaries`: recovery alone turns loop mode on
  assert 'step 4' in str(e.value)
  logs = train.run_experiment.last_logs
  print(json.dumps(logs))
  assert train.run_experiment.last_step_launch == 'graph'
  assert [('recovered' if 'recovered_from' in x else 'loop', x['step']) for x in logs] == [
      ('loop', 2), ('loop', 4), ('recovered', 4), ('loop', 4)]
  rec = logs[2]
  assert rec['recovered_from'] == os.path.join(d, 'ckpt-2.pt') and rec['trial'] == 1 and rec['loss'] == logs[1]['training_loss']
  assert all(math.isfinite(x['training_loss']) and x['training_loss'] > 1e-9 for x in loop_lines(logs))
  assert str(logs[3]['training_loss']) in str(e.value)
  assert sorted(os.listdir(d)) == ['ckpt-2.pt']                  # the check comes before the save: no ckpt-4.pt; no event files


def test_recovery_without_a_checkpoint_says_so(tmp_path, monkeypatch):
  from mmt_amd import train
  set_graph(monkeypatch, '0')
  exp = experiment(2, steps_per_loop=1, loss_upper_bound=1e-9, recovery_max_trials=3)
  with pytest.raises(RuntimeError, match='no checkpoint'):
    train.run_experiment(exp, 'train', str(tmp_path / 'm'))
  assert [x['step'] for x in train.run_experiment.last_logs] == [1]


# ---- 5. recovery that succeeds ------------------------------------------------------------------------------------------------
def test_recovery_from_a_nan_step(tmp_path, monkeypatch):
  from mmt_amd import checkpoint, summaries, tasks, train
  set_graph(monkeypatch, '0')
  calls = []
  real = tasks.PretrainingTask.train_step

  def train_step(self, *a, **kw):
    out = real(self, *a, **kw)
    calls.append(kw.get('step'))
    if len(calls) == 5:
      out = dict(out)
      out[self.loss] = torch.full_like(out[self.loss], float('nan'))
    return out
  monkeypatch.setattr(tasks.PretrainingTask, 'train_step', train_step)
  d = str(tmp_path / 'm')
  exp = experiment(6, steps_per_loop=2, summary_interval=2, checkpoint_interval=2, recovery_max_trials=3)
  model, logs = train.run_experiment(exp, 'train', d, summaries=True)
  assert train.run_experiment.last_step_launch == 'eager'
  print(json.dumps(logs))
  assert calls == [1, 2, 3, 4, 5, 6, 5, 6]
  rec = recovery_lines(logs)
  assert len(rec) == 1 and rec[0]['recovered_from'] == os.path.join(d, 'ckpt-4.pt')
  assert rec[0]['step'] == 6 and rec[0]['trial'] == 1 and math.isnan(rec[0]['loss'])
  lines = loop_lines(logs)
  assert [x['step'] for x in lines] == [2, 4, 6, 6]
  assert math.isnan(lines[2]['training_loss']) and all(math.isfinite(lines[i]['training_loss']) for i in (0, 1, 3))
  assert logs.index(rec[0]) == logs.index(lines[2]) + 1
  assert checkpoint.latest_checkpoint(d) == os.path.join(d, 'ckpt-6.pt')
  assert sorted(f for f in os.listdir(d) if f.startswith('ckpt-')) == ['ckpt-2.pt', 'ckpt-4.pt', 'ckpt-6.pt']
  assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
  # the bad loop wrote no summary: the steps of the event file ascend
  assert_events_are_lines(os.path.join(d, 'train'), [lines[0], lines[1], lines[3]])
  assert [s for s, _ in summaries.read_scalars(os.path.join(d, 'train'))['training_loss']] == [2, 4, 6]
