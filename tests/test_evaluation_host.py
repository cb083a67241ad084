"""Host logic of the validation loop (mmt_amd/evaluation.py): the schedule, the best-checkpoint exporter, the checks a
run makes before its first train step, the loop of `evaluate` on a stand-in task with CPU tensors, and the read of the
metrics by two gloo ranks of which one ran no batch."""
import json
import os
import socket
import time

import pytest
import torch

import __graft_entry__  # noqa: F401
from tests._parity import tiny_experiment


# ---- evaluation_due ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step, interval, train_steps, want', [
    (1, 2, 10, False), (2, 2, 10, True), (3, 2, 10, False), (10, 2, 10, True),          # every multiple, and the end
    (2000, 2000, 10000, True), (4000, 2000, 10000, True), (1999, 2000, 10000, False),
    (6, 4, 6, True), (4, 4, 6, True), (5, 4, 6, False), (8, 4, 6, True),                  # train_steps no multiple of the interval
    (5, 0, 5, True), (4, 0, 5, False), (5, -1, 5, True), (3, -1, 5, False), (0, 0, 5, False),     # interval <= 0: the end only
    (0, 2, 10, False),                                                                     # no evaluation before the first step
    (7, 3, 9, False), (9, 3, 9, True),
])
def test_evaluation_due_table(step, interval, train_steps, want):
  from mmt_amd.evaluation import evaluation_due
  assert evaluation_due(step, interval, train_steps) is want


def test_evaluation_due_of_a_resumed_run():
  """A run resumed after step 5 of 12 with interval 4 evaluates at 8 and 12, like the run that was never interrupted."""
  from mmt_amd.evaluation import evaluation_due
  whole = [s for s in range(1, 13) if evaluation_due(s, 4, 12)]
  resumed = [s for s in range(5 + 1, 13) if evaluation_due(s, 4, 12)]
  assert whole == [4, 8, 12] and resumed == [8, 12]


# ---- BestCheckpointExporter ---------------------------------------------------------------------------------------------
def _stub():
  torch.manual_seed(0)
  model = torch.nn.Linear(3, 2)
  return model, torch.optim.SGD(model.parameters(), lr=0.1)


def _files(d):
  return sorted(os.listdir(d))


@pytest.mark.parametrize('comp, values, kept', [('higher', [0.5, 0.7, 0.6, 0.7, 0.9], [1, 2, 5]),
                                                 ('lower', [0.5, 0.7, 0.4, 0.4, 0.1], [1, 3, 5])])
def test_exporter_keeps_the_strictly_better_result(tmp_path, comp, values, kept):
  from mmt_amd import checkpoint
  from mmt_amd.evaluation import BestCheckpointExporter
  model, opt = _stub()
  d = str(tmp_path / 'best_ckpt')
  ex = BestCheckpointExporter(d, 'validation_auc', comp)
  for step, v in enumerate(values, start=1):
    with torch.no_grad():
      model.weight.fill_(float(step))                            # the saved weights say which step was kept
    logs = {'validation_loss': 1.0 / step, 'validation_auc': v, 'validation_batches': 3}
    before = (_files(d), open(os.path.join(d, 'info.json')).read()) if os.path.isdir(d) else None
    exported = ex.maybe_export(step, logs, model, opt)
    assert exported is (step in kept), (step, v)
    if not exported:                                             # a tie or a worse result changes nothing
      assert (_files(d), open(os.path.join(d, 'info.json')).read()) == before
      continue
    assert _files(d) == [f'ckpt-{step}.pt', 'info.json']         # exactly one checkpoint, no temporary file left
    info = json.load(open(os.path.join(d, 'info.json')))
    assert info == {'step': step, 'metric_name': 'validation_auc', 'metric_comp': comp, 'metric_value': v, 'eval_logs': logs}
    fresh, _ = _stub()
    assert checkpoint.restore(os.path.join(d, f'ckpt-{step}.pt'), fresh) == step
    assert float(fresh.weight[0, 0]) == float(step)
  assert ex.best == values[kept[-1] - 1] and ex.best_step == kept[-1]


def test_exporter_continues_from_an_existing_directory(tmp_path):
  from mmt_amd.evaluation import BestCheckpointExporter
  model, opt = _stub()
  d = str(tmp_path / 'best_ckpt')
  first = BestCheckpointExporter(d, 'validation_loss', 'lower')
  assert first.maybe_export(4, {'validation_loss': 0.25}, model, opt)
  resumed = BestCheckpointExporter(d, 'validation_loss', 'lower')
  assert resumed.best == 0.25 and resumed.best_step == 4
  assert not resumed.maybe_export(6, {'validation_loss': 0.5}, model, opt)      # worse: the better checkpoint stays
  assert not resumed.maybe_export(7, {'validation_loss': 0.25}, model, opt)     # a tie too
  assert _files(d) == ['ckpt-4.pt', 'info.json'] and json.load(open(os.path.join(d, 'info.json')))['step'] == 4
  assert resumed.maybe_export(8, {'validation_loss': 0.125}, model, opt)
  assert _files(d) == ['ckpt-8.pt', 'info.json'] and json.load(open(os.path.join(d, 'info.json')))['metric_value'] == 0.125
  with pytest.warns(UserWarning, match='starting over'):                        # the best of another metric is not comparable
    other = BestCheckpointExporter(d, 'validation_auc', 'higher')
  assert other.best is None


def test_exporter_refusals_nan_and_the_ranks(tmp_path):
  from mmt_amd.evaluation import BestCheckpointExporter
  model, opt = _stub()
  with pytest.raises(ValueError, match="'higher' or 'lower'"):
    BestCheckpointExporter(str(tmp_path / 'x'), 'validation_loss', 'highest')
  ex = BestCheckpointExporter(str(tmp_path / 'nan'), 'validation_loss', 'lower')
  assert not ex.maybe_export(1, {'validation_loss': float('nan')}, model, opt) and not os.path.exists(tmp_path / 'nan')
  with pytest.raises(KeyError, match='validation_auc'):
    BestCheckpointExporter(str(tmp_path / 'y'), 'validation_auc', 'higher').maybe_export(1, {'validation_loss': 1.0}, model, opt)
  # every rank takes the decision, rank 0 alone writes
  r1 = BestCheckpointExporter(str(tmp_path / 'rank1'), 'validation_loss', 'lower', rank=1)
  assert r1.maybe_export(1, {'validation_loss': 1.0}, model, opt) and not r1.maybe_export(2, {'validation_loss': 2.0}, model, opt)
  assert r1.best == 1.0 and not os.path.exists(tmp_path / 'rank1')


# ---- the checks before the first train step --------------------------------------------------------------------------------
def _tasks():
  import mmt_amd
  from mmt_amd import configs
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp = configs.get_exp_config('mmt/classification')
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(), 'num_classes': 2,
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': exp.task.train_data.as_dict()}}, strict=False)
  return (exp, mmt_amd.tasks.get_task(exp.task)), (cexp, mmt_amd.tasks.get_task(cexp.task))


def test_startup_refuses_an_evaluation_without_end_on_endless_data(tmp_path):
  import copy
  from mmt_amd import evaluation
  from tests import _record_cases as R
  (exp, task), _ = _tasks()
  v = copy.deepcopy(exp.task.train_data)
  v.is_training = False
  exp.trainer.validation_steps = -1
  had = hasattr(task, 'input_source')
  with pytest.raises(ValueError, match='endless synthetic'):
    evaluation.check_startup(task, exp.trainer, v)
  assert hasattr(task, 'input_source') == had                    # the probe leaves the task as it was
  exp.trainer.validation_steps = 3
  assert evaluation.check_startup(task, exp.trainer, v) is None   # a count of batches is fine on any data
  # records end: the same configuration with shards and a vocabulary passes with validation_steps = -1
  R.write_shards(tmp_path, R.loader_records(4), 1)
  v.input_path, v.vocab_filename = str(tmp_path / '*.tfrecord'), R.write_vocab(tmp_path / 'vocab.txt')
  v.text_special_token_field_dict = json.dumps(R.FIELD_DICT)
  exp.trainer.validation_steps = -1
  assert evaluation.validation_source(task, v) == 'records'
  assert evaluation.check_startup(task, exp.trainer, v) is None


def test_startup_refuses_a_best_checkpoint_metric_nobody_reports():
  from mmt_amd import evaluation
  (exp, task), (cexp, ctask) = _tasks()
  assert evaluation.reported_names(task) == ['validation_loss', 'validation_mlm_accuracy', 'validation_mlm_loss',
                                             'validation_mpp_accuracy', 'validation_mpp_loss', 'validation_itm_accuracy',
                                             'validation_itm_loss']
  assert evaluation.reported_names(ctask) == ['validation_loss', 'validation_cls_accuracy', 'validation_auc',
                                              'validation_classification_loss']
  for e in (exp, cexp):
    e.trainer.validation_steps = 2
    e.trainer.best_checkpoint_export_subdir = 'best_ckpt'
  cexp.trainer.best_checkpoint_eval_metric = 'auc'               # as every fine-tuning YAML of the reference spells it
  assert evaluation.check_startup(ctask, cexp.trainer, cexp.task.validation_data) == 'validation_auc'
  cexp.trainer.best_checkpoint_eval_metric = 'validation_loss'
  assert evaluation.check_startup(ctask, cexp.trainer, cexp.task.validation_data) == 'validation_loss'
  exp.trainer.best_checkpoint_eval_metric = 'auc'                # the pretraining task has no such metric
  with pytest.raises(ValueError, match=r"'auc'.*validation_mlm_accuracy"):
    evaluation.check_startup(task, exp.trainer, exp.task.validation_data)
  cexp.trainer.best_checkpoint_eval_metric = 'acu'               # the typo that must not wait 2000 steps
  with pytest.raises(ValueError, match=r"'acu'.*validation_auc"):
    evaluation.check_startup(ctask, cexp.trainer, cexp.task.validation_data)
  cexp.trainer.best_checkpoint_eval_metric, cexp.trainer.best_checkpoint_metric_comp = 'auc', 'max'
  with pytest.raises(ValueError, match="'higher' or 'lower'"):
    evaluation.check_startup(ctask, cexp.trainer, cexp.task.validation_data)
  cexp.trainer.best_checkpoint_export_subdir = ''                # nothing exported: nothing to check
  assert evaluation.check_startup(ctask, cexp.trainer, cexp.task.validation_data) is None


# ---- the loop, on a stand-in task ----------------------------------------------------------------------------------------
class _Task:
  """Batches of a finite list (or without end), a loss that depends on the model's weight, two metrics."""
  loss = 'loss'

  def __init__(self, sizes, endless=False):
    self.sizes, self.endless = sizes, endless
    self.built = 0

  def build_inputs(self, data_cfg, device='cpu', rank=0, **kw):
    self.built += 1
    self.input_source = 'synthetic' if self.endless else 'records'
    def it():
      k = 0
      while True:
        for n in self.sizes:
          k += 1
          yield {'x': torch.arange(n, dtype=torch.float32, device=device) + k}, {'y': torch.ones(n, device=device)}
        if not self.endless:
          return
    return it()

  def build_metrics(self, training=None):
    from mmt_amd import metrics as M
    return [M.Mean('x_mean'), M.AUC('auc')]

  def validation_step(self, batch, model, metrics=None):
    from mmt_amd import metrics as M
    assert not torch.is_grad_enabled()
    inputs, labels = batch
    M.by_name(metrics)['x_mean'].update_state(inputs['x'], labels['y'])
    return {'loss': (model.weight.sum() * inputs['x']).mean()}


def test_evaluate_loop_on_cpu_tensors(monkeypatch):
  from mmt_amd import evaluation, fused, step_scalars
  model = torch.nn.Linear(1, 1, bias=False)
  with torch.no_grad():
    model.weight.fill_(2.0)
  model.train()
  task = _Task([4, 4, 2])
  for name in ('next_seed', 'set_seed_stream'):                  # an evaluation draws no dropout seed
    monkeypatch.setattr(fused, name, lambda *a, **k: pytest.fail(f'fused.{name} called'))
  monkeypatch.setattr(step_scalars, 'set_step', lambda *a, **k: pytest.fail('step_scalars.set_step called'))
  got = evaluation.evaluate(task, model, None, device='cpu', rank=0, steps=-1)
  # batches k = 1, 2, 3: x = arange(n) + k; the loss of a batch is 2 * mean(x), the validation loss their unweighted mean
  means = [1.5 + 1, 1.5 + 2, 0.5 + 3]
  f32 = lambda num, den: float(torch.tensor(float(num)) / torch.tensor(float(den)))         # the sums and the quotient are fp32
  assert got == {'validation_loss': f32(2 * sum(means), 3), 'validation_x_mean': f32(4 * means[0] + 4 * means[1] + 2 * means[2], 10),
                 'validation_auc': 0.0, 'validation_batches': 3}
  assert all(type(got[k]) is float for k in got if k != 'validation_batches') and type(got['validation_batches']) is int
  assert model.training                                          # left as it was found
  assert evaluation.evaluate(task, model, None, device='cpu', steps=-1) == got        # a fresh iterator: the same batches
  assert task.built == 2
  two = evaluation.evaluate(task, model, None, device='cpu', steps=2)
  assert two['validation_batches'] == 2 and two['validation_loss'] == 2 * (means[0] + means[1]) / 2
  assert evaluation.evaluate(task, model, None, device='cpu', steps=7)['validation_batches'] == 3      # the pass ends first
  # a step that outlives the call keeps its metrics; they start from zero every time; on CPU tensors it never records
  step = evaluation.GraphedEvalStep(task, model, graph=True)
  for _ in range(2):
    assert evaluation.evaluate(task, model, None, device='cpu', steps=-1, step_fn=step) == got
  assert step.graph is None and step.replays == 0
  with pytest.raises(ValueError, match='brings its own metrics'):
    evaluation.evaluate(task, model, None, device='cpu', steps=1, step_fn=step, metrics=task.build_metrics())
  assert isinstance(evaluation.make_eval_step(task, model, 'cpu'), evaluation.EvalStep)
  # endless data: a count is fine, "until the end" is refused before any batch runs
  endless = _Task([4], endless=True)
  assert evaluation.evaluate(endless, model, None, device='cpu', steps=3)['validation_batches'] == 3
  ran = []
  probe = evaluation.EvalStep(endless, model)
  probe._run = lambda batch: ran.append(1)
  with pytest.raises(ValueError, match='endless synthetic'):
    evaluation.evaluate(endless, model, None, device='cpu', steps=-1, step_fn=probe)
  assert not ran


def test_metric_ensure():
  from mmt_amd import metrics as M
  m = M.Mean('m')
  assert m.state is None and m.ensure('cpu') is m and m.state.tolist() == [0.0, 0.0]
  m.update_state(torch.tensor([1.0, 3.0]))
  assert m.ensure('cpu').state.tolist() == [4.0, 2.0]            # sums that exist are kept
  a = M.AUC('auc').ensure('cpu')
  assert tuple(a.state.shape) == (800,) and float(a.result()) == 0.0


# ---- two ranks, one of them without a batch --------------------------------------------------------------------------------
def _free_port():
  s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_worker(rank, world, port, out):
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from mmt_amd import evaluation
  model = torch.nn.Linear(1, 1, bias=False)
  with torch.no_grad():
    model.weight.fill_(2.0)
  task = _Task([4, 2] if rank == 0 else [])                      # rank 1 runs no batch: none of its sums exists before the read
  out[rank] = evaluation.evaluate(task, model, None, device='cpu', rank=rank, steps=-1)
  dist.destroy_process_group()


def test_a_rank_without_batches_takes_part_in_the_read():
  """Without `Metric.ensure` rank 1's never-updated metrics would skip their all-reduce and rank 0 would wait for ever;
  the children run under a time limit of their own."""
  import torch.multiprocessing as mp
  world = 2
  with mp.Manager() as mgr:
    out = mgr.dict()
    ctx = mp.spawn(_rank_worker, args=(world, _free_port(), out), nprocs=world, join=False)
    deadline = time.monotonic() + 120
    while not ctx.join(timeout=1):
      if time.monotonic() > deadline:
        for p in ctx.processes:
          p.kill()
        pytest.fail('the ranks did not finish: a rank is waiting in an all-reduce the other one skipped')
    r0, r1 = out[0], out[1]
  assert r0 == r1
  assert r0 == {'validation_loss': 2 * (2.5 + 2.5) / 2, 'validation_x_mean': (4 * 2.5 + 2 * 2.5) / 6, 'validation_auc': 0.0,
                'validation_batches': 2}
