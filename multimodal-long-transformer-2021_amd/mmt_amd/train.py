"""Training driver with the reference's flag surface (`src/train.py:37-91`):
  python -m mmt_amd.train --experiment mmt/pretraining --mode train --model_dir /tmp/m \\
      --config_file a.yaml --params_override task.train_data.max_seq_len=1024
Launch one process per GPU (torchrun / torch.distributed.run).  The pretraining task trains from TFRecord shards when
`task.train_data.input_path` is a local file pattern and `task.train_data.vocab_filename` names a vocabulary file
(`pretrain_dataloader.MmtPretrainDataLoader`); otherwise -- the `gs://` placeholder of the committed YAMLs, an empty
path, the classification task -- data are synthetic (`input_utils.synthetic_batch`).  One log line says which.

Modes: `train` trains; `train_and_eval` / `continuous_train_and_eval` also evaluate `task.validation_data` on the schedule
of `trainer.validation_interval` / `validation_steps` and keep the best checkpoint when `trainer.best_checkpoint_*` say
so; `eval` restores the latest checkpoint of `model_dir` and evaluates once (`mmt_amd/evaluation.py`).  With a
`trainer.optimizer_config.ema` block the optimizer keeps an exponential moving average of the weights, every evaluation
runs on the averages, and the checkpoints carry them (`ema_items`).

Loop mode (on from the command line; `--no_summaries` turns it off): the loss and the train metrics accumulate on the
device and are read once per loop of `trainer.steps_per_loop` steps; rank 0 writes them to `model_dir/train`, and every
evaluation's result to `model_dir/<trainer.validation_summary_subdir>`, as TensorBoard scalars (`mmt_amd/summaries.py`).
With `trainer.recovery_max_trials` a loop whose mean loss is not finite or above `trainer.loss_upper_bound` restores the
latest checkpoint (`Recovery`).  DESIGN.md section 4, "Trainer loop, summaries, recovery".
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time
from typing import Dict, Optional

import torch

from . import checkpoint, configs, distribute, evaluation, graphed, optimization, summaries as summaries_lib, tasks
from . import metrics as metrics_lib

LOOP_LOSS_KEY = 'training_loss'


class Recovery:
  """TFM's recovery rule (restated from memory of `official/core/base_trainer.py`; DESIGN.md section 4 is the contract),
  without device code: `check(step, loss)` at every loop end on the loop's mean loss, the value summed over the replicas,
  so every rank decides alike.  A loss that is not finite, or above `loss_upper_bound` from step `recovery_begin_steps`
  on (a loss equal to the bound is fine), is a bad loop: the trial counter goes up by one, and beyond `max_trials` the
  run ends with a RuntimeError -- `max_trials` 0 fails on the first bad loop."""

  def __init__(self, max_trials: int, begin_steps: int = 0, loss_upper_bound: float = 1e6):
    self.max_trials, self.begin_steps, self.loss_upper_bound = int(max_trials), int(begin_steps), float(loss_upper_bound)
    self.trials = 0

  @classmethod
  def from_config(cls, trainer_cfg) -> Optional['Recovery']:
    if trainer_cfg.recovery_max_trials is None:
      return None
    return cls(trainer_cfg.recovery_max_trials, trainer_cfg.recovery_begin_steps, trainer_cfg.loss_upper_bound)

  def should_recover(self, step: int, loss: float) -> bool:
    if not math.isfinite(loss):
      return True
    return int(step) >= self.begin_steps and loss > self.loss_upper_bound

  def check(self, step: int, loss: float) -> Optional[int]:
    """None for a healthy loop; for a bad one the number of this trial (from 1), or the RuntimeError."""
    if not self.should_recover(step, loss):
      return None
    self.trials += 1
    if self.trials > self.max_trials:
      raise RuntimeError(f'the loop that ended at step {int(step)} has training loss {loss} (not finite, or above '
                         f'loss_upper_bound {self.loss_upper_bound} from step {self.begin_steps} on): this would be '
                         f'recovery trial {self.trials} of {self.max_trials}; giving up')
    return self.trials


def read_loop_results(loss_mean, train_metrics, device) -> Dict[str, float]:
  """THE host read of a loop: the sums of the loss mean and of every train metric, concatenated on the device, summed
  over the replicas in one all-reduce (as `metrics.results` sums each) and copied once; the results are then worked out
  from the host copy.  {'training_loss', <metric name>: ...}, the same values on every rank."""
  dev = evaluation._full_device(device)
  every = [loss_mean] + list(metrics_lib.by_name(train_metrics).values())
  sums = metrics_lib._dist_sum_(torch.cat([m.ensure(dev).state for m in every]))
  host = sums.cpu()
  out, at = {}, 0
  for m in every:
    out[m.name] = float(m.result_of(host[at:at + m.n_state]))
    at += m.n_state
  return out


def _numeric(line: Dict) -> Dict[str, float]:
  """What of a log line becomes a scalar summary: every number but the step."""
  return {k: v for k, v in line.items() if k != 'step' and isinstance(v, (int, float)) and not isinstance(v, bool)}


def run_experiment(params: configs.ExperimentConfig, mode: str, model_dir: str, device=None,
                   log_every: int = 10, max_steps=None, summaries: Optional[bool] = None):
  """Minimal `train_lib.run_experiment`: build task/model/optimizer under the strategy, loop.

  Loop mode is on when `summaries` is true or `trainer.recovery_max_trials` is set.  Then `log_every` is ignored: the
  host reads once per loop of `trainer.steps_per_loop` steps (`read_loop_results`) and logs {'step', 'training_loss',
  'learning_rate', 'steps_per_second', <train metrics>}, `step` being the count of steps done; with `summaries` rank 0
  also writes the event files.  Off (`None` / `False`, the default), the loop logs by `log_every` as it always did."""
  rt = params.runtime
  strategy = distribute.get_distribution_strategy(
      distribution_strategy=rt.distribution_strategy, all_reduce_alg=rt.all_reduce_alg,
      num_gpus=rt.num_gpus, tpu_address=rt.tpu)
  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  device = device or torch.device('cuda', local_rank)
  torch.cuda.set_device(device)
  task = tasks.get_task(params.task, logging_dir=model_dir,
                        compute_dtype=tasks._compute_dtype(rt.mixed_precision_dtype),
                        num_replicas=strategy.num_replicas_in_sync)
  torch.manual_seed(0)     # identical initial weights on every replica
  model = task.build_model().to(device)
  task.initialize(model)              # warm start from task.init_checkpoint (no-op when empty)
  opt_cfg = params.trainer.optimizer_config
  reducer = strategy.make_reducer(list(model.parameters()), reduce=tasks.gradient_reduce_mode(params.task))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  data = task.build_inputs(params.task.train_data, device=device, rank=strategy.rank)
  train_prefetch = getattr(task, 'input_prefetch', None)      # (an evaluation's build_inputs sets the attribute again)
  if strategy.rank == 0:
    print(json.dumps({'input_source': getattr(task, 'input_source', 'synthetic'),
                      'input_prefetch': train_prefetch.depth if train_prefetch is not None else 0,
                      'input_path': params.task.train_data.input_path if getattr(task, 'input_source', '') == 'records' else ''}), flush=True)
  steps = max_steps or params.trainer.train_steps
  logs = []
  run_experiment.last_logs = logs       # also readable when the run ends in an exception
  recovery = Recovery.from_config(params.trainer)
  loop_mode = bool(summaries) or recovery is not None
  if loop_mode and 'train' in mode:
    evaluation.check_loop_startup(params.trainer)               # before the first train step, like check_startup below
  start = 0
  resume_from = checkpoint.latest_checkpoint(model_dir) if model_dir and os.path.isdir(model_dir) else None
  if resume_from:                       # restart: model, optimizer moments and step from the latest checkpoint
    start = checkpoint.restore(resume_from, model, optimizer)
    if hasattr(optimizer, 'refresh_shadow'):
      optimizer.refresh_shadow()
    if strategy.rank == 0:
      print(json.dumps({'resumed_from': resume_from, 'step': start}), flush=True)
  ckpt_every = params.trainer.checkpoint_interval

  def save(step):
    if strategy.rank == 0 and model_dir:
      checkpoint.save(model_dir, step, model, optimizer, max_to_keep=params.trainer.max_to_keep)

  # the validation loop (evaluation.py): `train` mode runs none; `train_and_eval` / `continuous_train_and_eval` evaluate
  # task.validation_data after every train step that `evaluation_due` names; `eval` evaluates once and trains nothing
  evaluates = 'eval' in mode
  eval_step = exporter = None
  if evaluates:
    best_key = evaluation.check_startup(task, params.trainer, params.task.validation_data)     # before the first train step
    if best_key and model_dir:
      exporter = evaluation.BestCheckpointExporter(
          os.path.join(model_dir, params.trainer.best_checkpoint_export_subdir), best_key,
          params.trainer.best_checkpoint_metric_comp, rank=strategy.rank)
    eval_step = evaluation.make_eval_step(task, model, device)
  writers = {}                          # 'train' / 'validation' -> summaries.EventFileWriter, on rank 0 with `summaries`

  def open_writer(name, subdir):
    if summaries and strategy.rank == 0 and model_dir:
      writers[name] = summaries_lib.EventFileWriter(os.path.join(model_dir, subdir))

  def close_writers():
    for w in writers.values():
      w.close()

  if evaluates:
    open_writer('validation', params.trainer.validation_summary_subdir)

  def run_evaluation(step, **note):
    # on the weight averages when the optimizer keeps them (TFM's eval_begin / eval_end: swap_weights round the loop);
    # the exchange is exact and in place, so the recorded steps and the weights after it are what they were
    with optimization.averaged_weights(optimizer):
      eval_logs = evaluation.evaluate(task, model, params.task.validation_data, device=device, rank=strategy.rank,
                                      steps=params.trainer.validation_steps, step_fn=eval_step)
    logs.append({'step': step, **eval_logs, **note})
    if strategy.rank == 0:
      print(json.dumps(logs[-1]), flush=True)
    if 'validation' in writers:
      writers['validation'].scalars(step, _numeric(logs[-1]))
      writers['validation'].flush()
    if exporter is not None and 'train' in mode:
      exporter.maybe_export(step, eval_logs, model, optimizer)

  if 'train' in mode:
    t0 = time.perf_counter()
    # `task.build_metrics()` objects, updated on the device inside every step (process_metrics, pretraining.py:297);
    # read -- one all-reduce + one host copy each -- only on logging steps, then reset like orbit's summary loop
    train_metrics = task.build_metrics(training=True)
    # the step as a HIP graph (recorded after three eager steps, graphed.py) when everything it touches has a fixed
    # address: flat optimizer on the GPU, bf16 compute.  MMT_STEP_GRAPH: unset = on with one replica, 0 / 1 = off / on
    graphed_step = None
    env = os.environ.get('MMT_STEP_GRAPH')
    if ((strategy.num_replicas_in_sync == 1 if env is None else env != '0') and hasattr(optimizer, 'slabs')
        and task.compute_dtype == torch.bfloat16):
      graphed_step = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, metrics=train_metrics,
                                              clip_norm=opt_cfg.gradient_clip_norm)
    run_experiment.last_step_launch = 'graph' if graphed_step is not None else 'eager'
    loss_mean = metrics_lib.Mean(LOOP_LOSS_KEY)
    per_loop, summary_every = params.trainer.steps_per_loop, params.trainer.summary_interval
    loop_t0, loop_begin = time.perf_counter(), start

    def end_loop(done):
      """The end of the loop that train step `done` (from 1) closes: the read, the line, the recovery check, the
      summaries.  Returns (the step to go on from, recovered?): `done`, or the step of the checkpoint a recovery restored."""
      nonlocal loop_t0, loop_begin
      read = read_loop_results(loss_mean, train_metrics, device)
      metrics_lib.reset(train_metrics)
      loss_mean.reset_state()
      now = time.perf_counter()
      line = {'step': done, LOOP_LOSS_KEY: read.pop(LOOP_LOSS_KEY),
              'learning_rate': optimization.learning_rate_at(opt_cfg, done - 1),
              'steps_per_second': (done - loop_begin) / max(now - loop_t0, 1e-9), **read}
      logs.append(line)
      if strategy.rank == 0:
        print(json.dumps(line), flush=True)
      trial = recovery.check(done, line[LOOP_LOSS_KEY]) if recovery is not None else None
      if trial is not None:             # before a checkpoint due at this step is written; the bad loop gets no summary
        path = checkpoint.latest_checkpoint(model_dir) if model_dir and os.path.isdir(model_dir) else None
        if path is None:
          raise RuntimeError(f'the loop that ended at step {done} has training loss {line[LOOP_LOSS_KEY]} and there is '
                             f'no checkpoint in {model_dir!r} to recover from')
        done = checkpoint.restore(path, model, optimizer)
        if hasattr(optimizer, 'refresh_shadow'):
          optimizer.refresh_shadow()
        logs.append({'recovered_from': path, 'step': line['step'], 'loss': line[LOOP_LOSS_KEY], 'trial': trial})
        if strategy.rank == 0:
          print(json.dumps(logs[-1]), flush=True)
      elif 'train' in writers and (done % summary_every == 0 or done == steps):
        writers['train'].scalars(done, _numeric(line))
        writers['train'].flush()
      loop_t0, loop_begin = time.perf_counter(), done
      return done, trial is not None

    try:
      if loop_mode:
        open_writer('train', 'train')
      step = start
      while step < steps:
        if graphed_step is not None:
          out = graphed_step(next(data), step + 1)
        else:
          optimization.set_learning_rate(optimizer, optimization.learning_rate_at(opt_cfg, step))
          out = task.train_step(next(data), model, optimizer, metrics=train_metrics, reducer=reducer,
                                clip_norm=opt_cfg.gradient_clip_norm, step=step + 1)
        if loop_mode:                    # nothing is read on the host inside a loop
          loss_mean.update_state(out[task.loss])
          if evaluation.loop_end_due(step + 1, per_loop, steps):
            done, recovered = end_loop(step + 1)
            if recovered:                # on from the restored checkpoint's step, with the data iterator where it is
              step = done
              continue
        elif step % log_every == 0 or step == steps - 1:
          loss = float(out[task.loss])
          logs.append({'step': step, 'loss': loss, 'elapsed_s': time.perf_counter() - t0,
                       **{k: round(v, 6) for k, v in metrics_lib.results(train_metrics).items()}})
          metrics_lib.reset(train_metrics)
          if strategy.rank == 0:
            print(json.dumps(logs[-1]), flush=True)
        if ckpt_every and (step + 1) % ckpt_every == 0 and step + 1 < steps:
          save(step + 1)
        if step + 1 == steps:
          save(steps)                  # before the last evaluation: what `eval` mode restores is what was evaluated
        if evaluates and evaluation.evaluation_due(step + 1, params.trainer.validation_interval, steps):
          run_evaluation(step + 1)
        step += 1
    except BaseException:
      close_writers()
      raise
    finally:
      if 'train' in writers:
        writers.pop('train').close()
      if graphed_step is not None:       # also when the loop raised: the device-resident step scalars must not outlive it
        graphed_step.close()
      if train_prefetch is not None:     # the loader's worker thread ends with the loop
        train_prefetch.close()
    if evaluates and start >= steps:     # a resumed run with nothing left to train still reports where it stands
      run_evaluation(start)
  elif evaluates:                        # `eval`: the restored weights (the JSON line says from where; null = none found)
    run_evaluation(start, restored_from=resume_from)
  if eval_step is not None:
    eval_step.close()
  if train_prefetch is not None:         # (`eval` mode: built, never read)
    train_prefetch.close()
  close_writers()
  return model, logs


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument('--experiment', required=True)
  ap.add_argument('--mode', required=True,
                  choices=['train', 'eval', 'train_and_eval', 'continuous_train_and_eval'])
  ap.add_argument('--model_dir', required=True)
  ap.add_argument('--config_file', action='append', default=[])
  ap.add_argument('--params_override', default=None)
  ap.add_argument('--tpu', default=None)
  ap.add_argument('--tpu_zone', default=None)
  ap.add_argument('--pretrain_steps', type=int, default=None)
  ap.add_argument('--max_steps', type=int, default=None)
  ap.add_argument('--no_summaries', action='store_true',
                  help='log by log_every instead of trainer.steps_per_loop and write no TensorBoard event files')
  args = ap.parse_args(argv)
  params = configs.parse_configuration(args.experiment, args.config_file, args.params_override)
  if 'train' in args.mode and args.model_dir:
    os.makedirs(args.model_dir, exist_ok=True)
    with open(os.path.join(args.model_dir, 'params.yaml'), 'w') as f:
      import yaml
      yaml.safe_dump(params.as_dict(), f)
  run_experiment(params, args.mode, args.model_dir, max_steps=args.max_steps, summaries=not args.no_summaries)


if __name__ == '__main__':
  main()
