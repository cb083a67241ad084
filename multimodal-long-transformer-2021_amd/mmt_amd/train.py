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
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from . import checkpoint, configs, distribute, evaluation, graphed, optimization, tasks


def run_experiment(params: configs.ExperimentConfig, mode: str, model_dir: str, device=None,
                   log_every: int = 10, max_steps=None):
  """Minimal `train_lib.run_experiment`: build task/model/optimizer under the strategy, loop."""
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

  from . import metrics as metrics_lib
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

  def run_evaluation(step, **note):
    # on the weight averages when the optimizer keeps them (TFM's eval_begin / eval_end: swap_weights round the loop);
    # the exchange is exact and in place, so the recorded steps and the weights after it are what they were
    with optimization.averaged_weights(optimizer):
      eval_logs = evaluation.evaluate(task, model, params.task.validation_data, device=device, rank=strategy.rank,
                                      steps=params.trainer.validation_steps, step_fn=eval_step)
    logs.append({'step': step, **eval_logs, **note})
    if strategy.rank == 0:
      print(json.dumps(logs[-1]), flush=True)
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
    try:
      for step in range(start, steps):
        if graphed_step is not None:
          out = graphed_step(next(data), step + 1)
        else:
          optimization.set_learning_rate(optimizer, optimization.learning_rate_at(opt_cfg, step))
          out = task.train_step(next(data), model, optimizer, metrics=train_metrics, reducer=reducer,
                                clip_norm=opt_cfg.gradient_clip_norm, step=step + 1)
        if step % log_every == 0 or step == steps - 1:
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
    finally:
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
  args = ap.parse_args(argv)
  params = configs.parse_configuration(args.experiment, args.config_file, args.params_override)
  if 'train' in args.mode and args.model_dir:
    os.makedirs(args.model_dir, exist_ok=True)
    with open(os.path.join(args.model_dir, 'params.yaml'), 'w') as f:
      import yaml
      yaml.safe_dump(params.as_dict(), f)
  run_experiment(params, args.mode, args.model_dir, max_steps=args.max_steps)


if __name__ == '__main__':
  main()
