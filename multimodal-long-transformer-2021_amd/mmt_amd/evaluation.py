"""The validation loop of the trainer: `evaluate` runs `task.validation_step` over `task.validation_data` without
gradients and reads the metrics once at the end; `GraphedEvalStep` records that forward-only step once as a HIP graph
and replays it; `BestCheckpointExporter` keeps the checkpoint with the best value of one reported metric;
`evaluation_due` is the schedule, `loop_end_due` the one of the trainer's loops beside it.  DESIGN.md section 4,
"Validation loop".

The reference gets all of this from TFM's trainer: `trainer.validation_interval` / `validation_steps` drive
`orbit.Controller.evaluate`, the `validation_loss` is a `Mean` over the batches' losses (unweighted per batch), and
`best_checkpoint_export_subdir` / `best_checkpoint_eval_metric` / `best_checkpoint_metric_comp` configure TFM's
`BestCheckpointExporter` (set by every fine-tuning YAML: src/configs/exp_yamls/finetune/*/itm*.yaml).  TFM is a pinned
dependency that is not at hand; the rules here are stated in DESIGN.md and tested as stated."""
from __future__ import annotations

import json
import os
import warnings
from typing import Dict, List, Optional

import torch

from . import checkpoint, prefetch
from . import metrics as metrics_lib

# `graph=None` with MMT_STEP_GRAPH unset.  Eager: at the BASELINE config-3 shape the replayed step's median per batch was
# not below the eager step's in the same run (4.83 against 4.80 ms, tools/eval_timing.py, profiles/eval_timing.json,
# DESIGN.md section 5 "Validation loop: readings") -- the forward is long enough for the host to run ahead of it, and
# the replay adds the copy of the batch into its input buffers.  MMT_STEP_GRAPH=1 turns the recorded step on.
GRAPH_DEFAULT = False

# arrival counters reserved for a recorded step (one word per attention plane, batch x heads: ops.reserve_sync_words)
_SYNC_WORDS = 4096

LOSS_KEY = 'validation_loss'
BATCHES_KEY = 'validation_batches'


def evaluation_due(step: int, interval: int, train_steps: int) -> bool:
  """Is an evaluation due after train step `step` (counted from 1)?  At every positive multiple of `interval` and at
  `train_steps`; with `interval <= 0` at `train_steps` only."""
  step, interval, train_steps = int(step), int(interval), int(train_steps)
  if step == train_steps:
    return True
  return interval > 0 and step > 0 and step % interval == 0


def loop_end_due(step: int, steps_per_loop: int, train_steps: int) -> bool:
  """Does a trainer loop end after train step `step` (counted from 1, steps before a resume included)?  At every
  positive multiple of `steps_per_loop` and at `train_steps`."""
  step, steps_per_loop, train_steps = int(step), int(steps_per_loop), int(train_steps)
  if step == train_steps:
    return True
  return step > 0 and step % steps_per_loop == 0


def check_loop_startup(trainer_cfg) -> None:
  """What a run in loop mode checks before its first train step: `steps_per_loop` and `summary_interval` are at least 1,
  and summaries fall on loop ends (`summary_interval` a multiple of `steps_per_loop`, as orbit requires).  ValueError
  naming both values."""
  per_loop, interval = int(trainer_cfg.steps_per_loop), int(trainer_cfg.summary_interval)
  if per_loop < 1 or interval < 1:
    raise ValueError(f'trainer.steps_per_loop ({per_loop}) and trainer.summary_interval ({interval}) must both be at least 1')
  if interval % per_loop != 0:
    raise ValueError(f'trainer.summary_interval ({interval}) must be a multiple of trainer.steps_per_loop ({per_loop}): '
                     f'summaries are written at loop ends')


def reported_names(task) -> List[str]:
  """The keys `evaluate` returns for this task, `validation_batches` aside: the loss, then one per metric."""
  return [LOSS_KEY] + [f'validation_{name}' for name in metrics_lib.by_name(task.build_metrics(training=False))]


def resolve_metric_key(name: str, task) -> str:
  """`trainer.best_checkpoint_eval_metric` as a key of the evaluation's result: the key itself ('validation_auc',
  'validation_loss') or the bare metric name the reference's YAMLs give ('auc').  ValueError, listing the names, for
  anything the evaluation will not report."""
  names = reported_names(task)
  for key in (name, f'validation_{name}'):
    if key in names:
      return key
  raise ValueError(f'trainer.best_checkpoint_eval_metric is {name!r}, but the evaluation of this task reports {names} '
                   f'(a metric may be named with or without the validation_ prefix)')


def validation_source(task, data_cfg) -> str:
  """'records' | 'synthetic': what `task.build_inputs(data_cfg)` would read, found without a device and without
  reading a record (`task.input_source` is left as it was)."""
  had, before = hasattr(task, 'input_source'), getattr(task, 'input_source', None)
  try:
    task.build_inputs(data_cfg, device='cpu')
    return task.input_source
  finally:
    if had:
      task.input_source = before
    elif hasattr(task, 'input_source'):
      del task.input_source


def _endless(steps: int) -> ValueError:
  return ValueError(f'validation_steps is {steps} (until the data end), but the validation data are the endless synthetic '
                    f'stand-in (no local input_path with a vocab_filename): give a positive trainer.validation_steps')


def check_startup(task, trainer_cfg, data_cfg) -> Optional[str]:
  """What a run that evaluates checks before its first train step, so that a typo does not wait `validation_interval`
  steps to fail: an evaluation until the data end needs data that end, and the best-checkpoint metric must be a name the
  evaluation reports.  Returns that metric's key in the result, or None when no best checkpoint is exported."""
  if int(trainer_cfg.validation_steps) < 0 and validation_source(task, data_cfg) == 'synthetic':
    raise _endless(int(trainer_cfg.validation_steps))
  if not trainer_cfg.best_checkpoint_export_subdir:
    return None
  if trainer_cfg.best_checkpoint_metric_comp not in ('higher', 'lower'):
    raise ValueError(f"trainer.best_checkpoint_metric_comp must be 'higher' or 'lower', got {trainer_cfg.best_checkpoint_metric_comp!r}")
  return resolve_metric_key(trainer_cfg.best_checkpoint_eval_metric, task)


class EvalStep:
  """`step(batch)`: one `task.validation_step` without gradients; the task's metrics and the mean of the batches'
  losses accumulate on the device in `self.metrics` / `self.loss_mean`.  Nothing is read on the host."""

  def __init__(self, task, model, metrics=None):
    self.task, self.model = task, model
    self.metrics = metrics if metrics is not None else task.build_metrics(training=False)
    self.loss_mean = metrics_lib.Mean(LOSS_KEY)

  def all_metrics(self) -> List[metrics_lib.Metric]:
    return [self.loss_mean] + list(metrics_lib.by_name(self.metrics).values())

  def _run(self, batch) -> None:
    out = self.task.validation_step(batch, self.model, metrics=self.metrics)
    self.loss_mean.update_state(out[self.task.loss])             # unweighted per batch, as TFM keeps its validation_loss

  def __call__(self, batch) -> None:
    with torch.no_grad():
      self._run(batch)

  def close(self) -> None:
    pass


def _signature(batch):
  """Keys, tensor shapes / dtypes / devices and non-tensor values of an (inputs, labels) batch."""
  return tuple(tuple((k, (tuple(v.shape), v.dtype, v.device) if torch.is_tensor(v) else v) for k, v in tree.items())
               for tree in batch)


class GraphedEvalStep(EvalStep):
  """The forward-only step recorded once as a HIP graph and replayed (`graphed.GraphedTrainStep` and
  `retrieval.PairScorer._record` are the models).  The first batch runs eagerly: that creates the metric sums and AUC's
  thresholds, whose addresses the recorded launches then name.  The next batch of the same signature is recorded, on a
  stream of the step's own with arrival counters reserved before the capture and held until `close()`; from then on a
  batch that fits is copied into the step's input buffers and replayed, and one that does not (the short last batch)
  runs eagerly, silently -- it is expected.  The graph outlives an evaluation: it reads the parameters where the
  optimizer writes them (fp32 masters and their bf16 shadows, both updated in place), so a replay after further train
  steps sees the weights as they are then; the metric sums are zeroed in place between evaluations.

  `graph`: True / False, or None = the MMT_STEP_GRAPH switch (0 / 1), `GRAPH_DEFAULT` (off: see there) when unset; CUDA
  devices only.  A capture that raises falls back to eager steps with one warning.  Same bits as the eager step
  (tests/test_gpu_evaluation.py)."""

  def __init__(self, task, model, metrics=None, graph: Optional[bool] = None):
    super().__init__(task, model, metrics)
    if graph is None:
      env = os.environ.get('MMT_STEP_GRAPH')
      graph = GRAPH_DEFAULT if env is None else env != '0'
    self.use_graph = bool(graph)
    self.graph = None
    self.sync_words = None
    self.static_batch = None
    self._static_sig = None
    self._eager_sig = None                                       # signature of the last batch that ran eagerly
    self.replays = 0

  @staticmethod
  def _device_of(batch):
    for tree in batch:
      for v in tree.values():
        if torch.is_tensor(v):
          return v.device
    return None

  def _same_signature(self, batch) -> bool:
    """Does `batch` fit the recorded graph's input buffers?  Same keys, same tensor shapes / dtypes / devices, equal
    non-tensor values (`copy_` would broadcast a short last batch over the recorded one)."""
    return _signature(batch) == self._static_sig

  def _sync_shadows(self) -> None:
    """A torch-side write to a master parameter since the last step (a checkpoint restore) re-derives its bf16 shadow
    here, on the host's side of the replay: the recorded launches only read."""
    from . import layers
    for p in self.model.parameters():
      shadow = getattr(p, '_mmt_shadow', None)
      if shadow is not None:
        layers._current_shadow(p, shadow.dtype)

  def _copy_in(self, batch) -> None:
    for src_tree, dst_tree in zip(batch, self.static_batch):
      for k, v in src_tree.items():
        if torch.is_tensor(v) and v.data_ptr() != dst_tree[k].data_ptr():
          dst_tree[k].copy_(v, non_blocking=True)

  def _record(self, batch) -> None:
    from . import ops
    dev = self._device_of(batch)
    self.static_batch = tuple({k: (v.clone() if torch.is_tensor(v) else v) for k, v in tree.items()} for tree in batch)
    self._static_sig = _signature(self.static_batch)
    for m in self.all_metrics():                                 # no sum is allocated inside the capture
      m.ensure(dev)
    self._sync_shadows()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    # the capture stream is this step's own, with arrival counters reserved on it BEFORE the capture (made and zeroed
    # eagerly, held until close()): the recorded attention launches name them, and nothing else ever does
    stream = torch.cuda.Stream(dev)
    self.sync_words = ops.reserve_sync_words(dev, stream, _SYNC_WORDS)
    try:
      with prefetch.capture_gate, torch.cuda.graph(graph, stream=stream):     # (no loader thread allocates or waits inside the capture)
        self._run(self.static_batch)
    finally:
      ops.release_sync_words(dev, stream)
    self.graph = graph

  def _replay(self) -> None:
    self._sync_shadows()
    self.graph.replay()
    self.replays += 1

  def __call__(self, batch) -> None:
    with torch.no_grad():
      if self.graph is not None:
        if self._same_signature(batch):
          self._copy_in(batch)
          self._replay()
        else:
          self._run(batch)
        return
      dev = self._device_of(batch)
      if self.use_graph and dev is not None and dev.type == 'cuda':
        sig = _signature(batch)
        if sig == self._eager_sig:
          try:
            self._record(batch)                                  # recording runs nothing: the batch itself is the first replay
            self._replay()
            return
          except Exception as e:       # something in this configuration cannot be captured: stay eager, say so once
            warnings.warn(f'validation step not recorded as a HIP graph ({type(e).__name__}: {e}); continuing with eager steps')
            self.close()
            self.use_graph = False
            torch.cuda.synchronize(dev)
        self._eager_sig = sig
      self._run(batch)

  def close(self) -> None:
    """Drops the recorded graph, then the arrival counters and input buffers its launches name."""
    self.graph = None
    self.sync_words = None
    self.static_batch = None
    self._static_sig = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass


def make_eval_step(task, model, device, metrics=None, graph: Optional[bool] = None) -> EvalStep:
  """The step the trainer evaluates with: a `GraphedEvalStep` on a CUDA device (which records when `graph` or
  MMT_STEP_GRAPH=1 says so and runs eagerly otherwise), the plain eager step elsewhere."""
  if torch.device(device).type == 'cuda':
    return GraphedEvalStep(task, model, metrics, graph=graph)
  return EvalStep(task, model, metrics)


def _full_device(device) -> torch.device:
  dev = torch.device(device)
  if dev.type == 'cuda' and dev.index is None:
    dev = torch.device('cuda', torch.cuda.current_device())
  return dev


def run_batches(task, step: EvalStep, data_cfg, *, device, rank: int = 0, steps: int = -1, **build_args) -> int:
  """The loop of `evaluate` without the read: a fresh iterator, zeroed sums, up to `steps` batches.  Returns the number
  of batches this rank ran."""
  steps = int(steps)
  data = task.build_inputs(data_cfg, device=device, rank=rank, **build_args)
  if steps < 0 and getattr(task, 'input_source', 'synthetic') == 'synthetic':
    raise _endless(steps)
  for m in step.all_metrics():
    m.reset_state()
  n = 0
  try:
    while steps < 0 or n < steps:
      batch = next(data, None)
      if batch is None:                                          # a finite pass that ends earlier ends the evaluation
        break
      step(batch)
      n += 1
  finally:
    if isinstance(data, prefetch.Prefetcher):                    # an evaluation that stops early leaves no loader reading and decoding
      data.close()
  return n


def read_results(step: EvalStep, device) -> Dict[str, float]:
  """The one read of an evaluation: every metric's sums are made to exist on `device` (a rank that ran no batch still
  takes part in every all-reduce), summed over the replicas, turned into results on the device and copied to the host
  together.  `validation_batches` is the count of the loss mean: the batches of all replicas.  Every rank returns the
  same values."""
  dev = _full_device(device)
  for m in step.all_metrics():
    m.ensure(dev)
  st = step.loss_mean.synced_state()
  named = metrics_lib.by_name(step.metrics)
  values = torch.stack([metrics_lib._divide_no_nan(st[0], st[1]), st[1]] + [m.result().to(torch.float32) for m in named.values()])
  host = values.tolist()
  out = {LOSS_KEY: float(host[0])}
  for name, v in zip(named, host[2:]):
    out[f'validation_{name}'] = float(v)
  out[BATCHES_KEY] = int(round(host[1]))
  return out


def evaluate(task, model, data_cfg, *, device, rank: int = 0, steps: int = -1, metrics=None,
             step_fn: Optional[EvalStep] = None, **build_args) -> Dict[str, float]:
  """One evaluation: `task.validation_step` under `torch.no_grad()` over a FRESH iterator of `data_cfg` (every
  evaluation sees the same batches), up to `steps` batches (`steps < 0`: until the iterator ends; ValueError before any
  batch if the data are the endless synthetic stand-in).  Returns {'validation_loss', 'validation_<metric name>' ...,
  'validation_batches'} as Python floats and an int, read once at the end -- no host read inside the loop.

  `step_fn`: an `EvalStep` that outlives this call (a `GraphedEvalStep` keeps its graph between evaluations); it brings
  its own metrics, zeroed here.  Without one an eager `EvalStep` is made, on `metrics` or on
  `task.build_metrics(training=False)`.  `build_args` go to `task.build_inputs` (`batch_size`, `loader_args`).

  No dropout seed is consumed (the forward runs with training off, which draws none) and `model.training` is not
  touched.  Under data parallelism the ranks may run different numbers of batches, also none: see `read_results`."""
  if step_fn is not None and metrics is not None and metrics is not step_fn.metrics:
    raise ValueError('evaluate: a step_fn brings its own metrics; pass metrics to the step, not beside it')
  step = step_fn if step_fn is not None else EvalStep(task, model, metrics)
  run_batches(task, step, data_cfg, device=device, rank=rank, steps=steps, **build_args)
  return read_results(step, device)


class BestCheckpointExporter:
  """Keeps, in `export_dir`, the one checkpoint whose evaluation had the best `eval_logs[metric_name]` so far
  (`metric_comp`: 'higher' | 'lower'), with `info.json` beside it: {'step', 'metric_name', 'metric_comp',
  'metric_value', 'eval_logs'}.  A new exporter on a directory that has `info.json` continues from its best, so a
  resumed run never replaces a better checkpoint with a worse one.  Every rank takes the same decision, because the
  value it compares is the one summed over the replicas; rank 0 alone writes."""

  def __init__(self, export_dir: str, metric_name: str, metric_comp: str = 'higher', rank: int = 0):
    if metric_comp not in ('higher', 'lower'):
      raise ValueError(f"metric_comp must be 'higher' or 'lower', got {metric_comp!r}")
    self.export_dir, self.metric_name, self.metric_comp, self.rank = export_dir, metric_name, metric_comp, int(rank)
    self.best: Optional[float] = None
    self.best_step: Optional[int] = None
    info = self.info_path
    if os.path.isfile(info):
      with open(info) as f:
        old = json.load(f)
      if old.get('metric_name') == metric_name and old.get('metric_comp') == metric_comp:
        self.best, self.best_step = float(old['metric_value']), int(old['step'])
      else:
        warnings.warn(f'{info} holds the best {old.get("metric_name")!r} ({old.get("metric_comp")}), not {metric_name!r} '
                      f'({metric_comp}): starting over')

  @property
  def info_path(self) -> str:
    return os.path.join(self.export_dir, 'info.json')

  def is_better(self, value: float) -> bool:
    if value != value:                                           # NaN is never a best
      return False
    if self.best is None:
      return True
    return value > self.best if self.metric_comp == 'higher' else value < self.best

  def maybe_export(self, step: int, eval_logs: Dict, model, optimizer=None) -> bool:
    """True when `eval_logs[metric_name]` is strictly better than the best so far (then the checkpoint and `info.json`
    are replaced); a tie or a worse result changes nothing."""
    if self.metric_name not in eval_logs:
      raise KeyError(f'the evaluation reported {sorted(eval_logs)}, not {self.metric_name!r}')
    value = float(eval_logs[self.metric_name])
    if not self.is_better(value):
      return False
    self.best, self.best_step = value, int(step)
    if self.rank == 0:
      checkpoint.save(self.export_dir, int(step), model, optimizer, max_to_keep=1)
      tmp = self.info_path + '.tmp'
      with open(tmp, 'w') as f:
        json.dump({'step': int(step), 'metric_name': self.metric_name, 'metric_comp': self.metric_comp,
                   'metric_value': value, 'eval_logs': dict(eval_logs)}, f, indent=1)
      os.replace(tmp, self.info_path)                            # a crash never leaves a truncated info.json
    return True
