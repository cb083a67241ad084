"""The weight averages on the GPU (`trainer.optimizer_config.ema`; csrc/ema.hip through mmt_amd/optimization.py): the two
kernels against their host mirrors, the flat optimizers' `slab['avg']` against the mirror applied to their own parameter
snapshots, the decay in device memory and replayed from a HIP graph, and the trainer: evaluation on the averages,
checkpoints that carry them, resume and `eval` mode.  Every comparison is bitwise: both sides run the same per-element
functions (csrc/ema.h), and the fused multiply-add is spelt out on both."""
import copy
import ctypes
import os
import re
import shutil

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from tests import _lamb_cases as C
from tests._parity import tiny_experiment

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
  from mmt_amd import _lib
  return _lib


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _host_step(param, avg, omd):
  """mmt_ema_step_host on copies of two device (or host) fp32 tensors: the new averages, a host tensor."""
  lib = _lib()
  p, a = param.detach().cpu().contiguous().numpy(), avg.detach().cpu().contiguous().numpy().copy()
  d = lib.EmaDesc()
  d.n, d.one_minus_decay = p.size, omd
  lib.check(lib.lib().mmt_ema_step_host(d, p.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p)))
  return torch.from_numpy(a)


def _max_blocks():
  src = open(os.path.join(ROOT, 'multimodal-long-transformer-2021_amd', 'csrc', 'ema.h')).read()
  return int(re.search(r'kEmaMaxBlocks = (\d+);', src).group(1))


def _chunk_counts():
  """1 chunk, 3 chunks, and 3 G + 1 chunks with G = kEmaMaxBlocks workgroups, the cap of the grid.  A workgroup b takes
  chunks b and b + G in its first iteration and b + 2G and b + 3G in its second: with 3 G + 1 chunks the first iteration
  is a full pass of all G workgroups over two chunks each, in the second every workgroup still has its first chunk, and
  only workgroup 0 has a second one (chunk 3 G) -- for all others the second chunk of the last iteration is missing."""
  g = _max_blocks()
  assert g == 2048
  return [1, 3, 3 * g + 1]


@pytest.fixture(scope='module')
def slabs():
  """chunks -> (param, avg) device tensors, made once and left unchanged."""
  out = {}
  gen = torch.Generator(device='cuda').manual_seed(7)
  for chunks in _chunk_counts():
    n = chunks * 1024
    param = torch.randn(n, device='cuda', generator=gen)
    avg = param + 0.05 * torch.randn(n, device='cuda', generator=gen)
    out[chunks] = (param, avg)
  return out


# ---------------------------------------------------------------- the kernels against the host mirrors
@pytest.mark.parametrize('chunks', _chunk_counts())
def test_step_kernel_equals_the_host_mirror(slabs, chunks):
  lib = _lib()
  L = lib.lib()
  param, avg0 = slabs[chunks]
  n = param.numel()
  for omd in (float(np.float32(1 - 2 / 11)), float(np.float32(1 - 0.99)), 1.0, 0.0):
    want = _host_step(param, avg0, omd)
    # 1 - decay from the descriptor
    avg = avg0.clone()
    d = lib.EmaDesc()
    d.n, d.one_minus_decay = n, omd
    lib.check(L.mmt_ema_step(d, param.data_ptr(), avg.data_ptr(), _stream()))
    assert torch.equal(avg.cpu(), want), omd
    # ... and from the device word, the descriptor's field poisoned
    avg2, word = avg0.clone(), torch.tensor([omd], dtype=torch.float32, device='cuda')
    d.one_minus_decay, d.one_minus_decay_dev = 7.0, word.data_ptr()
    lib.check(L.mmt_ema_step(d, param.data_ptr(), avg2.data_ptr(), _stream()))
    assert torch.equal(avg2, avg), omd
    if omd == 1.0:
      assert torch.equal(avg, param)
    if omd == 0.0:
      assert torch.equal(avg, avg0)
  assert not torch.equal(_host_step(param, avg0, 0.5), avg0.cpu())


@pytest.mark.parametrize('chunks', _chunk_counts())
def test_swap_kernel(slabs, chunks):
  lib = _lib()
  L = lib.lib()
  p0, a0 = slabs[chunks]
  n = p0.numel()
  param, avg = p0.clone(), a0.clone()
  shadow = torch.empty(n, dtype=torch.bfloat16, device='cuda').copy_(param)
  shadow0 = shadow.clone()
  lib.check(L.mmt_ema_swap(n, param.data_ptr(), avg.data_ptr(), shadow.data_ptr(), _stream()))
  assert torch.equal(param, a0) and torch.equal(avg, p0)                     # the exchange is exact
  assert torch.equal(shadow, param.to(torch.bfloat16))                       # what slab['shadow'].copy_(slab['param']) gives
  assert not torch.equal(shadow, shadow0)
  # the host mirror gives the same three buffers
  hp, ha, hs = p0.cpu().numpy().copy(), a0.cpu().numpy().copy(), np.zeros(n, np.uint16)
  vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
  lib.check(L.mmt_ema_swap_host(n, vp(hp), vp(ha), vp(hs)))
  assert np.array_equal(hp, param.cpu().numpy()) and np.array_equal(ha, avg.cpu().numpy())
  assert np.array_equal(hs, shadow.view(torch.int16).cpu().numpy().view(np.uint16))
  lib.check(L.mmt_ema_swap(n, param.data_ptr(), avg.data_ptr(), shadow.data_ptr(), _stream()))
  assert torch.equal(param, p0) and torch.equal(avg, a0) and torch.equal(shadow, shadow0)      # twice is the identity
  lib.check(L.mmt_ema_swap(n, param.data_ptr(), avg.data_ptr(), None, _stream()))              # NULL shadow is accepted
  assert torch.equal(param, a0) and torch.equal(avg, p0) and torch.equal(shadow, shadow0)


# ---------------------------------------------------------------- the flat optimizers
def _named():
  params, _ = C.inputs()
  return [(n, torch.nn.Parameter(torch.from_numpy(params[n].copy()).cuda())) for n in C.NAMES]


def _run(kind, ema=True, bucket_mb=48.0, given_scales=None, device_scalars=False, check=None):
  """`C.STEPS` steps of FusedAdamW / FusedLamb on the LAMB test model, start_step = 2, the reducer's clip factor (or
  `given_scales`) as grad_scale.  `check(t, opt, omd, before)` runs after every step with the averages as they were
  before it.  Returns the optimizer, the named parameters and the clip factors."""
  from mmt_amd import distribute, optimization, step_scalars
  named = _named()
  reducer = distribute.DataParallelStrategy(None, bucket_mb=bucket_mb).make_reducer([p for _, p in named])
  cfg = C.optimizer_config(optimizer_type=kind, ema_enabled=ema, ema_start_step=2)
  opt = (optimization.FusedLamb if kind == 'lamb' else optimization.FusedAdamW)(named, cfg, reducer)
  _, grads = C.inputs()
  scales = []
  for step in range(C.STEPS):
    reducer.zero_grad()
    for n, p in named:
      p.grad.copy_(torch.from_numpy(grads[step][n].copy()))
    scale = reducer.clip_by_global_norm(C.CLIP, apply=False)
    if given_scales is not None:
      scale = torch.tensor(given_scales[step], dtype=torch.float32, device='cuda')
    scales.append(float(scale))
    before = [s['avg'].clone() for s in opt.slabs] if ema else None
    t = opt.t + 1
    if device_scalars:
      sc = step_scalars.DeviceStepScalars(torch.device('cuda', torch.cuda.current_device()))
      sc.enable()
      right = opt.cfg
      try:
        sc.write(step + 1, C.LR, t, C.BETA_1, C.BETA_2)
        opt.write_ema_scalar(t)
        # the host's own learning rate and decay must not be read: both are wrong from here to the end of the step
        optimization.set_learning_rate(opt, 123.0)
        opt.cfg = copy.copy(right)
        opt.cfg.ema_dynamic_decay, opt.cfg.ema_average_decay, opt.cfg.ema_start_step = False, 0.5, 0
        opt.step(grad_scale=scale)
      finally:
        sc.disable()
        opt.cfg = right
        optimization.set_learning_rate(opt, C.LR)
    else:
      opt.step(grad_scale=scale)
    if check is not None:
      check(t, opt, optimization.ema_one_minus_decay(cfg, t), before)
  return opt, named, scales


def _by_name(opt, named, key):
  names = {p: n for n, p in named}
  return {names[p]: opt.slabs[gi][key][off:off + p.numel()].clone() for p, gi, off in opt.reducer.layout}


@pytest.mark.parametrize('kind', ['adamw', 'lamb'])
def test_flat_optimizers_keep_the_averages(kind):
  from mmt_amd import optimization
  seen = []

  def check(t, opt, omd, before):
    assert omd == [1.0, 1 - 1 / 10, 1 - 2 / 11][t - 1]
    for s, a0 in zip(opt.slabs, before):
      assert torch.equal(s['avg'].cpu(), _host_step(s['param'], a0, omd)), t         # the mirror on the optimizer's own parameters
      if t == 1:
        assert torch.equal(s['avg'], s['param'])                                     # before start_step
      else:
        assert not torch.equal(s['avg'], s['param']) and not torch.equal(s['avg'], a0)
      pad = torch.ones(s['param'].numel(), dtype=torch.bool, device='cuda')
      for p, gi, off in opt.reducer.layout:
        if opt.slabs[gi] is s:
          pad[off:off + p.numel()] = False
      assert int(pad.sum()) > 0 and not bool(s['avg'][pad].any())                    # padding stays exactly zero
    seen.append(t)

  opt, named, scales = _run(kind, check=check)
  assert seen == [1, 2, 3] and opt.ema_enabled and len(opt.slabs) == 1
  assert type(opt) is (optimization.FusedLamb if kind == 'lamb' else optimization.FusedAdamW)
  # parameters, moments and shadows are those of the same run without the averages
  plain, named_p, scales_p = _run(kind, ema=False)
  assert scales_p == scales and not plain.ema_enabled and 'avg' not in plain.slabs[0]
  for key in ('param', 'm', 'v', 'shadow', 'grad'):
    assert torch.equal(opt.slabs[0][key], plain.slabs[0][key]), key
  assert set(opt.state_dict()) == set(plain.state_dict()) == {'t', 'lr', 'slabs'}
  assert all(set(s) == {'m', 'v'} for s in opt.state_dict()['slabs'])
  # several slabs (10 KB buckets) give the same averages as one, handed the same clip factors
  many, named_m, _ = _run(kind, bucket_mb=0.01, given_scales=scales)
  assert len(many.slabs) == 4
  one_avg, many_avg = _by_name(opt, named, 'avg'), _by_name(many, named_m, 'avg')
  for n in C.NAMES:
    assert torch.equal(one_avg[n], many_avg[n]), n
  # swap_weights: exact, the shadows follow, torch's version counters and the shadow versions do not move
  versions = [(p._version, p._mmt_shadow_version) for _, p in named]
  w, a = _by_name(opt, named, 'param'), _by_name(opt, named, 'avg')
  with optimization.averaged_weights(opt) as inside:
    assert inside is opt
    for n, p in named:
      assert torch.equal(p.detach().reshape(-1), a[n]) and torch.equal(p._mmt_shadow, p.detach().to(torch.bfloat16)), n
    assert all(torch.equal(x, w[n]) for n, x in _by_name(opt, named, 'avg').items())
  for n, p in named:
    assert torch.equal(p.detach().reshape(-1), w[n]) and torch.equal(p._mmt_shadow, p.detach().to(torch.bfloat16)), n
  assert [(p._version, p._mmt_shadow_version) for _, p in named] == versions
  plain.swap_weights()                                                               # a no-op without the averages
  assert torch.equal(opt.slabs[0]['param'], plain.slabs[0]['param'])


@pytest.mark.parametrize('kind', ['adamw', 'lamb'])
def test_decay_in_device_memory_equals_the_descriptor(kind):
  opt1, _, _ = _run(kind)
  opt2, _, _ = _run(kind, device_scalars=True)
  for key in ('avg', 'param', 'm', 'v'):
    assert torch.equal(opt1.slabs[0][key], opt2.slabs[0][key]), key


def _tiny_graphed(eager: bool):
  from mmt_amd import distribute, graphed, optimization, tasks
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': 0.1, 'attention_probs_dropout_prob': 0.1}}},
                         'micro_batch_size': 2},
                'trainer': {'optimizer_config': {'initial_learning_rate': 1e-3, 'ema': {'start_step': 3}}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16, num_replicas=1)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt_cfg = exp.trainer.optimizer_config
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  assert isinstance(optimizer, optimization.FusedAdamW) and optimizer.ema_enabled
  batch = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2))
  gs = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, clip_norm=opt_cfg.gradient_clip_norm, eager_steps=1,
                                static_inputs=True)
  if eager:
    gs.eager_left = 1 << 62
  return gs, batch


def test_graphed_step_keeps_the_averages_of_the_eager_loop():
  """Six steps through GraphedTrainStep (one eager, then the recorded graph replayed five times) against six eager steps
  of a twin, start_step = 3: the replays cross it (decay 0 at t = 2, then 1/10, 2/11, 3/12, 4/13 from the device word)
  and end with the eager loop's averages, parameters and losses, bit for bit."""
  res = {}
  for eager in (True, False):
    gs, batch = _tiny_graphed(eager)
    losses, moved = [], []
    for step in range(1, 7):
      losses.append(float(gs(batch, step)['loss']))
      moved.append(not all(torch.equal(s['avg'], s['param']) for s in gs.optimizer.slabs))
    assert (gs.graph is None) == eager and gs.optimizer.t == 6
    assert moved == [False, False, True, True, True, True]
    res[eager] = (losses, *(torch.cat([s[k] for s in gs.optimizer.slabs]).clone() for k in ('avg', 'param', 'm')))
    gs.close()
  assert res[True][0] == res[False][0] and len(set(res[False][0])) > 3
  for a, b in zip(res[True][1:], res[False][1:]):
    assert torch.equal(a, b)


# ---------------------------------------------------------------- the trainer
BATCH = 4
STEPS = 6


def trainer_experiment(train_steps=STEPS, ema=True):
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  oc = {'initial_learning_rate': 1e-3}
  if ema:
    oc['ema'] = {'start_step': 2}
  exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': 0.1, 'attention_probs_dropout_prob': 0.1}}},
                         'train_data': {'global_batch_size': BATCH}, 'micro_batch_size': BATCH},
                'runtime': {'mixed_precision_dtype': 'bfloat16'},
                'trainer': dict(train_steps=train_steps, checkpoint_interval=0, validation_interval=3, validation_steps=3,
                                optimizer_config=oc)})
  exp.task.validation_data = copy.deepcopy(exp.task.train_data)              # synthetic, like the train data
  exp.task.validation_data.is_training = False
  return exp


def _state(opt):
  return {k: torch.cat([s[k] for s in opt.slabs]).clone() for k in ('param', 'm', 'v', 'shadow', 'avg') if k in opt.slabs[0]}


def _spy(mp):
  from mmt_amd import optimization
  made, real = [], optimization.create_optimizer

  def spy(*a, **k):
    made.append(real(*a, **k))
    return made[-1]
  mp.setattr(optimization, 'create_optimizer', spy)
  return made


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
  """`train_and_eval` and `train` with the `ema` block, six steps (three eager, then the recorded step), evaluations after
  steps 3 and 6: per run the directory, the model, the optimizer, the logs and a copy of the optimizer's slabs."""
  from mmt_amd import train
  out = {}
  with pytest.MonkeyPatch.context() as mp:
    mp.delenv('MMT_STEP_GRAPH', raising=False)
    made = _spy(mp)
    for name, mode in (('eval', 'train_and_eval'), ('train', 'train')):
      d = tmp_path_factory.mktemp(name)
      model, logs = train.run_experiment(trainer_experiment(), mode, str(d), log_every=1)
      assert train.run_experiment.last_step_launch == 'graph'
      out[name] = dict(dir=str(d), model=model, opt=made[-1], logs=logs, state=_state(made[-1]))
  return out


def _validation_entries(logs):
  return [e for e in logs if 'validation_loss' in e]


def test_validation_on_the_averages_disturbs_nothing(runs):
  from mmt_amd import checkpoint, optimization
  a, b = runs['eval'], runs['train']
  assert isinstance(a['opt'], optimization.FusedAdamW) and a['opt'].ema_enabled and a['opt'].t == STEPS
  assert set(a['state']) == {'param', 'm', 'v', 'shadow', 'avg'}
  for k in a['state']:
    assert torch.equal(a['state'][k], b['state'][k]), k          # weights, moments, shadows and averages, bit for bit
  assert not torch.equal(a['state']['avg'], a['state']['param'])
  assert [e['step'] for e in _validation_entries(a['logs'])] == [3, 6] and not _validation_entries(b['logs'])
  ca, cb = (torch.load(checkpoint.latest_checkpoint(r['dir']), map_location='cpu', weights_only=True) for r in (a, b))
  assert set(ca) == {'step', 'items', 'optimizer', 'ema_items'} and ca['step'] == STEPS
  for key in ('items', 'ema_items'):
    for item in ca[key]:
      for name, t in ca[key][item].items():
        assert torch.equal(t, cb[key][item][name]), (key, item, name)
  assert any(not torch.equal(t, ca['items'][item][name]) for item in ca['ema_items'] for name, t in ca['ema_items'][item].items())


def test_logged_validation_is_the_evaluation_of_the_averages(runs):
  """The `train` run's own model, evaluated as it stands (the raw weights), then with its masters overwritten with the
  averages by torch copies and the shadows refreshed: the second is what `train_and_eval` logged after its last step."""
  import mmt_amd
  from mmt_amd import evaluation
  a, b = runs['eval'], runs['train']
  exp = trainer_experiment()
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  model, opt = b['model'], b['opt']
  raw = evaluation.evaluate(task, model, exp.task.validation_data, device='cuda', steps=3)
  saved = [s['param'].clone() for s in opt.slabs]
  for s in opt.slabs:
    s['param'].copy_(s['avg'])
  opt.refresh_shadow()
  averaged = evaluation.evaluate(task, model, exp.task.validation_data, device='cuda', steps=3)
  for s, w in zip(opt.slabs, saved):                             # put the weights back: the fixture's objects are shared
    s['param'].copy_(w)
  opt.refresh_shadow()
  logged = {k: v for k, v in _validation_entries(a['logs'])[-1].items() if k != 'step'}
  print('logged', logged, 'raw', raw)
  assert logged == averaged
  assert logged != raw and logged['validation_loss'] != raw['validation_loss']
  assert _state(opt).keys() == b['state'].keys() and all(torch.equal(v, b['state'][k]) for k, v in _state(opt).items())


def test_eval_mode_reports_the_averaged_result(runs, tmp_path):
  from mmt_amd import train
  a = runs['eval']
  model_dir = str(tmp_path / 'copy')
  shutil.copytree(a['dir'], model_dir)
  with pytest.MonkeyPatch.context() as mp:
    made = _spy(mp)
    model, logs = train.run_experiment(trainer_experiment(), 'eval', model_dir, log_every=1)
  final = _validation_entries(a['logs'])[-1]
  assert len(logs) == 1 and {k: v for k, v in logs[0].items() if k != 'restored_from'} == final
  got = _state(made[-1])
  for k in ('param', 'shadow', 'avg'):                           # restored, evaluated on the averages, swapped back
    assert torch.equal(got[k], a['state'][k]), k
  # the same file evaluated without the block: the raw weights, another result
  _, plain = train.run_experiment(trainer_experiment(ema=False), 'eval', model_dir, log_every=1)
  assert plain[0]['validation_loss'] != final['validation_loss']


def test_a_resumed_run_continues_bit_identically(runs, tmp_path):
  """A seventh step of the six-step run's own objects, on the batch a restarted run draws first (the synthetic input
  restarts with the process), against a run resumed from its checkpoint for one more step: weights, moments and
  averages, bit for bit."""
  import mmt_amd
  from mmt_amd import optimization, train
  a = runs['eval']
  exp = trainer_experiment(STEPS + 1)
  opt_cfg = exp.trainer.optimizer_config
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16, num_replicas=1)
  batch = next(task.build_inputs(exp.task.train_data, device=torch.device('cuda', 0), rank=0))
  opt = a['opt']
  optimization.set_learning_rate(opt, optimization.learning_rate_at(opt_cfg, STEPS))
  task.train_step(batch, a['model'], opt, reducer=opt.reducer, clip_norm=opt_cfg.gradient_clip_norm, step=STEPS + 1)
  want = _state(opt)
  model_dir = str(tmp_path / 'resumed')
  shutil.copytree(a['dir'], model_dir)
  with pytest.MonkeyPatch.context() as mp:
    mp.delenv('MMT_STEP_GRAPH', raising=False)
    made = _spy(mp)
    _, logs = train.run_experiment(exp, 'train', model_dir, log_every=1)
  assert [e['step'] for e in logs] == [STEPS] and made[-1].t == STEPS + 1
  got = _state(made[-1])
  for k in want:
    assert torch.equal(got[k], want[k]), k
  assert not torch.equal(want['avg'], a['state']['avg'])
