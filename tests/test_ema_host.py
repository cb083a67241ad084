"""The weight averages without a GPU (`trainer.optimizer_config.ema`: mmt_amd/configs.py, mmt_amd/optimization.py
`ema_decay_at` / `WeightAverages` / `averaged_weights`, mmt_amd/checkpoint.py `ema_items`, the task key
`init_checkpoint_averages`; csrc/ema.hip `mmt_ema_step_host` / `mmt_ema_swap_host`, the kernels' per-element functions
as plain loops): the decay rule by hand, configuration parsing, the host mirror against a numpy oracle, the plain-torch
averages against the recurrence on parameter snapshots, and the checkpoint layouts."""
import ctypes
import dataclasses
import os
import warnings

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from mmt_amd import checkpoint, configs, optimization
from tests._parity import tiny_experiment

EMA_YAML = """
trainer:
  optimizer_config:
    optimizer:
      type: adamw
      adamw:
        weight_decay_rate: 0.05
    ema:
      average_decay: 0.98
      start_step: 7
      dynamic_decay: false
      trainable_weights_only: true
"""


def _cfg(**kw):
  return configs.OptimizerConfig(ema_enabled=True, **kw)


# ---------------------------------------------------------------- the decay rule
def test_decay_by_hand():
  c = _cfg()                                               # TFM's defaults: 0.99, start 0, dynamic
  assert (c.ema_average_decay, c.ema_start_step, c.ema_dynamic_decay, c.ema_trainable_weights_only) == (0.99, 0, True, True)
  for t, want in ((1, 2 / 11), (2, 3 / 12), (81, 82 / 91), (82, 83 / 92)):
    assert optimization.ema_decay_at(c, t) == want, t
  assert optimization.ema_decay_at(c, 82) < 0.99           # the cap is first reached at s = 890: 891 / 900
  for t in (891, 892, 10 ** 6):
    assert optimization.ema_decay_at(c, t) == 0.99, t
  assert abs(optimization.ema_decay_at(c, 890) - 0.99) < 1e-15 and optimization.ema_decay_at(c, 889) < 0.99
  c3 = _cfg(ema_start_step=3)
  assert [optimization.ema_decay_at(c3, t) for t in (2, 3, 4)] == [0.0, 1 / 10, 2 / 11]
  fixed = _cfg(ema_dynamic_decay=False, ema_start_step=3, ema_average_decay=0.75)
  assert [optimization.ema_decay_at(fixed, t) for t in (1, 2, 3, 4, 10 ** 6)] == [0.0, 0.0, 0.75, 0.75, 0.75]
  assert optimization.ema_one_minus_decay(fixed, 3) == 0.25 and optimization.ema_one_minus_decay(fixed, 2) == 1.0


# ---------------------------------------------------------------- configuration
def test_the_yaml_block_is_parsed_and_its_absence_changes_nothing(tmp_path):
  path = tmp_path / 'ema.yaml'
  path.write_text(EMA_YAML)
  with warnings.catch_warnings():
    warnings.simplefilter('error')                         # nothing of the block is unknown, nothing is dropped
    oc = configs.parse_configuration('mmt/classification', [str(path)]).trainer.optimizer_config
  assert oc.ema_enabled is True
  assert (oc.ema_average_decay, oc.ema_start_step, oc.ema_dynamic_decay, oc.ema_trainable_weights_only) == (0.98, 7, False, True)
  assert oc.weight_decay_rate == 0.05 and oc.optimizer_type == 'adamw'
  # an empty block is a block: TFM's defaults
  bare = configs.get_exp_config('mmt/pretraining')
  bare.override({'trainer': {'optimizer_config': {'ema': {}}}}, strict=True)
  oc = bare.trainer.optimizer_config
  assert (oc.ema_enabled, oc.ema_average_decay, oc.ema_start_step, oc.ema_dynamic_decay) == (True, 0.99, 0, True)
  # the block absent (or `ema: null`, TFM's "no EMA"): off, no warning, and the fields of the config are the old ones
  for values in ({'trainer': {'optimizer_config': {'optimizer': {'type': 'adamw'}}}}, {'trainer': {'optimizer_config': {'ema': None}}}):
    with warnings.catch_warnings():
      warnings.simplefilter('error')
      plain = configs.get_exp_config('mmt/pretraining').override(values, strict=True)
    assert plain.trainer.optimizer_config.ema_enabled is False
    assert not any(k.startswith('ema') for k in dataclasses.asdict(plain.trainer.optimizer_config))
    assert not any(k.startswith('ema') for k in plain.as_dict()['trainer']['optimizer_config'])
  # --params_override: the block's dotted keys, and the flat fields
  dotted = configs.parse_configuration('mmt/pretraining', (), 'trainer.optimizer_config.ema.average_decay=0.9,'
                                       'trainer.optimizer_config.ema.start_step=3', strict=True).trainer.optimizer_config
  assert (dotted.ema_enabled, dotted.ema_average_decay, dotted.ema_start_step, dotted.ema_dynamic_decay) == (True, 0.9, 3, True)
  flat = configs.parse_configuration('mmt/pretraining', (), 'trainer.optimizer_config.ema_enabled=true,'
                                     'trainer.optimizer_config.ema_average_decay=0.5', strict=True).trainer.optimizer_config
  assert (flat.ema_enabled, flat.ema_average_decay) == (True, 0.5)
  # what train.py writes as params.yaml reads back
  exp = configs.parse_configuration('mmt/classification', [str(path)])
  again = configs.get_exp_config('mmt/classification').override(exp.as_dict(), strict=True).trainer.optimizer_config
  assert (again.ema_enabled, again.ema_average_decay, again.ema_start_step, again.ema_dynamic_decay) == (True, 0.98, 7, False)
  # an unknown key of the block warns like any other
  with pytest.warns(UserWarning, match='optimizer_config.ema.decay'):
    configs.get_exp_config('mmt/pretraining').override({'trainer': {'optimizer_config': {'ema': {'decay': 0.5}}}})
  with pytest.raises(KeyError):
    configs.get_exp_config('mmt/pretraining').override({'trainer': {'optimizer_config': {'ema': {'decay': 0.5}}}}, strict=True)


@pytest.mark.parametrize('bad', [{'ema_average_decay': 1.5}, {'ema_average_decay': -0.1}, {'ema_average_decay': float('nan')},
                                 {'ema_start_step': -1}, {'ema_average_decay': 'high'}])
def test_bad_values_are_refused_before_the_first_step(bad):
  m = torch.nn.Linear(4, 4)
  with pytest.raises(ValueError, match='optimizer_config.ema'):
    optimization.create_optimizer(m, _cfg(**bad))
  # without the block the same values are never looked at
  opt = optimization.create_optimizer(m, configs.OptimizerConfig(**bad))
  assert optimization.weight_averager(opt) is None


# ---------------------------------------------------------------- the host mirror
@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


def _ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _host_step(lib, param, avg, omd, word=None):
  d = lib.EmaDesc()
  d.n, d.one_minus_decay = param.size, omd
  if word is not None:
    d.one_minus_decay_dev = word.ctypes.data
  lib.check(lib.lib().mmt_ema_step_host(d, _ptr(param), _ptr(avg)))


def test_host_mirror_against_the_numpy_oracle(lib):
  """d32 = fp32(p - a); omd * d32 + a in float64, rounded once to fp32.  The mirror's fused multiply-add rounds the exact
  sum once; the float64 sum can land on an fp32 midpoint, the only way the two differ: at most 1 ulp of the result."""
  rs = np.random.RandomState(5)
  n = 3 * 1024
  param = (rs.randn(n) * np.exp(rs.randn(n) * 3)).astype(np.float32)
  avg0 = (param + rs.randn(n).astype(np.float32) * 0.05 * np.abs(param)).astype(np.float32)
  avg0[::7] = (rs.randn(len(avg0[::7])) * 10).astype(np.float32)            # far from the parameter too
  worst = 0.0
  for omd in (np.float32(1 - 2 / 11), np.float32(1 - 0.99), np.float32(0.5), np.float32(1e-3)):
    avg = avg0.copy()
    _host_step(lib, param, avg, float(omd))
    d32 = (param - avg0).astype(np.float32)
    want = (np.float64(omd) * d32.astype(np.float64) + avg0.astype(np.float64)).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    err = np.abs(avg.astype(np.float64) - want.astype(np.float64)) / ulp
    worst = max(worst, float(err.max()))
    assert float(err.max()) <= 1.0, omd
    # the device word's form (on the host: a host float) with the field poisoned
    avg2, word = avg0.copy(), np.array([omd], np.float32)
    _host_step(lib, param, avg2, 7.0, word)
    assert np.array_equal(avg.view(np.uint32), avg2.view(np.uint32))
  print('host mirror: max |mirror - oracle| =', worst, 'ulp')
  # decay 0: the parameter itself, bitwise, whatever the magnitudes; decay 1: untouched
  avg = avg0.copy()
  _host_step(lib, param, avg, 1.0)
  assert np.array_equal(avg.view(np.uint32), param.view(np.uint32))
  tiny, huge = (param * np.float32(1e-12)).astype(np.float32), (avg0 * np.float32(1e12)).astype(np.float32)
  avg = huge.copy()
  _host_step(lib, tiny, avg, 1.0)
  assert np.array_equal(avg.view(np.uint32), tiny.view(np.uint32))
  avg = avg0.copy()
  _host_step(lib, param, avg, 0.0)
  assert np.array_equal(avg.view(np.uint32), avg0.view(np.uint32))


def test_host_swap_and_refusals(lib):
  L = lib.lib()
  rs = np.random.RandomState(6)
  n = 2048
  p0, a0 = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
  param, avg, shadow = p0.copy(), a0.copy(), np.zeros(n, np.uint16)
  lib.check(L.mmt_ema_swap_host(n, _ptr(param), _ptr(avg), _ptr(shadow)))
  assert np.array_equal(param, a0) and np.array_equal(avg, p0)
  want = torch.from_numpy(a0).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
  assert np.array_equal(shadow, want)
  lib.check(L.mmt_ema_swap_host(n, _ptr(param), _ptr(avg), None))              # NULL shadow is accepted
  assert np.array_equal(param, p0) and np.array_equal(avg, a0) and np.array_equal(shadow, want)
  d = lib.EmaDesc()
  d.n, d.one_minus_decay = n, 0.5
  assert L.mmt_ema_step_host(d, _ptr(param), _ptr(param)) == -1 and b'same slab' in L.mmt_last_error()
  assert L.mmt_ema_step_host(d, None, _ptr(avg)) == -1 and b'NULL' in L.mmt_last_error()
  assert L.mmt_ema_step(d, None, None, None) == -1                             # the device entry refuses before any launch
  assert L.mmt_ema_swap(n, None, None, None, None) == -1
  for bad in (0, -1024, 1000, 1025):
    d.n = bad
    assert L.mmt_ema_step_host(d, _ptr(param), _ptr(avg)) == -1 and b'multiple of 1024' in L.mmt_last_error()
    assert L.mmt_ema_swap_host(bad, _ptr(param), _ptr(avg), None) == -1
  d.n = n
  for bad in (-1e-6, 1.0001, float('nan'), float('inf')):
    d.one_minus_decay = bad
    assert L.mmt_ema_step_host(d, _ptr(param), _ptr(avg)) == -1 and b'[0, 1]' in L.mmt_last_error()
  assert np.array_equal(param, p0) and np.array_equal(avg, a0)


# ---------------------------------------------------------------- WeightAverages
def _small_model():
  torch.manual_seed(3)
  m = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 5))
  m[2].bias.requires_grad_(False)                          # not trainable: not averaged
  return m


@pytest.mark.parametrize('kind', ['adamw', 'lamb'])
def test_weight_averages_follow_the_recurrence(kind):
  """Six steps, start_step = 2, of the optimizers `create_optimizer` returns off the flat path, against the recurrence in
  float64 on snapshots of the parameters.  Bound: 6 * 2^-23 * max(|p|, |avg|) -- one rounding of the difference and one
  of the result per step, and no growth because decay <= 1."""
  cfg = _cfg(ema_start_step=2, optimizer_type=kind, initial_learning_rate=1e-2)
  m = _small_model()
  opt = optimization.create_optimizer(m, cfg)
  assert type(opt) is (optimization.Lamb if kind == 'lamb' else torch.optim.AdamW)
  wa = optimization.weight_averager(opt)
  assert isinstance(wa, optimization.WeightAverages) and len(wa.params) == 5
  assert all(torch.equal(a, p) and a.data_ptr() != p.data_ptr() for p, a in zip(wa.params, wa.averages))     # shadow_copy
  ref = [p.detach().double().clone() for p in wa.params]
  g = torch.Generator().manual_seed(0)
  for t in range(1, 7):
    x = torch.randn(8, 33, generator=g)
    opt.zero_grad()
    m(x).square().mean().backward()
    opt.step()
    d = optimization.ema_decay_at(cfg, t)
    omd = float(np.float32(1.0 - d))
    assert wa.t == t
    for p, a, r in zip(wa.params, wa.averages, ref):
      r.add_(p.detach().double() - r, alpha=omd)
      bound = 6 * 2.0 ** -23 * torch.maximum(p.detach().abs(), a.abs()).double()
      assert bool(((a.double() - r).abs() <= bound).all()), t
      if d == 0.0:
        assert torch.equal(a, p.detach())                  # before start_step the average IS the parameter
  assert any(not torch.equal(a, p) for p, a in zip(wa.params, wa.averages))
  # swap, and the context manager also when the body raises
  before = [p.detach().clone() for p in m.parameters()]
  avgs = [a.clone() for a in wa.averages]
  with optimization.averaged_weights(opt) as inside:
    assert inside is wa
    assert all(torch.equal(p, a) for p, a in zip(wa.params, avgs))
    assert torch.equal(m[2].bias, before[-1])
  assert all(torch.equal(p, q) for p, q in zip(m.parameters(), before))
  with pytest.raises(RuntimeError, match='boom'):
    with optimization.averaged_weights(opt):
      raise RuntimeError('boom')
  assert all(torch.equal(p, q) for p, q in zip(m.parameters(), before))
  assert all(torch.equal(a, b) for a, b in zip(wa.averages, avgs))
  # without the block: nothing to swap, and the context manager is a no-op
  plain = optimization.create_optimizer(_small_model(), configs.OptimizerConfig(optimizer_type=kind))
  assert optimization.weight_averager(plain) is None
  with optimization.averaged_weights(plain) as inside:
    assert inside is None


# ---------------------------------------------------------------- checkpoints
def _task_model(seed, **task_kw):
  import mmt_amd
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': task_kw})
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.float32)
  torch.manual_seed(seed)
  return task, task.build_model()


def _trained(model, cfg, steps=3):
  """`steps` optimizer steps on made-up gradients: parameters and averages move apart."""
  opt = optimization.create_optimizer(model, cfg)
  g = torch.Generator().manual_seed(11)
  for _ in range(steps):
    for p in model.parameters():
      p.grad = torch.randn(p.shape, generator=g) * 0.1
    opt.step()
  return opt


def test_checkpoints_carry_the_averages(tmp_path):
  cfg = _cfg(initial_learning_rate=1e-2)
  task, a = _task_model(1)
  opt_a = _trained(a, cfg)
  wa = optimization.weight_averager(opt_a)
  assert any(not torch.equal(x, p) for p, x in zip(wa.params, wa.averages))
  weights = [p.detach().clone() for p in a.parameters()]
  path = checkpoint.save(str(tmp_path / 'ema'), 3, a, opt_a)
  assert all(torch.equal(p, q) for p, q in zip(a.parameters(), weights))       # swap, collect, swap back
  payload = torch.load(path, map_location='cpu', weights_only=True)
  assert set(payload) == {'step', 'items', 'optimizer', 'ema_items'}
  assert set(payload['ema_items']) == set(payload['items'])
  assert all(set(payload['ema_items'][k]) == set(payload['items'][k]) for k in payload['items'])
  # round trip: weights, averages and the step count of the averages, bitwise
  _, b = _task_model(2)
  opt_b = optimization.create_optimizer(b, cfg)
  assert checkpoint.restore(path, b, opt_b) == 3
  wb = optimization.weight_averager(opt_b)
  assert wb.t == 3
  for (n, p), q in zip(a.named_parameters(), b.parameters()):
    assert torch.equal(p, q), n
  for x, y in zip(wa.averages, wb.averages):
    assert torch.equal(x, y)
  # the restored run continues like the uninterrupted one
  g1, g2 = torch.Generator().manual_seed(12), torch.Generator().manual_seed(12)
  for model, opt, g in ((a, opt_a, g1), (b, opt_b, g2)):
    for p in model.parameters():
      p.grad = torch.randn(p.shape, generator=g) * 0.1
    opt.step()
  for x, y in zip(wa.averages, wb.averages):
    assert torch.equal(x, y)
  # an EMA file restores into an optimizer without averages, which ignores the key
  _, c = _task_model(3)
  opt_c = optimization.create_optimizer(c, configs.OptimizerConfig(initial_learning_rate=1e-2))
  assert checkpoint.restore(path, c, opt_c) == 3
  assert all(torch.equal(p, q) for p, q in zip(c.parameters(), weights))
  # a save without averages has exactly today's keys, and restores to averages equal to the parameters
  plain_path = checkpoint.save(str(tmp_path / 'plain'), 3, c, opt_c)
  assert set(torch.load(plain_path, map_location='cpu', weights_only=True)) == {'step', 'items', 'optimizer'}
  assert set(torch.load(checkpoint.save(str(tmp_path / 'bare'), 1, c), map_location='cpu', weights_only=True)) == {'step', 'items', 'optimizer'}
  _, d = _task_model(4)
  opt_d = _trained(d, cfg, steps=2)
  assert checkpoint.restore(plain_path, d, opt_d) == 3
  wd = optimization.weight_averager(opt_d)
  assert all(torch.equal(p, q) for p, q in zip(d.parameters(), weights))
  assert all(torch.equal(x, p) and x.data_ptr() != p.data_ptr() for p, x in zip(wd.params, wd.averages))


def test_warm_start_from_the_averages(tmp_path):
  cfg = _cfg(initial_learning_rate=1e-2)
  _, a = _task_model(1)
  opt_a = _trained(a, cfg)
  path = checkpoint.save(str(tmp_path / 'ema'), 3, a, opt_a)
  with optimization.averaged_weights(opt_a):
    averages = [p.detach().clone() for p in a.parameters()]
  weights = [p.detach().clone() for p in a.parameters()]
  assert any(not torch.equal(x, y) for x, y in zip(averages, weights))
  task, fresh = _task_model(5, init_checkpoint=path, init_checkpoint_averages=True)
  assert set(task.initialize(fresh)) >= {'encoder', 'masked_lm', 'masked_pp'}
  assert all(torch.equal(p, q) for p, q in zip(fresh.parameters(), averages))
  task, fresh = _task_model(5, init_checkpoint=path)                           # the default: the weights
  task.initialize(fresh)
  assert all(torch.equal(p, q) for p, q in zip(fresh.parameters(), weights))
  # a file without averages is named
  plain_path = checkpoint.save(str(tmp_path / 'plain'), 3, a)
  task, fresh = _task_model(5, init_checkpoint=plain_path, init_checkpoint_averages=True)
  with pytest.raises(ValueError, match='ckpt-3.pt'):
    task.initialize(fresh)
  # the classification task has the key too
  import mmt_amd
  cexp = configs.get_exp_config('mmt/classification')
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp.override({'task': {'init_checkpoint': path, 'init_checkpoint_averages': True,
                          'model': {'encoder': exp.task.model.encoder.as_dict(),
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': exp.task.train_data.as_dict()}}, strict=False)
  ctask = mmt_amd.tasks.get_task(cexp.task, compute_dtype=torch.float32)
  torch.manual_seed(7)
  cmodel = ctask.build_model()
  assert ctask.initialize(cmodel) == ['encoder']
  with optimization.averaged_weights(opt_a):
    for (n, p), q in zip(a.encoder.named_parameters(), cmodel.encoder.parameters()):
      assert torch.equal(p, q), n
  cexp.task.init_checkpoint = plain_path
  with pytest.raises(ValueError, match='ckpt-3.pt'):
    mmt_amd.tasks.get_task(cexp.task, compute_dtype=torch.float32).initialize(cmodel)


# ---------------------------------------------------------------- the sanitizer program
def test_sanitizer_program_of_the_ema_host_stage():
  """`make asan-ema` (csrc/Makefile): the argument checks, mmt_ema_step_host and mmt_ema_swap_host under AddressSanitizer
  + UBSan, driven by csrc/asan/ema_driver.c in exact-size heap blocks.  A stand-alone program; CPU only."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  csrc = os.path.join(root, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-ema'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'ema asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
