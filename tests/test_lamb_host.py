"""LAMB without a GPU (mmt_amd/optimization.py `Lamb`, `create_optimizer`; mmt_amd/configs.py `optimizer.type: lamb`;
csrc/lamb.hip `mmt_lamb_step_host`, the kernels' per-element and per-chunk functions as plain loops): configuration
parsing, dispatch, and both fp32 paths against the float64 oracle of tests/_lamb_cases.py within its bound."""
import ctypes
import dataclasses
import glob
import os
import warnings

import numpy as np
import pytest
import torch
import yaml

import __graft_entry__  # noqa: F401
from mmt_amd import checkpoint, configs, optimization
from tests import _lamb_cases as C

LAMB_YAML = """
trainer:
  optimizer_config:
    optimizer:
      type: lamb
      lamb:
        weight_decay_rate: 0.01
        exclude_from_weight_decay: ['LayerNorm', 'layer_norm', 'bias']
        beta_2: 0.98
    learning_rate:
      polynomial:
        initial_learning_rate: 0.002
        decay_steps: 40000
    warmup:
      polynomial:
        warmup_steps: 4000
        power: 2.0
"""

# OptimizerConfig() before this optimizer existed, field for field
ADAMW_DEFAULTS = dict(weight_decay_rate=0.01, exclude_from_weight_decay=['LayerNorm', 'layer_norm', 'bias'], beta_1=0.9, beta_2=0.999,
                      epsilon=1e-7, gradient_clip_norm=1.0, initial_learning_rate=1e-4, end_learning_rate=0.0, decay_steps=1000000,
                      power=1.0, warmup_steps=0, warmup_power=1.0)
REF_YAMLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'exp_yamls')


def test_a_lamb_block_sets_the_type_its_values_and_the_lamb_defaults(tmp_path):
  path = tmp_path / 'lamb.yaml'
  path.write_text(LAMB_YAML)
  with warnings.catch_warnings():
    warnings.simplefilter('error')                       # nothing of the block is unknown, nothing is dropped
    oc = configs.parse_configuration('mmt/pretraining', [str(path)]).trainer.optimizer_config
  assert oc.optimizer_type == 'lamb'
  assert (oc.weight_decay_rate, oc.exclude_from_weight_decay, oc.beta_2) == (0.01, ['LayerNorm', 'layer_norm', 'bias'], 0.98)
  assert (oc.epsilon, oc.beta_1, oc.exclude_from_layer_adaptation) == (1e-6, 0.9, None)       # LAMBConfig defaults for omitted keys
  assert (oc.initial_learning_rate, oc.decay_steps, oc.warmup_steps, oc.warmup_power) == (0.002, 40000, 4000, 2.0)
  assert oc.gradient_clip_norm == 1.0
  # a bare `type: lamb` takes every LAMBConfig default; an adaptation list of its own is carried
  bare = configs.get_exp_config('mmt/pretraining')
  bare.override({'trainer': {'optimizer_config': {'optimizer': {'type': 'lamb'}}}}, strict=True)
  oc = bare.trainer.optimizer_config
  assert (oc.optimizer_type, oc.weight_decay_rate, oc.exclude_from_weight_decay, oc.epsilon) == ('lamb', 0.0, [], 1e-6)
  own = configs.get_exp_config('mmt/pretraining')
  own.override({'trainer': {'optimizer_config': {'optimizer': {'type': 'lamb', 'lamb': {'exclude_from_layer_adaptation': ['bias']}}}}}, strict=True)
  assert own.trainer.optimizer_config.exclude_from_layer_adaptation == ['bias']
  # the flat spelling of --params_override
  flat = configs.parse_configuration('mmt/pretraining', (), 'trainer.optimizer_config.optimizer_type=lamb', strict=True)
  assert flat.trainer.optimizer_config.optimizer_type == 'lamb'
  assert flat.trainer.optimizer_config.epsilon == 1e-7        # (the flat key alone moves nothing else)


def test_adamw_configurations_are_unchanged_field_for_field():
  """OptimizerConfig(), an explicit `type: adamw`, and every committed reference YAML: the flattened fields are what the
  YAML's adamw / polynomial blocks say over the experiment's defaults, and the two new fields stay at their defaults."""
  assert dataclasses.asdict(configs.OptimizerConfig()) == dict(ADAMW_DEFAULTS, optimizer_type='adamw', exclude_from_layer_adaptation=None)
  cfg = configs.get_exp_config('mmt/pretraining')
  cfg.override({'trainer': {'optimizer_config': {'optimizer': {'type': 'adamw', 'adamw': {'weight_decay_rate': 0.05},
                                                               'lamb': {'epsilon': 1.0}}}}}, strict=True)
  assert dataclasses.asdict(cfg.trainer.optimizer_config) == dict(ADAMW_DEFAULTS, weight_decay_rate=0.05, optimizer_type='adamw',
                                                                  exclude_from_layer_adaptation=None)
  paths = sorted(glob.glob(os.path.join(REF_YAMLS, '*', '*', '*.yaml')))
  assert len(paths) >= 9
  for path in paths:
    exp = 'mmt/pretraining' if os.sep + 'pretrain' + os.sep in path else 'mmt/classification'
    want = dataclasses.asdict(configs.get_exp_config(exp).trainer.optimizer_config)
    oc = ((yaml.safe_load(open(path)) or {}).get('trainer') or {}).get('optimizer_config') or {}
    assert (oc.get('optimizer') or {}).get('type') in (None, 'adamw'), path
    want.update((oc.get('optimizer') or {}).get('adamw') or {})
    want.update((oc.get('learning_rate') or {}).get('polynomial') or {})
    want.update({('warmup_power' if k == 'power' else k): v for k, v in ((oc.get('warmup') or {}).get('polynomial') or {}).items()})
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      got = configs.parse_configuration(exp, [path]).trainer.optimizer_config
    assert dataclasses.asdict(got) == want, path
    assert got.optimizer_type == 'adamw' and got.exclude_from_layer_adaptation is None


def _torch_params():
  params, _ = C.inputs()
  return [(n, torch.nn.Parameter(torch.from_numpy(params[n].copy()))) for n in C.NAMES]


def _module():
  m = torch.nn.Module()
  m.dense_kernel = torch.nn.Parameter(torch.randn(130, 70))
  m.dense_bias = torch.nn.Parameter(torch.randn(130))
  m.layer_norm = torch.nn.LayerNorm(70)
  return m


def test_create_optimizer_dispatch():
  m = _module()
  opt = optimization.create_optimizer(m, C.optimizer_config())
  assert isinstance(opt, optimization.Lamb) and isinstance(opt, torch.optim.Optimizer)
  assert sum(len(g['params']) for g in opt.param_groups) == 4
  by_flags = {(g['weight_decay'], g['adapt']): len(g['params']) for g in opt.param_groups}
  assert by_flags == {(C.WD, True): 1, (0.0, False): 3}
  for cfg in (configs.OptimizerConfig(), configs.OptimizerConfig(optimizer_type='adamw'), configs.OptimizerConfig(optimizer_type='sgd')):
    assert type(optimization.create_optimizer(m, cfg)) is torch.optim.AdamW


def _run_lamb(**kw):
  named = _torch_params()
  opt = optimization.Lamb(named, lr=C.LR, betas=(C.BETA_1, C.BETA_2), eps=C.EPS, weight_decay=C.WD,
                          exclude_from_weight_decay=C.EXCLUDE, **kw)
  _, grads = C.inputs()
  want = C.oracle(C.EXCLUDE, None if 'exclude_from_layer_adaptation' not in kw else tuple(kw['exclude_from_layer_adaptation']))
  worst = 0.0
  for step in range(C.STEPS):
    for n, p in named:
      p.grad = torch.from_numpy(grads[step][n].copy())
    opt.step(grad_scale=torch.tensor(want[step][3], dtype=torch.float32))
    w, m, v, _ = want[step]
    worst = max(worst, C.max_error(dict(named), w), C.max_error({n: opt.state[p]['exp_avg'] for n, p in named}, m),
                C.max_error({n: opt.state[p]['exp_avg_sq'] for n, p in named}, v))
  return dict(named), worst


def test_lamb_matches_the_oracle():
  named, worst = _run_lamb()
  print('Lamb (torch, fp32): max |ours - oracle| =', worst)
  assert worst < C.BOUND
  # r = 1 for a parameter whose norm is zero: it moves by lr * u all the same
  assert float(named['zero/kernel'].detach().abs().max()) > 0 and float(named['layer_norm/beta'].detach().abs().max()) > 0


def test_lamb_with_an_empty_adaptation_list_adapts_the_bias_without_decay():
  named, worst = _run_lamb(exclude_from_layer_adaptation=[])
  print('Lamb, exclude_from_layer_adaptation=[]: max |ours - oracle| =', worst)
  assert worst < C.BOUND
  both = C.oracle(C.EXCLUDE, None)[-1][0]['dense/bias']
  ratio_only = C.oracle(C.EXCLUDE, ())[-1][0]['dense/bias']
  assert float(np.abs(both - ratio_only).max()) > 100 * C.BOUND      # (the two lists do give different biases)


# ---------------------------------------------------------------- the host mirror through ctypes
def _slab():
  """One slab of all eight parameters, every parameter padded to whole chunks."""
  params, _ = C.inputs()
  offs, off = {}, 0
  for n in C.NAMES:
    offs[n] = off
    off += (params[n].size + 1023) & ~1023
  a = {k: np.zeros(off, np.float32) for k in ('param', 'grad', 'm', 'v')}
  a['shadow'] = np.zeros(off, np.uint16)
  a['wd'] = np.zeros(off >> 10, np.float32)
  for n in C.NAMES:
    a['param'][offs[n]:offs[n] + params[n].size] = params[n].reshape(-1)
    if not C._matches(n, C.EXCLUDE):
      a['wd'][offs[n] >> 10:(offs[n] + params[n].size + 1023) >> 10] = C.WD
  a['seg'] = np.array([offs[n] >> 10 for n in C.NAMES] + [off >> 10], np.int32)
  a['adapt'] = np.array([0 if C._matches(n, C.EXCLUDE) else 1 for n in C.NAMES], np.int32)
  return a, offs, off


def _desc(_lib, n, n_segments, t, lr=C.LR):
  d = _lib.LambDesc()
  d.n, d.lr, d.beta1, d.beta2, d.eps = n, lr, C.BETA_1, C.BETA_2, C.EPS
  d.bias_correction1, d.bias_correction2 = 1 - C.BETA_1 ** t, 1 - C.BETA_2 ** t
  d.zero_grad, d.n_segments = 1, n_segments
  return d


def _ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def test_host_mirror_matches_the_oracle():
  from mmt_amd import _lib
  L = _lib.lib()
  a, offs, n = _slab()
  params, grads = C.inputs()
  want = C.oracle()
  ws_bytes = L.mmt_lamb_workspace_bytes(n)
  assert ws_bytes == ((n >> 10) * 12 + 15) // 16 * 16
  ws = np.zeros(ws_bytes // 4, np.float32)
  worst = 0.0
  pad = np.ones(n, bool)
  for name in C.NAMES:
    pad[offs[name]:offs[name] + params[name].size] = False
  for step in range(C.STEPS):
    for name in C.NAMES:
      a['grad'][offs[name]:offs[name] + params[name].size] = grads[step][name].reshape(-1)
    scale = np.array([want[step][3]], np.float32)
    _lib.check(L.mmt_lamb_step_host(_desc(_lib, n, len(C.NAMES), step + 1), _ptr(a['param']), _ptr(a['grad']), _ptr(a['m']), _ptr(a['v']),
                                    _ptr(a['shadow']), _ptr(a['wd']), _ptr(a['seg']), _ptr(a['adapt']), _ptr(scale), _ptr(ws), ws_bytes))
    for key, ref in zip(('param', 'm', 'v'), want[step][:3]):
      worst = max(worst, C.max_error({nm: a[key][offs[nm]:offs[nm] + params[nm].size] for nm in C.NAMES}, ref))
      assert not a[key][pad].any()                                   # padding stays exactly zero
    assert not a['grad'].any() and not a['shadow'][pad].any()
    assert np.array_equal(a['shadow'], torch.from_numpy(a['param']).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
  print('mmt_lamb_step_host: max |ours - oracle| =', worst)
  assert worst < C.BOUND


def test_every_argument_refusal_returns_its_code_and_a_message():
  from mmt_amd import _lib
  L = _lib.lib()
  a, _, n = _slab()
  ws_bytes = L.mmt_lamb_workspace_bytes(n)
  ws = np.zeros(ws_bytes // 4, np.float32)
  good = [_ptr(a['param']), _ptr(a['grad']), _ptr(a['m']), _ptr(a['v']), _ptr(a['shadow']), _ptr(a['wd']), _ptr(a['seg']), _ptr(a['adapt']),
          None, _ptr(ws), ws_bytes]
  INVALID, WORKSPACE = -1, -3

  def refused(code, d, args):
    for fn, extra in ((L.mmt_lamb_step_host, []), (L.mmt_lamb_step, [None])):     # the same checks in front of the launches
      assert fn(d, *args, *extra) == code
      assert len(L.mmt_last_error()) > 0 and (b'mmt_lamb_step' in L.mmt_last_error())

  d = _desc(_lib, n, len(C.NAMES), 1)
  refused(INVALID, None, good)
  for i in (0, 1, 2, 3, 5, 6, 7):                                    # every pointer that must not be NULL
    refused(INVALID, d, good[:i] + [None] + good[i + 1:])
  for bad_n in (0, -1024, 1000, n + 1):
    refused(INVALID, _desc(_lib, bad_n, len(C.NAMES), 1), good)
    assert L.mmt_lamb_workspace_bytes(bad_n) == 0
  for field in ('bias_correction1', 'bias_correction2'):
    for bad in (0.0, -0.5, float('nan')):
      e = _desc(_lib, n, len(C.NAMES), 1)
      setattr(e, field, bad)
      refused(INVALID, e, good)
  for bad in (0, -1):
    refused(INVALID, _desc(_lib, n, bad, 1), good)
  refused(WORKSPACE, d, good[:9] + [None, ws_bytes])
  refused(WORKSPACE, d, good[:9] + [_ptr(ws), ws_bytes - 1])
  refused(WORKSPACE, d, good[:9] + [_ptr(ws), 0])
  assert not a['m'].any() and not a['v'].any()                       # a refused call wrote nothing


def test_a_resumed_lamb_run_equals_the_uninterrupted_one(tmp_path):
  cfg = C.optimizer_config()

  def fresh():
    torch.manual_seed(3)
    m = _module()
    return m, optimization.create_optimizer(m, cfg)

  def step(m, opt, i):
    g = torch.Generator().manual_seed(100 + i)
    for p in m.parameters():
      p.grad = torch.randn(p.shape, generator=g) * 0.1
    opt.step()

  m, opt = fresh()
  for i in range(2):
    step(m, opt, i)
  path = checkpoint.save(str(tmp_path), 2, m, opt)
  step(m, opt, 2)
  m2, opt2 = fresh()
  assert checkpoint.restore(path, m2, opt2) == 2
  step(m2, opt2, 2)
  for (n, p), q in zip(m.named_parameters(), m2.parameters()):
    assert torch.equal(p, q), n
  for p, q in zip(m.parameters(), m2.parameters()):
    assert opt.state[p]['step'] == opt2.state[q]['step'] == 3
    assert torch.equal(opt.state[p]['exp_avg'], opt2.state[q]['exp_avg']) and torch.equal(opt.state[p]['exp_avg_sq'], opt2.state[q]['exp_avg_sq'])


def test_sanitizer_program_of_the_lamb_host_stage():
  """`make asan-lamb` (csrc/Makefile): the argument checks and mmt_lamb_step_host under AddressSanitizer + UBSan, driven by
  a C program with its own main in exact-size heap blocks: every refusal, slabs of 1, 2 and 7 segments, wrong segment
  tables against the clamping.  CPU only; nothing is loaded into Python."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  csrc = os.path.join(root, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-lamb'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'lamb asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
