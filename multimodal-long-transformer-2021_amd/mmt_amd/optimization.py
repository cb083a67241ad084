"""AdamW with the reference's decay-exclusion list (and LAMB, TFM's `optimizer.type: lamb`) + polynomial decay with polynomial warm-up
(`src/configs/pretraining_experiments.py:24-47`; TFM `optimization.OptimizerFactory`)."""
from __future__ import annotations

import re

import torch

from . import step_scalars
from .configs import OptimizerConfig


def learning_rate_at(cfg: OptimizerConfig, step: int) -> float:
  """TFM PolynomialDecay wrapped in PolynomialWarmUp (both power 1 by default)."""
  s = min(step, cfg.decay_steps)
  decayed = ((cfg.initial_learning_rate - cfg.end_learning_rate) *
             (1 - s / max(cfg.decay_steps, 1)) ** cfg.power + cfg.end_learning_rate)
  if cfg.warmup_steps and step < cfg.warmup_steps:
    return decayed * (step / cfg.warmup_steps) ** cfg.warmup_power
  return decayed


def split_decay_groups(named_params, exclude_patterns):
  decay, no_decay = [], []
  for name, p in named_params:
    if not p.requires_grad:
      continue
    (no_decay if any(re.search(pat, name) for pat in exclude_patterns) else decay).append(p)
  return decay, no_decay


def _matches(name, patterns):
  return any(re.search(pat, name) for pat in patterns)


def _adaptation_exclusions(cfg: OptimizerConfig):
  """LAMB's second list; absent means the decay list (tfa.optimizers.LAMB)."""
  ex = cfg.exclude_from_layer_adaptation
  return list(cfg.exclude_from_weight_decay) if ex is None else list(ex)


class _FlatSlabOptimizer:
  """What the flat optimizers share: per gradient bucket of the reducer one slab each of fp32 master parameters, the
  two moments and the bf16 shadow weights the forward pass uses (`param._mmt_shadow`), and a per-chunk weight-decay
  array (every parameter owns whole 1024-element chunks, `distribute.GradientBucketReducer`).  The parameters are
  re-homed into `slab['param']`.  A subclass adds `step`."""

  def __init__(self, named_params, cfg: OptimizerConfig, reducer, shadow_dtype=torch.bfloat16):
    from . import _lib
    self._lib = _lib
    self.cfg, self.reducer = cfg, reducer
    self.param_groups = [{'lr': cfg.initial_learning_rate}]
    self.t = 0
    names = self._names = {p: n for n, p in named_params}
    self.slabs = []
    for gi, grad in enumerate(reducer.buckets):
      n = grad.numel()
      dev = grad.device
      slab = dict(grad=grad, param=torch.zeros(n, device=dev), m=torch.zeros(n, device=dev),
                  v=torch.zeros(n, device=dev), shadow=torch.zeros(n, device=dev, dtype=shadow_dtype),
                  wd=torch.zeros(n >> 10, device=dev))
      self.slabs.append(slab)
    for p, gi, off in reducer.layout:
      slab = self.slabs[gi]
      k = p.numel()
      slab['param'][off:off + k].copy_(p.data.reshape(-1))
      p.data = slab['param'][off:off + k].view_as(p)              # re-home the parameter
      excluded = _matches(names.get(p, ''), cfg.exclude_from_weight_decay)
      slab['wd'][off >> 10:(off + k + 1023) >> 10] = 0.0 if excluded else cfg.weight_decay_rate
      p._mmt_shadow = slab['shadow'][off:off + k].view_as(p)
    for slab in self.slabs:
      slab['shadow'].copy_(slab['param'])
    for p, _, _ in reducer.layout:
      p._mmt_shadow_version = p._version     # layers._current_shadow re-syncs after any later torch-side write

  def zero_grad(self, set_to_none: bool = False):
    self.reducer.zero_grad()

  def state_dict(self):
    """Step count, learning rate and the flat moment slabs (the parameters themselves are model state)."""
    return {'t': self.t, 'lr': self.param_groups[0]['lr'],
            'slabs': [{'m': s['m'].detach().cpu(), 'v': s['v'].detach().cpu()} for s in self.slabs]}

  def load_state_dict(self, state):
    if len(state['slabs']) != len(self.slabs) or any(a['m'].numel() != b['m'].numel() for a, b in zip(state['slabs'], self.slabs)):
      raise ValueError('optimizer state does not match this model / bucket layout')
    self.t = int(state['t'])
    self.param_groups[0]['lr'] = float(state['lr'])
    for src, dst in zip(state['slabs'], self.slabs):
      dst['m'].copy_(src['m']); dst['v'].copy_(src['v'])
    self.refresh_shadow()

  def refresh_shadow(self):
    """Re-derive the bf16 shadow weights after the master parameters were written from outside
    (checkpoint restore, manual initialisation)."""
    for slab in self.slabs:
      slab['shadow'].copy_(slab['param'])
    for p, _, _ in self.reducer.layout:
      p._mmt_shadow_version = p._version

  def _fill_desc(self, d):
    c = self.cfg
    d.lr, d.beta1, d.beta2, d.eps = self.param_groups[0]['lr'], c.beta_1, c.beta_2, c.epsilon
    d.bias_correction1, d.bias_correction2 = 1 - c.beta_1 ** self.t, 1 - c.beta_2 ** self.t
    d.zero_grad = 1
    return d


class FusedAdamW(_FlatSlabOptimizer):
  """AdamW over the reducer's flat layout: one `mmt_adamw_step` launch per gradient bucket updates
  the fp32 master parameters and moments, applies the global-norm clip factor while reading the
  gradients, writes the bf16 shadow weights the forward pass uses (`param._mmt_shadow`) and
  clears the gradient bucket.  Same update rule as torch.optim.AdamW."""

  @torch.no_grad()
  def step(self, grad_scale=None):
    self.t += 1
    d = self._fill_desc(self._lib.AdamwDesc())
    L = self._lib.lib()
    for slab in self.slabs:
      d.n = slab['grad'].numel()
      dev = slab['grad'].device
      d.hyper = step_scalars.hyper_ptr(dev)       # device-resident {lr, bias corrections} of a replayed step, or None
      with torch.cuda.device(dev):
        self._lib.check(L.mmt_adamw_step(
            d, slab['param'].data_ptr(), slab['grad'].data_ptr(), slab['m'].data_ptr(), slab['v'].data_ptr(),
            slab['shadow'].data_ptr(), slab['wd'].data_ptr(),
            None if grad_scale is None else grad_scale.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream))
    self.reducer.buckets_are_zero = True


class FusedLamb(_FlatSlabOptimizer):
  """LAMB (TFM `optimizer.type: lamb`) over the reducer's flat layout: one `mmt_lamb_step` per gradient bucket -- AdamW's
  moments, then a trust ratio ||w|| / ||u|| per parameter in front of the update (include/mmt_layer.h has the
  definition).  Beside `FusedAdamW`'s slabs every slab carries its segment table (the first chunk of each parameter),
  the per-parameter adaptation flags and the kernels' workspace, all on the device: a step allocates nothing and does
  not wait for the device, so it records into a HIP graph like AdamW's."""

  def __init__(self, named_params, cfg: OptimizerConfig, reducer, shadow_dtype=torch.bfloat16):
    super().__init__(named_params, cfg, reducer, shadow_dtype)
    no_adapt = _adaptation_exclusions(cfg)
    tables = [([], []) for _ in self.slabs]
    for p, gi, off in reducer.layout:              # offsets rise within a bucket
      tables[gi][0].append(off >> 10)
      tables[gi][1].append(0 if _matches(self._names.get(p, ''), no_adapt) else 1)
    L = self._lib.lib()
    for slab, (starts, adapt) in zip(self.slabs, tables):
      n, dev = slab['grad'].numel(), slab['grad'].device
      slab['n_segments'] = len(starts)
      slab['segment_start'] = torch.tensor(starts + [n >> 10], dtype=torch.int32, device=dev)
      slab['segment_adapt'] = torch.tensor(adapt, dtype=torch.int32, device=dev)
      slab['workspace'] = torch.zeros(L.mmt_lamb_workspace_bytes(n) // 4, dtype=torch.float32, device=dev)

  @torch.no_grad()
  def step(self, grad_scale=None):
    self.t += 1
    d = self._fill_desc(self._lib.LambDesc())
    L = self._lib.lib()
    for slab in self.slabs:
      d.n = slab['grad'].numel()
      d.n_segments = slab['n_segments']
      dev = slab['grad'].device
      d.hyper = step_scalars.hyper_ptr(dev)       # device-resident {lr, bias corrections} of a replayed step, or None
      with torch.cuda.device(dev):
        self._lib.check(L.mmt_lamb_step(
            d, slab['param'].data_ptr(), slab['grad'].data_ptr(), slab['m'].data_ptr(), slab['v'].data_ptr(),
            slab['shadow'].data_ptr(), slab['wd'].data_ptr(), slab['segment_start'].data_ptr(),
            slab['segment_adapt'].data_ptr(), None if grad_scale is None else grad_scale.data_ptr(),
            slab['workspace'].data_ptr(), slab['workspace'].numel() * 4, torch.cuda.current_stream(dev).cuda_stream))
    self.reducer.buckets_are_zero = True


class Lamb(torch.optim.Optimizer):
  """LAMB per parameter in plain torch ops: the path for CPU and for GPU parameters without a reducer, and the fp32
  yardstick of `FusedLamb`.  `named_params`: (name, parameter) pairs as `named_parameters()` yields them ((parameter,
  name) is taken too); the names decide, by `re.search`, which parameters take weight decay and which a trust ratio.
  Restates tfa.optimizers.LAMB (recalled, not pinned):
    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) [+ wd w]
    r = ||w|| / ||u|| if the parameter is adapted and both norms are > 0, else 1;  w -= lr r u"""

  def __init__(self, named_params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0,
               exclude_from_weight_decay=(), exclude_from_layer_adaptation=None):
    if exclude_from_layer_adaptation is None:
      exclude_from_layer_adaptation = exclude_from_weight_decay
    groups = {}
    for a, b in named_params:
      name, p = (a, b) if isinstance(a, str) else (b, a)
      if not p.requires_grad:
        continue
      key = (not _matches(name, exclude_from_weight_decay), not _matches(name, exclude_from_layer_adaptation))
      groups.setdefault(key, []).append(p)
    super().__init__([{'params': ps, 'weight_decay': weight_decay if decay else 0.0, 'adapt': adapt}
                      for (decay, adapt), ps in sorted(groups.items(), reverse=True)],
                     dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, adapt=True))

  @torch.no_grad()
  def step(self, closure=None, grad_scale=None):
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    for group in self.param_groups:
      (b1, b2), lr, eps, wd = group['betas'], group['lr'], group['eps'], group['weight_decay']
      for p in group['params']:
        if p.grad is None:
          continue
        g = p.grad if grad_scale is None else p.grad * grad_scale
        st = self.state[p]
        if not st:
          st['step'] = 0
          st['exp_avg'], st['exp_avg_sq'] = torch.zeros_like(p), torch.zeros_like(p)
        st['step'] += 1
        t, m, v = st['step'], st['exp_avg'], st['exp_avg_sq']
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt_() + eps)
        if wd:
          u.add_(p, alpha=wd)
        if group['adapt']:
          wn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
          u.mul_(torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn)))
        p.add_(u, alpha=-lr)
    return loss


def create_optimizer(model: torch.nn.Module, cfg: OptimizerConfig, reducer=None):
  """torch.optim.AdamW (fused) by default; with a gradient reducer on the GPU, the flat
  `FusedAdamW` that shares the reducer's bucket layout.  `cfg.optimizer_type == 'lamb'`: `FusedLamb` under the same
  condition, else `Lamb`."""
  flat = reducer is not None and all(p.is_cuda for p in reducer.params)
  if cfg.optimizer_type == 'lamb':
    if flat:
      return FusedLamb(list(model.named_parameters()), cfg, reducer)
    return Lamb(model.named_parameters(), lr=cfg.initial_learning_rate, betas=(cfg.beta_1, cfg.beta_2), eps=cfg.epsilon,
                weight_decay=cfg.weight_decay_rate, exclude_from_weight_decay=cfg.exclude_from_weight_decay,
                exclude_from_layer_adaptation=cfg.exclude_from_layer_adaptation)
  if flat:
    return FusedAdamW(list(model.named_parameters()), cfg, reducer)
  decay, no_decay = split_decay_groups(model.named_parameters(), cfg.exclude_from_weight_decay)
  groups = [{'params': decay, 'weight_decay': cfg.weight_decay_rate},
            {'params': no_decay, 'weight_decay': 0.0}]
  fused = all(p.is_cuda for p in decay + no_decay)
  return torch.optim.AdamW(groups, lr=cfg.initial_learning_rate, betas=(cfg.beta_1, cfg.beta_2),
                           eps=cfg.epsilon, fused=fused)


def set_learning_rate(optimizer: torch.optim.Optimizer, lr: float) -> None:
  for g in optimizer.param_groups:
    g['lr'] = lr
