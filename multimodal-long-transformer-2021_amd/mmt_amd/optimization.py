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


def check_ema_config(cfg: OptimizerConfig) -> None:
  """ValueError for an `ema` block no decay can be computed from (`create_optimizer` calls this: before the first step)."""
  if not getattr(cfg, 'ema_enabled', False):
    return
  d, s = cfg.ema_average_decay, cfg.ema_start_step
  if isinstance(d, bool) or not isinstance(d, (int, float)) or not 0.0 <= d <= 1.0:       # NaN fails the comparison too
    raise ValueError(f'optimizer_config.ema.average_decay must be in [0, 1], got {d!r}')
  if isinstance(s, bool) or not isinstance(s, int) or s < 0:
    raise ValueError(f'optimizer_config.ema.start_step must be a non-negative integer, got {s!r}')


def ema_decay_at(cfg: OptimizerConfig, t: int) -> float:
  """Decay of the weight averages at optimizer step `t` (counted after the step's increment: 1 for the first step), in
  Python floats.  TFM `ExponentialMovingAverage` (official/modeling/optimization/ema_optimizer.py; recalled, not pinned):
  0 before `start_step` -- the average IS the parameter -- then `average_decay`, capped by (1 + s) / (10 + s) with
  s = t - start_step while `dynamic_decay` is on."""
  t = int(t)
  if t < cfg.ema_start_step:
    return 0.0
  if not cfg.ema_dynamic_decay:
    return float(cfg.ema_average_decay)
  s = t - cfg.ema_start_step
  return min(float(cfg.ema_average_decay), (1 + s) / (10 + s))


def ema_one_minus_decay(cfg: OptimizerConfig, t: int) -> float:
  """What the update multiplies with: 1 - decay in double (the descriptor, `Tensor.fill_` and numpy round it to fp32
  the same way)."""
  return 1.0 - ema_decay_at(cfg, t)


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
  re-homed into `slab['param']`.  A subclass adds `step`.

  With `cfg.ema_enabled` every slab carries one more fp32 slab, `slab['avg']`: the exponential moving average of the
  parameters (TFM `optimizer_config.ema`; `ema_decay_at`), a copy of them to begin with, updated by one `mmt_ema_step`
  launch per slab behind the slab's update launch, on the same stream -- so it is recorded with the step.  Eager steps
  carry 1 - decay in the descriptor; while the device step scalars are active the descriptor names a one-float device
  word of the optimizer's (`write_ema_scalar`), as `hyper` does for the learning rate.  `swap_weights` exchanges
  parameters and averages in place (`mmt_ema_swap`, which also writes the bf16 shadow of what becomes the parameter):
  exact, so twice is the identity."""

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
    self.ema_enabled = bool(getattr(cfg, 'ema_enabled', False))
    self._ema_word = {}                      # device -> the one-float DEVICE word mmt_ema_desc.one_minus_decay_dev names
    if self.ema_enabled:
      check_ema_config(cfg)
      for slab in self.slabs:
        slab['avg'] = slab['param'].clone()  # TFM's shadow_copy: the averages start as the parameters
        dev = slab['param'].device
        if dev not in self._ema_word:
          self._ema_word[dev] = torch.ones(1, dtype=torch.float32, device=dev)

  # ---- the weight averages (no-ops without an `ema` block) ----
  def _ema_desc(self):
    """The descriptor of this step's `mmt_ema_step` launches, or None without EMA.  `self.t` is already this step's."""
    if not self.ema_enabled:
      return None
    d = self._lib.EmaDesc()
    d.one_minus_decay = ema_one_minus_decay(self.cfg, self.t)
    return d

  def _queue_ema(self, L, d, slab, dev):
    d.n = slab['param'].numel()
    d.one_minus_decay_dev = self._ema_word[dev].data_ptr() if step_scalars.device_active(dev) else None
    self._lib.check(L.mmt_ema_step(d, slab['param'].data_ptr(), slab['avg'].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))

  def write_ema_scalar(self, t: int) -> None:
    """Queues 1 - decay of optimizer step `t` into the device word(s) on the current stream.  The value travels as a
    kernel argument of `fill_`'s launch, so the host may run ahead of the device (`DeviceStepScalars.write`)."""
    for word in self._ema_word.values():
      word.fill_(ema_one_minus_decay(self.cfg, t))

  @torch.no_grad()
  def swap_weights(self) -> None:
    """Exchanges the parameters and their averages in place, the bf16 shadows following the parameters (TFM's
    `swap_weights`).  torch's version counters are not touched and `_mmt_shadow_version` stays right: the kernel
    writes master and shadow together, as the optimizer step does."""
    if not self.ema_enabled:
      return
    L = self._lib.lib()
    for slab in self.slabs:
      dev = slab['param'].device
      with torch.cuda.device(dev):
        self._lib.check(L.mmt_ema_swap(slab['param'].numel(), slab['param'].data_ptr(), slab['avg'].data_ptr(),
                                       slab['shadow'].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))

  @torch.no_grad()
  def reset_averages(self) -> None:
    """The averages become a copy of the parameters (a restore from a file that has none)."""
    for slab in self.slabs:
      if 'avg' in slab:
        slab['avg'].copy_(slab['param'])

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
    ema = self._ema_desc()
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
        if ema is not None:
          self._queue_ema(L, ema, slab, dev)
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
    ema = self._ema_desc()
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
        if ema is not None:
          self._queue_ema(L, ema, slab, dev)
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


class WeightAverages:
  """The weight averages of an optimizer off the flat path (`torch.optim.AdamW`, `Lamb`; CPU, or no reducer) in plain
  torch ops, and the fp32 yardstick of the flat optimizers' `slab['avg']`: one fp32 average per trainable parameter, a
  copy of it to begin with, updated from a step post-hook of `optimizer` with the recurrence of `ema_decay_at`:
    avg <- fp32(avg + omd * fp32(param - avg)),  omd = fp32(1 - decay)
  -- the product and the sum in double, rounded once, which is the fused multiply-add of `mmt_ema_step` up to the last
  bit (the double sum can land on an fp32 midpoint); decay 0 copies the parameter and decay 1 changes nothing, exactly.
  `t` counts the optimizer's steps (a restore sets it from the checkpoint's step).  `swap_weights` exchanges parameters
  and averages in place."""

  def __init__(self, optimizer: torch.optim.Optimizer, cfg: OptimizerConfig):
    check_ema_config(cfg)
    self.cfg, self.t = cfg, 0
    self.params = [p for g in optimizer.param_groups for p in g['params'] if p.requires_grad]
    self.averages = [p.detach().clone() for p in self.params]
    self._hook = optimizer.register_step_post_hook(lambda *_: self.update())

  @torch.no_grad()
  def update(self) -> None:
    self.t += 1
    omd = float(torch.tensor(ema_one_minus_decay(self.cfg, self.t), dtype=torch.float32))
    if omd == 0.0:
      return
    for p, a in zip(self.params, self.averages):
      if omd == 1.0:
        a.copy_(p)
      else:
        a.copy_(a.double().add_((p - a).double(), alpha=omd))

  @torch.no_grad()
  def swap_weights(self) -> None:
    for p, a in zip(self.params, self.averages):
      tmp = p.detach().clone()
      p.copy_(a)
      a.copy_(tmp)

  @torch.no_grad()
  def reset_averages(self) -> None:
    for p, a in zip(self.params, self.averages):
      a.copy_(p)


def weight_averager(optimizer):
  """Who holds `optimizer`'s weight averages and can `swap_weights()` them in: the flat optimizer itself, the
  `WeightAverages` that `create_optimizer` hung on a torch optimizer, or None without an `ema` block."""
  if optimizer is None:
    return None
  if getattr(optimizer, 'ema_enabled', False):
    return optimizer
  return getattr(optimizer, 'weight_averages', None)


class averaged_weights:
  """`with averaged_weights(optimizer):` -- the model holds the averages inside (TFM's `swap_weights` around its
  evaluation) and its own weights again after, also when the body raises.  Nothing happens without an `ema` block."""

  def __init__(self, optimizer):
    self.averager = weight_averager(optimizer)

  def __enter__(self):
    if self.averager is not None:
      self.averager.swap_weights()
    return self.averager

  def __exit__(self, *exc):
    if self.averager is not None:
      self.averager.swap_weights()
    return False


def create_optimizer(model: torch.nn.Module, cfg: OptimizerConfig, reducer=None):
  """torch.optim.AdamW (fused) by default; with a gradient reducer on the GPU, the flat
  `FusedAdamW` that shares the reducer's bucket layout.  `cfg.optimizer_type == 'lamb'`: `FusedLamb` under the same
  condition, else `Lamb`.  With `cfg.ema_enabled` the flat optimizers keep the weight averages themselves; a torch
  optimizer gets a `WeightAverages` as `optimizer.weight_averages` (`weight_averager` finds either)."""
  check_ema_config(cfg)
  optimizer = _create_optimizer(model, cfg, reducer)
  if getattr(cfg, 'ema_enabled', False) and not hasattr(optimizer, 'slabs'):
    optimizer.weight_averages = WeightAverages(optimizer, cfg)
  return optimizer


def _create_optimizer(model: torch.nn.Module, cfg: OptimizerConfig, reducer=None):
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
