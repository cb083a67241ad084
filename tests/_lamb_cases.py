"""LAMB test model and oracle (tests/test_lamb_host.py, tests/test_gpu_lamb.py).

The oracle is a float64 numpy restatement of the definition in include/mmt_layer.h (tfa.optimizers.LAMB, recalled): it
works on whole parameters and knows nothing of chunks, slabs or segment tables.  One parameter set is used throughout --
the AdamW test's magnitudes, with shapes that reach the edges of the 1024-element chunks.  Inputs and oracle results are
computed once per process and handed out read-only."""
import functools
import re

import numpy as np

# name, shape                                       why
SHAPES = (('dense/kernel', (130, 70)),            # 8.9 chunks, padded tail
          ('dense/bias', (130,)),                 # excluded from decay and adaptation
          ('layer_norm/gamma', (70,)),            # excluded
          ('layer_norm/beta', (70,)),             # excluded; starts at zero
          ('wide/kernel', (3, 1025)),             # 3075 elements: 4 chunks, the last almost empty
          ('exact/kernel', (1024,)),              # exactly one chunk, no padding
          ('one/kernel', (1,)),                   # zero gradient at step 1: u = wd w, r = 1 / wd
          ('zero/kernel', (33,)))                 # all zeros: ||w|| = 0, so r = 1
NAMES = tuple(n for n, _ in SHAPES)
EXCLUDE = ('LayerNorm', 'layer_norm', 'bias')
LR, WD, STEPS, CLIP = 1e-2, 0.01, 3, 1.0
BETA_1, BETA_2, EPS = 0.9, 0.999, 1e-6
BOUND = 2e-6        # max |ours - oracle| on parameters and moments: the project's number for these magnitudes
                    # (test_fused_adamw_matches_torch_adamw); a plain fp32 torch evaluation of the definition stays within 3.7e-7


def _frozen(a):
  a.setflags(write=False)
  return a


@functools.lru_cache(maxsize=None)
def inputs():
  """(params, grads): params[name] float32; grads[step][name] float32 -- randn * 0.1, times 3.0 at step 2."""
  rs = np.random.RandomState(0)
  params, grads = {}, [dict() for _ in range(STEPS)]
  for name, shape in SHAPES:
    if name == 'layer_norm/gamma':
      w = np.ones(shape, np.float32)
    elif name in ('layer_norm/beta', 'zero/kernel'):
      w = np.zeros(shape, np.float32)
    else:
      w = rs.randn(*shape).astype(np.float32)
    params[name] = _frozen(w)
    for step in range(STEPS):
      g = (rs.randn(*shape) * 0.1 * (3.0 if step == 1 else 1.0)).astype(np.float32)
      if name == 'one/kernel' and step == 0:
        g[:] = 0
      grads[step][name] = _frozen(g)
  return params, tuple(grads)


def _matches(name, patterns):
  return any(re.search(p, name) for p in patterns)


@functools.lru_cache(maxsize=None)
def oracle(exclude_decay=EXCLUDE, exclude_adapt=None, clip=CLIP):
  """Per step: (w, m, v, scale) with w / m / v dicts of float64 arrays after that step and `scale` the global-norm clip
  factor min(1, clip / (||g|| + 1e-6)) the gradients were multiplied with (1.0 when clip is None)."""
  if exclude_adapt is None:
    exclude_adapt = exclude_decay
  params, grads = inputs()
  w = {n: params[n].astype(np.float64) for n in NAMES}
  m = {n: np.zeros_like(w[n]) for n in NAMES}
  v = {n: np.zeros_like(w[n]) for n in NAMES}
  out = []
  for t in range(1, STEPS + 1):
    g64 = {n: grads[t - 1][n].astype(np.float64) for n in NAMES}
    norm = np.sqrt(sum(float((g * g).sum()) for g in g64.values()))
    scale = 1.0 if clip is None else min(1.0, clip / (norm + 1e-6))
    for n in NAMES:
      g = g64[n] * scale
      m[n] = BETA_1 * m[n] + (1 - BETA_1) * g
      v[n] = BETA_2 * v[n] + (1 - BETA_2) * g * g
      u = (m[n] / (1 - BETA_1 ** t)) / (np.sqrt(v[n] / (1 - BETA_2 ** t)) + EPS)
      if not _matches(n, exclude_decay):
        u = u + WD * w[n]
      r = 1.0
      if not _matches(n, exclude_adapt):
        wn, un = np.sqrt((w[n] * w[n]).sum()), np.sqrt((u * u).sum())
        if wn > 0 and un > 0:
          r = wn / un
      w[n] = w[n] - LR * r * u
    out.append(({n: _frozen(w[n].copy()) for n in NAMES}, {n: _frozen(m[n].copy()) for n in NAMES},
                {n: _frozen(v[n].copy()) for n in NAMES}, scale))
  return tuple(out)


def optimizer_config(**kw):
  from mmt_amd import configs
  return configs.OptimizerConfig(**dict(dict(optimizer_type='lamb', initial_learning_rate=LR, weight_decay_rate=WD, beta_1=BETA_1,
                                             beta_2=BETA_2, epsilon=EPS, exclude_from_weight_decay=list(EXCLUDE)), **kw))


def max_error(got, want):
  """max |got - want| over a dict of arrays / tensors against the oracle's float64 dict."""
  worst = 0.0
  for n in NAMES:
    a = got[n]
    a = a.detach().cpu().double().numpy() if hasattr(a, 'detach') else np.asarray(a, np.float64)
    worst = max(worst, float(np.abs(a.reshape(want[n].shape) - want[n]).max()))
  return worst
