"""State that outlives a launch, host side (mmt_amd/deferred.py, and fused.py's two instances of its queue: weight-gradient
products and column-sum reduces that one launch at the end of a backward pass serves): the REAL queue code on CPU tensors, with only the launches
replaced by recorders that do the arithmetic in fp32 and log what one launch was given.  Plus the refusals of the C
boundary, which run before any launch.  No GPU."""
import contextlib
import ctypes

import pytest
import torch
from torch.utils.checkpoint import checkpoint

import __graft_entry__  # noqa: F401

M = N = 256                  # the smallest shape the grouped kernel's rules admit
K = 64


class Recorder:
  """Stands in for `_launch_wgrad_group` and `_launch_colsum_batch`."""

  def __init__(self):
    self.groups = []           # one entry per launch: [(kind, item key, output ranges)]
    self.launched = []         # item keys, in launch order
    self.keep = []             # (the items' tensors stay alive, so that no address is used twice)

  def wgrad(self, items, device):
    group = []
    for item in items:
      dw, dy, x, dbias = item.dw, item.dy, item.x, item.dbias
      self.keep.append(dy)
      dw += dy.float().t() @ x.float()
      ranges = [_range(dw)]
      if dbias is not None:
        dbias += dy.float().sum(0)
        ranges.append(_range(dbias))
      group.append(('wgrad', dy.data_ptr(), ranges))
      self.launched.append(dy.data_ptr())
    self.groups.append(group)

  def colsum(self, items, device):
    group = []
    for item in items:                                 # (the toy layers leave their finished sums in the "workspace")
      ws, outs = item.ws, item.outs
      self.keep.append(ws)
      for o, part in zip(outs, ws):
        o += part
      group.append(('colsum', ws.data_ptr(), [_range(o) for o in outs]))
      self.launched.append(ws.data_ptr())
    self.groups.append(group)

  def assert_no_launch_shares_an_output(self):
    for group in self.groups:
      flat = [(r, key) for _, key, ranges in group for r in ranges]
      for i, (a, ka) in enumerate(flat):
        for b, kb in flat[i + 1:]:
          assert not (a[0] < b[1] and b[0] < a[1]), f'one launch holds two items on the same output: {group}'


def _range(t):
  n = t.numel() if t.dim() != 2 else (t.shape[0] - 1) * t.stride(0) + t.shape[1]
  return (t.data_ptr(), t.data_ptr() + 4 * n)


def _shape_rules(dw, dy, x, dbias):
  """`_wgrad_groupable` without its device and alignment terms."""
  k, m = dy.shape
  n = x.shape[1]
  return (dw.dtype == torch.float32 and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dw.shape == (m, n)
          and x.shape[0] == k and m % 256 == 0 and n % 256 == 0 and k % 64 == 0 and k > 0 and dw.stride(1) == 1
          and (dbias is None or (dbias.dtype == torch.float32 and dbias.is_contiguous() and dbias.numel() == m)))


@pytest.fixture
def rec(monkeypatch):
  from mmt_amd import fused
  r = Recorder()
  fused.reset_host_queues()
  monkeypatch.setattr(fused, '_launch_wgrad_group', r.wgrad)
  monkeypatch.setattr(fused, '_launch_colsum_batch', r.colsum)
  monkeypatch.setattr(fused, '_wgrad_groupable', _shape_rules)
  yield r
  fused.reset_host_queues()


class ToyDense(torch.autograd.Function):
  """y = x W^T (+ b) whose backward queues its weight gradient as `layers._accumulate_dense_grads` does.  `slot` names
  the gradient buffers: the parameters' `.grad`, or views the test hands in."""

  @staticmethod
  def forward(ctx, x, weight, bias, slot):
    from mmt_amd import fused
    fused._desc(x)                       # (every fused op fills a descriptor in its forward pass)
    ctx.save_for_backward(x)
    ctx.weight, ctx.bias, ctx.slot = weight, bias, slot
    y = x.float() @ weight.detach().t()
    if bias is not None:
      y = y + bias.detach()
    return y.bfloat16()

  @staticmethod
  def backward(ctx, dy):
    from mmt_amd import fused
    x, = ctx.saved_tensors
    dw, db = ctx.slot(ctx.weight, ctx.bias)
    if ToyDense.raise_here(ctx.weight):
      raise RuntimeError('backward fails here (test)')
    dy = dy.contiguous()
    notify = (ctx.weight,) if ctx.bias is None else (ctx.weight, ctx.bias)
    assert fused.wgrad_accumulate_deferred_(dw, dy, x, db, notify)
    return (dy.float() @ ctx.weight.detach()).bfloat16(), None, None, None

  raise_here = staticmethod(lambda weight: False)


class ToyBias(torch.autograd.Function):
  """y = x + c whose backward leaves the column sums of dy in a "workspace" and queues their reduce into c.grad."""

  @staticmethod
  def forward(ctx, x, c):
    from mmt_amd import fused
    fused._desc(x)
    ctx.c = c
    return (x.float() + c.detach()).bfloat16()

  @staticmethod
  def backward(ctx, dy):
    from mmt_amd import fused
    ws = dy.float().sum(0, keepdim=True)
    fused._defer_colsum(ws, dy.shape[0], dy.shape[1], 3, (ctx.c.grad,))
    return dy, None


def _grads(weight, bias):
  return weight.grad, (None if bias is None else bias.grad)


def _param(*shape, seed):
  g = torch.Generator().manual_seed(seed)
  p = torch.nn.Parameter(torch.randn(*shape, generator=g) * 0.05)
  p.grad = torch.randn(*shape, generator=g)                   # preset fp32 master gradient: products ADD to it
  return p


def _x(seed, rows=K):
  return (torch.randn(rows, N, generator=torch.Generator().manual_seed(seed))).bfloat16().requires_grad_(True)


# ---- shared outputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_bias', [False, True], ids=['dw', 'dw+dbias'])
def test_a_weight_used_twice_goes_into_two_launches(rec, with_bias):
  """Two products into ONE dw (and dbias) in one backward pass: never in the same launch -- the queue is flushed before
  the second one is appended -- and the gradient is the fp64 sum of both contributions."""
  w, b = _param(M, N, seed=1), (_param(M, seed=2) if with_bias else None)
  other = _param(M, N, seed=3)
  w0, b0 = w.grad.clone(), (b.grad.clone() if with_bias else None)
  x = _x(4)
  h1 = ToyDense.apply(x, w, b, _grads)
  h2 = ToyDense.apply(h1, other, None, _grads)
  h3 = ToyDense.apply(h2, w, b, _grads)
  dy = torch.randn(K, M, generator=torch.Generator().manual_seed(5)).bfloat16()
  h3.backward(dy)
  rec.assert_no_launch_shares_an_output()
  assert len(rec.launched) == 3 and len(set(rec.launched)) == 3
  assert len(rec.groups) == 2 and [len(g) for g in rec.groups] == [2, 1]        # flushed BEFORE the duplicate was queued
  # reference: the definition in fp64 on the stored bf16 operands
  d3 = dy.double()                                          # (the bf16 gradients the layers handed down, as they did)
  d2 = (dy.float() @ w.detach()).bfloat16()
  d1 = (d2.float() @ other.detach()).bfloat16().double()
  want = w0.double() + d3.t() @ h2.detach().double() + d1.t() @ x.detach().double()
  assert float((w.grad.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())
  if with_bias:
    want_b = b0.double() + d3.sum(0) + d1.sum(0)
    assert float((b.grad.double() - want_b).abs().max()) <= 2e-5 * float(want_b.abs().max())
  from mmt_amd import fused
  assert not fused._wg_deferred
  assert not any(getattr(p, '_mmt_grad_deferred', False) for p in (w, other) + ((b,) if with_bias else ()))


def test_overlap_is_judged_by_address_range_not_by_pointer():
  """(the pure helper) A view into the same buffer at an offset overlaps; disjoint row blocks of one buffer do not."""
  from mmt_amd import fused
  buf = torch.zeros(3 * M, N)
  a, b, c = buf[:M], buf[M:2 * M], buf[M // 2:M // 2 + M]
  ra, rb, rc = (fused._byte_range(a),), (fused._byte_range(b),), (fused._byte_range(c),)
  assert not fused._ranges_overlap(ra, rb)
  assert fused._ranges_overlap(ra, rc) and fused._ranges_overlap(rc, rb)
  assert c.data_ptr() not in (a.data_ptr(), b.data_ptr())


def test_a_view_into_the_same_gradient_at_an_offset_counts_as_shared(rec):
  """Two layers whose gradient buffers are overlapping views of one flat buffer (different data pointers): two launches;
  two layers on disjoint row blocks of the same buffer: one."""
  flat = torch.zeros(3 * M, N)
  views = {}
  wa, wb, wc = (_param(M, N, seed=s) for s in (1, 2, 3))
  views[wa], views[wb], views[wc] = flat[:M], flat[M // 2:M // 2 + M], flat[2 * M:]
  slot = lambda weight, bias: (views[weight], None)
  x = _x(6)
  h = ToyDense.apply(ToyDense.apply(ToyDense.apply(x, wc, None, slot), wb, None, slot), wa, None, slot)
  dy = torch.randn(K, M, generator=torch.Generator().manual_seed(7)).bfloat16()
  h.backward(dy)
  rec.assert_no_launch_shares_an_output()
  assert [len(g) for g in rec.groups] == [1, 2]          # wa alone; wb (overlaps wa) with wc (disjoint rows of the buffer)
  d_a = dy.double()                                         # (the bf16 gradients the layers handed down, as they did)
  d_b = (dy.float() @ wa.detach()).bfloat16()
  d_c = (d_b.float() @ wb.detach()).bfloat16().double()
  d_b = d_b.double()
  h_c = ToyDense.apply(x, wc, None, slot).detach()
  h_b = ToyDense.apply(h_c, wb, None, slot).detach()
  want = torch.zeros(3 * M, N, dtype=torch.float64)
  want[:M] += d_a.t() @ h_b.double()
  want[M // 2:M // 2 + M] += d_b.t() @ h_c.double()
  want[2 * M:] += d_c.t() @ x.detach().double()
  assert float((flat.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_a_reduce_output_used_twice_goes_into_two_launches(rec):
  """The same for the queued column-sum reduces: one bias parameter used by two layers of one pass."""
  c, other = _param(N, seed=1), _param(N, seed=2)
  c0 = c.grad.clone()
  x = _x(8)
  y = ToyBias.apply(ToyBias.apply(ToyBias.apply(x, c), other), c)
  dy = torch.randn(K, N, generator=torch.Generator().manual_seed(9)).bfloat16()
  y.backward(dy)
  rec.assert_no_launch_shares_an_output()
  assert [len(g) for g in rec.groups] == [2, 1]
  want = c0.double() + 2 * dy.double().sum(0)
  assert float((c.grad.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())
  from mmt_amd import fused
  assert not fused._cs_deferred


# ---- nested backward ---------------------------------------------------------------------------------------------------

def _stack(params, x, use_checkpoint):
  """Two levels of (dense + bias, dense); the lower one optionally under a re-entrant checkpoint."""
  (w0, b0, c0, w1), (w2, b2, c2, w3) = params

  def level(t, w_a, b_a, c_a, w_b):
    return ToyDense.apply(ToyBias.apply(ToyDense.apply(t, w_a, b_a, _grads), c_a), w_b, None, _grads)
  lower = lambda t: level(t, w0, b0, c0, w1)
  h = checkpoint(lower, x, use_reentrant=True) if use_checkpoint else lower(x)
  return level(h, w2, b2, c2, w3)


def _stack_params():
  mk = lambda s: (_param(M, N, seed=s), _param(M, seed=s + 1), _param(N, seed=s + 2), _param(M, N, seed=s + 3))
  return mk(10), mk(20)


def _run_stack(rec, use_checkpoint):
  params = _stack_params()
  flat = [p for level in params for p in level]
  fired = {id(p): 0 for p in flat}
  weights = [p for p in flat if p.dim() == 2] + [params[0][1], params[1][1]]
  for p in weights:                               # (parameters with hooks keep their column-sum reduces out of the queue
    p._mmt_grad_ready_hooks = (lambda q: fired.__setitem__(id(q), fired[id(q)] + 1),)      # in the real layers: dense only)
  x = _x(30)
  y = _stack(params, x, use_checkpoint)
  dy = torch.randn(K, M, generator=torch.Generator().manual_seed(31)).bfloat16()
  y.backward(dy)
  return flat, weights, fired, x.grad.clone()


def test_a_nested_backward_pass_keeps_the_outer_passes_queue(rec):
  """The lower half of a two-level stack under `checkpoint(..., use_reentrant=True)`: its recomputed segment runs an
  inner backward pass with a graph-task id of its own.  Every product and reduce of the outer pass and of the inner pass
  is launched exactly once, every gradient equals the run without checkpointing bit for bit, no parameter stays marked
  as queued, and every gradient-ready hook has run once."""
  from mmt_amd import fused
  plain, _, _, dx_plain = _run_stack(rec, False)
  n_plain = len(rec.launched)
  assert n_plain == 6 and len(set(rec.launched)) == 6          # four products + two reduces
  rec.groups.clear(); rec.launched.clear()
  nested, weights, fired, dx_nested = _run_stack(rec, True)
  assert len(rec.launched) == 6 and len(set(rec.launched)) == 6
  assert len(rec.groups) == 4                                   # (products, reduces) x (outer pass, inner pass)
  rec.assert_no_launch_shares_an_output()
  for a, b in zip(plain, nested):
    assert torch.equal(a.grad, b.grad)
  assert torch.equal(dx_plain, dx_nested)
  assert not any(getattr(p, '_mmt_grad_deferred', False) for p in nested)
  assert [fired[id(p)] for p in weights] == [1] * len(weights)
  assert not fused._wg_deferred and not fused._cs_deferred


# ---- stale entries -----------------------------------------------------------------------------------------------------

def test_a_backward_that_raises_leaves_nothing_a_later_pass_launches(rec, monkeypatch):
  """A pass that raises half-way strands its queued items (its end-of-backward callback never runs): the next pass
  launches its own items only, the stranded ones are dropped and their parameters are no longer marked as queued."""
  from mmt_amd import fused
  (w0, b0, c0, w1), (w2, b2, c2, w3) = params = _stack_params()
  before = [p.grad.clone() for level in params for p in level]
  x = _x(40)
  y = _stack(params, x, False)
  monkeypatch.setattr(ToyDense, 'raise_here', staticmethod(lambda weight: weight is w1))
  with pytest.raises(RuntimeError, match='fails here'):
    y.backward(torch.ones_like(y))
  assert len(fused._wg_deferred.queued()) == 2 and len(fused._cs_deferred.queued()) == 1
  assert w3._mmt_grad_deferred and w2._mmt_grad_deferred
  assert not rec.launched
  monkeypatch.setattr(ToyDense, 'raise_here', staticmethod(lambda weight: False))
  # a later pass over other parameters
  w, c = _param(M, N, seed=50), _param(N, seed=51)
  w_before = w.grad.clone()
  x2 = _x(41)
  z = ToyBias.apply(ToyDense.apply(x2, w, None, _grads), c)
  dz = torch.randn(K, M, generator=torch.Generator().manual_seed(42)).bfloat16()
  z.backward(dz)
  assert len(rec.launched) == 2 and [len(g) for g in rec.groups] == [1, 1]
  assert torch.equal(w.grad, w_before + dz.float().t() @ x2.detach().float())
  for p, g in zip([p for level in params for p in level], before):
    assert torch.equal(p.grad, g)                              # nothing of the pass that raised was ever added
  assert not fused._wg_deferred and not fused._cs_deferred
  assert not any(getattr(p, '_mmt_grad_deferred', False) for level in params for p in level)


def test_reset_host_queues_empties_everything(rec, monkeypatch):
  from mmt_amd import fused
  (w0, b0, c0, w1), upper = params = _stack_params()
  y = _stack(params, _x(43), False)
  monkeypatch.setattr(ToyDense, 'raise_here', staticmethod(lambda weight: weight is w0))
  with pytest.raises(RuntimeError, match='fails here'):
    y.backward(torch.ones_like(y))
  assert fused._wg_deferred and fused._cs_deferred
  fused.reset_host_queues()
  assert not fused._wg_deferred and not fused._cs_deferred
  assert not any(getattr(p, '_mmt_grad_deferred', False) for level in params for p in level)
  assert not rec.launched


# ---- when a queue launches: its limit, and which items may share a launch ---------------------------------------------

def _outputs(group):
  """First output range of every item of one recorded launch, in the launch's order."""
  return [ranges[0] for _, _, ranges in group]


def test_the_reduce_queue_launches_at_its_limit(rec):
  """One more reduce than a batch holds, every one on an output of its own: a full batch is launched when the last
  place is taken, the one left over at the end of backward, both in the order the reduces were queued."""
  from mmt_amd import fused
  n = fused._CS_MAX + 1
  cs = [_param(N, seed=60 + i) for i in range(n)]
  before = [c.grad.clone() for c in cs]
  y = _x(59)
  for c in cs:
    y = ToyBias.apply(y, c)
  dy = torch.randn(K, N, generator=torch.Generator().manual_seed(58)).bfloat16()
  y.backward(dy)
  rec.assert_no_launch_shares_an_output()
  assert [len(g) for g in rec.groups] == [fused._CS_MAX, 1]
  queued = [_range(c.grad) for c in reversed(cs)]            # (backward meets the layers last to first)
  assert _outputs(rec.groups[0]) + _outputs(rec.groups[1]) == queued
  for c, g in zip(cs, before):
    assert torch.equal(c.grad, g + dy.float().sum(0))
  assert not fused._cs_deferred


def test_products_of_another_k_go_into_another_launch(rec):
  """Products with K = 64, 64, 128, 128 on outputs of their own, queued in that order by one backward pass: two
  launches of two, neither of them mixed (one grouped launch has one K)."""
  from mmt_amd import fused
  ws = [_param(M, N, seed=70 + i) for i in range(4)]
  k_of = {_range(w.grad): k for w, k in zip(ws, (2 * K, 2 * K, K, K))}
  xs = {k: _x(74 + k, rows=k) for k in (K, 2 * K)}
  # the graph of the K = 128 pair is built first, so backward (latest node first) meets the K = 64 pair first
  ys = [ToyDense.apply(ToyDense.apply(xs[k], a, None, _grads), b, None, _grads) for k, (a, b) in ((2 * K, ws[:2]), (K, ws[2:]))]
  dys = [torch.randn(k, M, generator=torch.Generator().manual_seed(78 + k)).bfloat16() for k in (2 * K, K)]
  torch.autograd.backward(ys, dys)
  rec.assert_no_launch_shares_an_output()
  assert [[k_of[r] for r in _outputs(g)] for g in rec.groups] == [[K, K], [2 * K, 2 * K]]
  assert len(set(rec.launched)) == 4
  assert not fused._wg_deferred
  assert not any(getattr(w, '_mmt_grad_deferred', False) for w in ws)


def _run_chain(rec, n, with_hooks):
  """`n` dense layers in a row, every weight with a gradient of its own; with hooks, every call of one is logged as
  (parameter, products launched so far, was its own product among them)."""
  ws = [_param(M, N, seed=80 + i) for i in range(n)]
  calls = []
  if with_hooks:
    launched_outputs = lambda: [r for g in rec.groups for r in _outputs(g)]
    for w in ws:
      w._mmt_grad_ready_hooks = (lambda q: calls.append((q, len(rec.launched), _range(q.grad) in launched_outputs())),)
  y = _x(79)
  for w in ws:
    y = ToyDense.apply(y, w, None, _grads)
  y.backward(torch.randn(K, M, generator=torch.Generator().manual_seed(78)).bfloat16())
  return ws, calls


def test_the_product_queue_launches_sooner_when_somebody_listens(rec):
  """One more product than a block's group holds.  With gradient-ready hooks on the parameters (a reducer listens) the
  queue launches when the group is full and again at the end of backward; every hook runs once, after the launch that
  holds its parameter's product, and no parameter stays marked as queued.  Without hooks nobody waits: one launch at
  the end of backward."""
  from mmt_amd import fused
  n = fused._WG_GROUP + 1
  assert n < fused._WG_GROUP_ALONE
  ws, calls = _run_chain(rec, n, True)
  rec.assert_no_launch_shares_an_output()
  assert [len(g) for g in rec.groups] == [fused._WG_GROUP, 1]
  queued = [_range(w.grad) for w in reversed(ws)]
  assert _outputs(rec.groups[0]) + _outputs(rec.groups[1]) == queued
  assert [q for q, _, _ in calls] == list(reversed(ws))                      # once per parameter, in launch order
  assert [seen for _, seen, _ in calls] == [fused._WG_GROUP] * fused._WG_GROUP + [n]    # the first launch came before the last product
  assert all(own for _, _, own in calls)
  assert not any(getattr(w, '_mmt_grad_deferred', False) for w in ws)
  assert not fused._wg_deferred
  rec.groups.clear(); rec.launched.clear()
  ws, calls = _run_chain(rec, n, False)
  assert [len(g) for g in rec.groups] == [n] and not calls
  assert _outputs(rec.groups[0]) == [_range(w.grad) for w in reversed(ws)]
  assert not any(getattr(w, '_mmt_grad_deferred', False) for w in ws)
  assert not fused._wg_deferred


# ---- the C boundary ----------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _host_buffers(n_floats):
  """Addresses for the refusal tests: nothing is ever read or written through them (the refusal comes first), but they
  are real so that a regression that reached a launch would not touch foreign memory either."""
  buf = (ctypes.c_float * (n_floats + 4))()
  yield (ctypes.addressof(buf) + 15) & ~15


def _problems(base, dw_offsets, db_offsets=None, ldw=N):
  from mmt_amd import _lib
  probs = (_lib.WgradProblem * len(dw_offsets))()
  for i, q in enumerate(probs):
    q.dw, q.ldw = base + 4 * dw_offsets[i], ldw
    q.dbias = None if db_offsets is None or db_offsets[i] is None else base + 4 * db_offsets[i]
    q.dy, q.ldy, q.x, q.ldx, q.M, q.N = base, M, base, N, M, N          # (operands may alias: they are only read)
  return probs


def test_wgrad_grouped_refuses_overlapping_outputs_without_gpu():
  """`mmt_wgrad_grouped` returns MMT_E_INVALID (-1) and `mmt_wgrad_group_workspace_bytes` 0 for a group in which two
  problems' dw ranges (M rows of ldw) or dbias ranges overlap, each with a message that names the two problems; disjoint
  row blocks of one buffer are not an overlap (the size query accepts them; no launch is attempted here)."""
  from mmt_amd import _lib
  L = _lib.lib()
  with _host_buffers(4 * M * N + 4 * M) as base:
    bias0 = 4 * M * N
    cases = {
        'same dw': (_problems(base, [0, M * N, 0]), b'dw of problem 2 overlaps dw of problem 0'),
        'dw view at an offset': (_problems(base, [0, M * N // 2 + 64]), b'dw of problem 1 overlaps dw of problem 0'),
        'last row only': (_problems(base, [0, (M - 1) * N + N - 4]), b'dw of problem 1 overlaps dw of problem 0'),
        'same dbias': (_problems(base, [0, M * N, 2 * M * N], [bias0, None, bias0]), b'dbias of problem 2 overlaps dbias of problem 0'),
        'dbias view at an offset': (_problems(base, [0, M * N], [bias0, bias0 + M - 4]), b'dbias of problem 1 overlaps dbias of problem 0'),
    }
    for name, (probs, message) in cases.items():
      n = len(probs)
      assert L.mmt_wgrad_group_workspace_bytes(n, probs, K) == 0, name
      assert message in L.mmt_last_error(), (name, L.mmt_last_error())
      assert L.mmt_wgrad_grouped(n, probs, K, None, 0, None) == -1, name
      assert b'mmt_wgrad_grouped' in L.mmt_last_error() and message in L.mmt_last_error(), (name, L.mmt_last_error())
    # what is NOT an overlap: consecutive row blocks, and a dbias right behind another
    ok = _problems(base, [0, M * N, 2 * M * N, 3 * M * N], [bias0, bias0 + M, None, bias0 + 2 * M])
    assert L.mmt_wgrad_group_workspace_bytes(4, ok, 4096) > 0          # (16 tiles, K = 4096: split, so slabs are needed)
    assert L.mmt_wgrad_grouped(4, ok, 4096, None, 0, None) == -3        # MMT_E_WORKSPACE: past the overlap check, still no launch


def test_colsum_reduce_batch_refuses_overlapping_outputs_without_gpu():
  """`mmt_colsum_reduce_batch`: two items (or two outputs of one item) on overlapping memory are MMT_E_INVALID with both
  items named, before any launch."""
  from mmt_amd import _lib
  L = _lib.lib()
  H = 256

  def items(*specs):
    arr = (_lib.ColsumItem * len(specs))()
    for q, (kind, outs) in zip(arr, specs):
      o = list(outs) + [None] * (3 - len(outs))
      q.workspace, q.o0, q.o1, q.o2 = base, *(None if v is None else base + 4 * v for v in o)
      q.rows, q.H, q.kind, q.accumulate = 512, H, kind, 1
    return arr
  with _host_buffers(16 * H) as base:
    cases = {
        'same bias': (items((3, [0]), (3, [H]), (3, [0])), b'output 0 of item 2 overlaps output 0 of item 0'),
        'gamma of two LayerNorms': (items((0, [0, H]), (1, [2 * H, 0, 3 * H])), b'output 1 of item 1 overlaps output 0 of item 0'),
        'view at an offset': (items((3, [0]), (2, [H - 8])), b'output 0 of item 1 overlaps output 0 of item 0'),
        'within one item': (items((0, [0, 0])), b'output 1 of item 0 overlaps output 0 of item 0'),
    }
    for name, (arr, message) in cases.items():
      assert L.mmt_colsum_reduce_batch(len(arr), arr, None) == -1, name
      assert b'mmt_colsum_reduce_batch' in L.mmt_last_error() and message in L.mmt_last_error(), (name, L.mmt_last_error())
