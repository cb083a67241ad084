"""Attention parity on strided [B,S,N,D] views (include/mmt_attn.h: arbitrary element strides, D contiguous).

Every case calls the kernels twice, on contiguous tensors and on views that live in NaN-poisoned storages
(tests/_cases.py `strided_view`), and asserts
  (a) the strided result within the standing tolerances of the dense fp64 oracle (output and lse, gradients: the bars
      of tests/_cases.py, through tests/_parity.py `check_against`), and
  (b) the strided result BIT FOR BIT equal to the contiguous call on the same route: addresses do not enter the
      arithmetic, and no route's instruction order depends on the layout.
Gradient storages are pre-filled with the poison pattern and must hold it outside the views afterwards.

With dropout the oracle is fed the restated keep mask (oracle.dropout_keep_mask), which is indexed by (b, n, q, k) and
not by address.

Shapes: the smallest with several 32-row tiles, a ragged tail, a 128-row block boundary, global rows and keys, and two
planes in each of b and n (CASES below).
"""
import functools

import numpy as np
import pytest
import torch

from tests._cases import (BF16_GRAD_TOL, BF16_TOL, F32_GRAD_TOL, LAYOUTS, assert_gaps_untouched, dense_side_inputs,
                          grad_error, parity_inputs, strided_view, _int_view)
from tests._parity import GRAD_NAMES, check_against, oracle_call, to_dev

pytestmark = pytest.mark.gpu

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
DROP_P, DROP_SEED = 0.1, 0x5EED_0123_4567

_A = dict(kind='pattern', B=2, S=200, N=2, D=64, R=32, id_mode=1, m=12, radius=40, g0=70, ng=8, valid=[200, 131])
CASES = {
    'A': _A,
    'B': dict(kind='pattern', B=1, S=200, N=2, D=64, R=49, id_mode=2, m=12, P=10, r=2, radius=20, g0=150, ng=5),
    'C': dict(_A, D=128, radius=32),
    'D': dict(kind='dense', B=2, S=96, N=2, D=64, R=9, id_mode=1, m=3),
    'E': dict(kind='packed', B=2, S=200, N=2, D=64, R=32, id_mode=1, m=12, radius=8, g0=100, ng=8,
              lengths=[[70, 80, 50], [33, 71, 64]]),
    'F': dict(kind='grid', B=2, S=200, N=2, D=64, R=32, id_mode=1, m=12, radius=8, g0=146, ng=8, P=12, a=1, g=2),
    # section "offsets at the documented limit": case A's pattern, one plane, S = 1000
    'A1000': dict(kind='pattern', B=1, S=1000, N=1, D=64, R=32, id_mode=1, m=12, radius=40, g0=70, ng=8, valid=[931]),
}


def _tuning(names):
  from mmt_amd import _lib
  t = 0
  for n in names.split('|'):
    if n != '0':
      t |= getattr(_lib, 'MMT_TUNE_' + n)
  return t


class Problem:
  """Inputs of one case in one dtype: numpy (the oracle's), contiguous device tensors, the call's keyword arguments."""

  def __init__(self, case, dt, dropout=0.0, broadcast=None):
    import mmt_amd
    c = self.cfg = CASES[case]
    self.dtype = DT[dt]
    B, S, N, D, R = c['B'], c['S'], c['N'], c['D'], c['R']
    q, k, v, emb, bias, dout = parity_inputs(B, S, N, R, self.dtype, seed=17, D=D)
    if broadcast == 'broadcast_heads':
      k, v = (np.broadcast_to(x[:, :, :1], x.shape).copy() for x in (k, v))
    if broadcast == 'broadcast_batch':
      k, v = (np.broadcast_to(x[:1], x.shape).copy() for x in (k, v))
    self.np = dict(q=q, k=k, v=v, emb=emb, bias=bias, dout=dout)
    kind, m = c['kind'], c['m']
    if kind == 'packed':
      self.ids = mmt_amd.example_ids_from_lengths(c['lengths'], S).numpy()
    mask, ids = dense_side_inputs(B, S, c.get('valid'), c.get('radius', 1 << 30), c.get('g0', 0), c.get('ng', 0), c['id_mode'],
                                  m, c.get('P', 0), c.get('r', 0), a=c.get('a', 0), g=c.get('g', 2),
                                  example_ids=self.ids if kind == 'packed' else None)
    self.mask, self.rel_ids = mask, ids
    self.dropout = dropout
    self._ref = None
    self.t = {n: to_dev(x, self.dtype) for n, x in self.np.items()}
    pat_kw = dict(local_radius=c.get('radius', 1 << 30), global_start=c.get('g0', 0), n_global=c.get('ng', 0),
                  id_mode=c['id_mode'], max_dist=m, patches_per_row=c.get('P', 0), core_layers=c.get('r', 0))
    if kind == 'dense':
      self.kw = dict(att_mask=to_dev(mask, torch.int32), relative_att_ids=to_dev(ids, torch.int32))
    elif kind == 'packed':
      self.kw = dict(pattern=mmt_amd.AttentionPattern(**pat_kw), example_ids=torch.from_numpy(self.ids).cuda())
    elif kind == 'grid':
      self.kw = dict(pattern=mmt_amd.AttentionPattern(grid_radius=c['a'], grid_start=c['g'], **pat_kw))
    else:
      vl = c.get('valid')
      self.kw = dict(pattern=mmt_amd.AttentionPattern(**pat_kw),
                     valid_len=None if vl is None else torch.tensor(vl, dtype=torch.int32, device='cuda'))
    if dropout:
      self.kw.update(dropout_p=dropout, dropout_seed=DROP_SEED)

  @property
  def ref(self):
    """The dense fp64 oracle: computed once per problem, shared by every test on it, never written."""
    if self._ref is None:
      self._ref = oracle_call(tuple(self.np.values()), self.mask, self.rel_ids,
                              dropout=(self.dropout, DROP_SEED) if self.dropout else None)
    return self._ref

  # ---- assertion (a) ----
  def check_forward(self, out, lse, what=''):
    check_against({'out': out, 'lse': lse}, {n: self.ref[n] for n in ('out', 'lse')}, self.dtype, what)

  def check_grads(self, grads, what='', only=None):
    names = GRAD_NAMES if only is None else only
    assert len(grads) == len(names)
    check_against(dict(zip(names, grads)), {n: self.ref[n] for n in names}, self.dtype, what)


@functools.lru_cache(maxsize=None)
def _problem(case, dt, dropout, broadcast):
  return Problem(case, dt, dropout, broadcast)


def problem(case, dt, dropout=0.0, broadcast=None):
  return _problem(case, dt, float(dropout), broadcast)


def contiguous_forward(case, dt, tuning, dropout=0.0, broadcast=None):
  """The call on contiguous tensors: made once per route, shared, never written."""
  return _contiguous_forward(case, dt, tuning, float(dropout), broadcast)


def contiguous_backward(case, dt, tuning, dropout=0.0):
  return _contiguous_backward(case, dt, tuning, float(dropout))


@functools.lru_cache(maxsize=None)
def _contiguous_forward(case, dt, tuning, dropout, broadcast):
  import mmt_amd
  p = problem(case, dt, dropout, broadcast)
  t = p.t
  return mmt_amd.relative_attention_forward(t['q'], t['k'], t['v'], t['emb'], t['bias'], tuning=_tuning(tuning), **p.kw)


@functools.lru_cache(maxsize=None)
def _contiguous_backward(case, dt, tuning, dropout):
  import mmt_amd
  p = problem(case, dt, dropout)
  t = p.t
  out, lse = contiguous_forward(case, dt, tuning, dropout)
  return mmt_amd.relative_attention_backward(t['dout'], t['q'], t['k'], t['v'], t['emb'], t['bias'], out, lse,
                                             tuning=_tuning(tuning), **p.kw)


# ---- assertion (b) ----
def assert_same_bits(got, want, what):
  assert got.shape == want.shape and got.dtype == want.dtype, what
  a, b = got.contiguous(), want.contiguous()
  a, b = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a.view(torch.int16), b.view(torch.int16))
  diff = int((a != b).sum())
  assert diff == 0, f'{what}: {diff} of {a.numel()} elements differ in bits from the contiguous call'


def _layouts3(layout):
  return tuple(layout.split('+')) if '+' in layout else (layout,) * 3


MIXED = 'head_major+qkv_per_head+padded'


def run_forward(case, dt, tuning, layout, dropout=0.0):
  import mmt_amd
  p = problem(case, dt, dropout)
  base_out, base_lse = contiguous_forward(case, dt, tuning, dropout)
  views = [strided_view(p.t[n], lay, slot=i) for i, (n, lay) in enumerate(zip('qkv', _layouts3(layout)))]
  out, lse = mmt_amd.relative_attention_forward(views[0][0], views[1][0], views[2][0], p.t['emb'], p.t['bias'],
                                                tuning=_tuning(tuning), **p.kw)
  torch.cuda.synchronize()
  what = f'{case}-{dt}-{tuning}-{layout}'
  p.check_forward(base_out, base_lse, what + ' (contiguous)')
  p.check_forward(out, lse, what)
  assert_same_bits(out, base_out, what + ' out')
  assert_same_bits(lse, base_lse, what + ' lse')
  for view, storage in views:
    assert_gaps_untouched(storage, view)


def run_backward(case, dt, tuning, layout, dropout=0.0):
  import mmt_amd
  p = problem(case, dt, dropout)
  base = contiguous_backward(case, dt, tuning, dropout)
  lays = _layouts3(layout)
  views = [strided_view(p.t[n], lay, slot=i) for i, (n, lay) in enumerate(zip('qkv', lays))]
  gviews = [strided_view(torch.zeros_like(p.t[n]), lay, slot=i) for i, (n, lay) in enumerate(zip('qkv', lays))]
  qv, kv, vv = (v for v, _ in views)
  out, lse = mmt_amd.relative_attention_forward(qv, kv, vv, p.t['emb'], p.t['bias'], tuning=_tuning(tuning), **p.kw)
  grads = mmt_amd.relative_attention_backward(p.t['dout'], qv, kv, vv, p.t['emb'], p.t['bias'], out, lse,
                                              grads_out=tuple(g for g, _ in gviews), tuning=_tuning(tuning), **p.kw)
  torch.cuda.synchronize()
  what = f'{case}-{dt}-{tuning}-{layout}'
  for got, (g, _) in zip(grads[:3], gviews):      # the kernels wrote the caller's views
    assert got.data_ptr() == g.data_ptr() and got.stride() == g.stride()
  p.check_grads(base, what + ' (contiguous)')
  p.check_grads(grads, what)
  for name, got, want in zip(GRAD_NAMES, grads, base):
    assert_same_bits(got, want, f'{what} {name}')
  for view, storage in gviews + views:
    assert_gaps_untouched(storage, view)


# ---- routes -----------------------------------------------------------------------------------------------------------
# By the selection logic of mmt_api.hip case A in bf16 is eligible for the per-wave, window, plane-walk and
# sliding-window kernels; B takes the lean 2-D path (bf16, table width 64); C (head size 128), E (packed), F (grid) and
# every fp32 call the general kernels; D the dense operator.
FWD_ROUTES = [('A', 'bf16', t) for t in ('0', 'FWD_NO_WIN', 'FWD_FORCE_WIN', 'FWD_FORCE_WIN|FWD_ROWS_ONE_WG', 'FWD_WALK', 'FWD_PWIN')] + \
             [('A', 'f32', '0')] + [(c, dt, '0') for c in 'BCDEF' for dt in ('f32', 'bf16')]
BWD_ROUTES = [('A', 'bf16', t) for t in ('0', 'BWD_NO_HANDOVER', 'BWD_HO_PER_WAVE', 'BWD_NO_PEEL_DQ', 'BWD_NO_PEEL_DKV', 'BWD_DQ_PLANE_MAJOR')] + \
             [('A', 'f32', '0')] + [(c, dt, '0') for c in 'BCDEF' for dt in ('f32', 'bf16')]
# every route: head-major, padded rows, and q / k / v in three different layouts; the remaining layouts on case A bf16
# default, case A fp32 and case C
EVERY_ROUTE = ('head_major', 'padded', MIXED)
REST = tuple(l for l in LAYOUTS if l not in ('contiguous', 'head_major', 'padded'))
FULL = [('A', 'bf16', '0'), ('A', 'f32', '0'), ('C', 'f32', '0'), ('C', 'bf16', '0')]


def _params(routes):
  ps = [(r, l) for r in routes for l in EVERY_ROUTE] + [(r, l) for r in FULL for l in REST]
  return [pytest.param(*r, l, id='-'.join(r) + '-' + l) for r, l in ps]


@pytest.mark.parametrize('case,dt,tuning,layout', _params(FWD_ROUTES))
def test_forward_on_strided_views(case, dt, tuning, layout):
  run_forward(case, dt, tuning, layout)


@pytest.mark.parametrize('case,dt,tuning,layout', _params(BWD_ROUTES))
def test_backward_on_strided_views(case, dt, tuning, layout):
  """`grads_out` are views of the layouts of q, k, v, so that the kernels see the strides on their stores too."""
  run_backward(case, dt, tuning, layout)


@pytest.mark.parametrize('case,dt,tuning', [pytest.param(*r, id='-'.join(r)) for r in FWD_ROUTES])
def test_forward_dropout_on_strided_views(case, dt, tuning):
  run_forward(case, dt, tuning, MIXED, dropout=DROP_P)


@pytest.mark.parametrize('case,dt,tuning', [pytest.param(*r, id='-'.join(r)) for r in BWD_ROUTES])
def test_backward_dropout_on_strided_views(case, dt, tuning):
  run_backward(case, dt, tuning, MIXED, dropout=DROP_P)


# ---- non-contiguous out / dout: reachable through the C entry points only ---------------------------------------------
def _c_call(p, tuning, q, k, v, out, lse, dout=None, grads=None):
  """mmt_attn_fwd (dout None) or mmt_attn_bwd with the descriptor ops._make_desc builds from the tensors' strides."""
  from mmt_amd import _lib, ops
  kw = p.kw
  R = p.t['emb'].shape[0]
  dense = 'att_mask' in kw
  desc = ops._make_desc(q, k, v, out, R, kw.get('pattern'), kw.get('valid_len'), None, -10000.0, False,
                        kw.get('dropout_p', 0.0), kw.get('dropout_seed', 0), _tuning(tuning), kw.get('example_ids'))
  L = _lib.lib()
  ws = torch.empty((max(L.mmt_workspace_bytes(desc), 16),), dtype=torch.uint8, device='cuda')
  ptr = lambda t: None if t is None else t.data_ptr()
  mask, ids = (kw.get('att_mask'), kw.get('relative_att_ids')) if dense else (None, None)
  stream = torch.cuda.current_stream().cuda_stream
  if dout is None:
    _lib.check(L.mmt_attn_fwd(desc, ptr(q), ptr(k), ptr(v), ptr(p.t['emb']), ptr(p.t['bias']), ptr(mask), ptr(ids),
                              ptr(out), ptr(lse), ptr(ws), ws.numel(), stream))
    return None
  dq, dk, dv = grads
  N, D = q.shape[2], q.shape[3]
  de = torch.empty((R, N, D), dtype=torch.float32, device='cuda')
  db = torch.empty((R, N), dtype=torch.float32, device='cuda')
  _lib.check(L.mmt_attn_bwd(desc, ptr(q), ptr(k), ptr(v), ptr(p.t['emb']), ptr(p.t['bias']), ptr(mask), ptr(ids),
                            ptr(out), ptr(dout), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ptr(de), ptr(db), ptr(ws),
                            ws.numel(), stream))
  return dq, dk, dv, de, db


@pytest.mark.parametrize('layout', ['head_major', 'padded'])
@pytest.mark.parametrize('case,dt,tuning', [('A', 'bf16', '0'), ('A', 'bf16', 'FWD_FORCE_WIN'), ('A', 'f32', '0'),
                                            ('D', 'f32', '0'), ('D', 'bf16', '0')],
                         ids=lambda x: x if isinstance(x, str) else None)
def test_strided_out_and_dout_through_the_c_entry_points(case, dt, tuning, layout):
  """`out` (forward: written, backward: read) and `dout` as views of a poisoned storage; q, k, v and the gradients in a
  second layout, so that o_stride differs from the other three."""
  p = problem(case, dt)
  base_out, base_lse = contiguous_forward(case, dt, tuning)
  base = contiguous_backward(case, dt, tuning)
  other = 'padded' if layout == 'head_major' else 'head_major'
  views = [strided_view(p.t[n], other, slot=i) for i, n in enumerate('qkv')]
  gviews = [strided_view(torch.zeros_like(p.t[n]), other, slot=i) for i, n in enumerate('qkv')]
  qv, kv, vv = (v for v, _ in views)
  out, out_storage = strided_view(torch.zeros_like(p.t['q']), layout)
  dout, dout_storage = strided_view(p.t['dout'], layout)
  lse = torch.empty_like(base_lse)
  _c_call(p, tuning, qv, kv, vv, out, lse)
  grads = _c_call(p, tuning, qv, kv, vv, out, lse, dout, tuple(g for g, _ in gviews))
  torch.cuda.synchronize()
  what = f'{case}-{dt}-{tuning}-out:{layout}'
  p.check_forward(out, lse, what)
  assert_same_bits(out, base_out, what + ' out')
  assert_same_bits(lse, base_lse, what + ' lse')
  p.check_grads(grads, what)
  for name, got, want in zip(GRAD_NAMES, grads, base):
    assert_same_bits(got, want, f'{what} {name}')
  for view, storage in gviews + views + [(out, out_storage), (dout, dout_storage)]:
    assert_gaps_untouched(storage, view)


# ---- broadcast inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['broadcast_heads', 'broadcast_batch'])
@pytest.mark.parametrize('case,dt,tuning', [('A', 'bf16', '0'), ('A', 'bf16', 'FWD_FORCE_WIN'), ('A', 'f32', '0'),
                                            ('C', 'bf16', '0'), ('D', 'f32', '0')],
                         ids=lambda x: x if isinstance(x, str) else None)
def test_forward_on_broadcast_k_and_v(case, dt, tuning, layout):
  """stride_n = 0 / stride_b = 0 for k and v: against the oracle fed the expanded arrays, and bit for bit against the
  call on the materialised expansion."""
  import mmt_amd
  p = problem(case, dt, 0.0, layout)
  base_out, base_lse = contiguous_forward(case, dt, tuning, 0.0, layout)
  (kv, ks), (vv, vs) = strided_view(p.t['k'], layout), strided_view(p.t['v'], layout)
  assert 0 in kv.stride() and kv.shape == p.t['k'].shape
  out, lse = mmt_amd.relative_attention_forward(p.t['q'], kv, vv, p.t['emb'], p.t['bias'], tuning=_tuning(tuning), **p.kw)
  torch.cuda.synchronize()
  what = f'{case}-{dt}-{tuning}-{layout}'
  p.check_forward(out, lse, what)
  assert_same_bits(out, base_out, what + ' out')
  assert_same_bits(lse, base_lse, what + ' lse')
  assert_gaps_untouched(ks, kv)
  assert_gaps_untouched(vs, vv)


@pytest.mark.parametrize('axis', [2, 0], ids=['heads', 'batch'])
@pytest.mark.parametrize('case,dt', [('A', 'bf16'), ('A', 'f32'), ('D', 'f32')])
def test_autograd_sums_the_gradient_of_expanded_k_and_v(case, dt, axis):
  """`relative_attention` on `k.expand(...)`: the gradient that reaches the un-expanded leaf is the oracle's dk summed
  over the broadcast axis.  Tolerance: each of the T summed terms carries the gradient bound of the other tests (fp32
  F32_GRAD_TOL absolute; bf16 BF16_GRAD_TOL of max |grad|, the per-term maximum), so T times that."""
  import mmt_amd
  lay = 'broadcast_heads' if axis == 2 else 'broadcast_batch'
  p = problem(case, dt, 0.0, lay)
  sl = (slice(None), slice(None), slice(0, 1)) if axis == 2 else (slice(0, 1),)
  tq = p.t['q'].clone().requires_grad_(True)
  tk, tv = (p.t[n][sl].clone().requires_grad_(True) for n in 'kv')
  out = mmt_amd.relative_attention(tq, tk.expand_as(tq), tv.expand_as(tq), p.t['emb'], p.t['bias'], **p.kw)
  out.backward(p.t['dout'])
  torch.cuda.synchronize()
  p.check_forward(out.detach(), contiguous_forward(case, dt, '0', 0.0, lay)[1], f'{case}-{dt}-{lay}')
  p.check_grads((tq.grad,), f'{case}-{dt}-{lay}', only=('dq',))
  T = tq.shape[axis]
  for name, leaf in (('dk', tk), ('dv', tv)):
    want = p.ref[name].sum(axis=axis, keepdims=True)
    got = leaf.grad.float().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    tol = T * (F32_GRAD_TOL if dt == 'f32' else BF16_GRAD_TOL * max(1.0, np.abs(p.ref[name]).max()))
    err = np.abs(got - want).max()
    print(f'{case}-{dt}-{lay}: {name} summed over {T} terms, max abs err {err:.3e} (tolerance {tol:.3e})')
    assert err < tol, f'{name}: {err}'


# ---- the wrapper's paths (mmt_amd/ops.py) -----------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['head_major', 'qkv_slices', 'padded', 'permuted_dout'])
@pytest.mark.parametrize('case,dt', [('A', 'bf16'), ('A', 'f32'), ('D', 'f32')])
def test_autograd_wrapper_on_views_equals_the_contiguous_call(case, dt, layout):
  """`relative_attention` with q, k, v as views (head-major: dense strides, the backward writes gradients of the same
  strides; fused qkv slices and padded rows: it goes through contiguous copies), and with a non-contiguous dout (the
  consumer permutes `out`): every result bit for bit the all-contiguous call's."""
  import mmt_amd
  p = problem(case, dt)
  base_out, _ = contiguous_forward(case, dt, '0')
  base = contiguous_backward(case, dt, '0')
  lay = 'contiguous' if layout == 'permuted_dout' else layout
  leaves = [strided_view(p.t[n], lay, slot=i)[0].detach().requires_grad_(True) for i, n in enumerate('qkv')]
  te, tb = (p.t[n].clone().requires_grad_(True) for n in ('emb', 'bias'))
  out = mmt_amd.relative_attention(*leaves, te, tb, **p.kw)
  if layout == 'permuted_dout':
    g = p.t['dout'].permute(0, 2, 1, 3).contiguous()         # [B,N,S,D]: what a head-major consumer hands back
    out.permute(0, 2, 1, 3).backward(g)
  else:
    out.backward(p.t['dout'])
  torch.cuda.synchronize()
  assert_same_bits(out.detach(), base_out, 'out')
  for name, leaf, want in zip(('dq', 'dk', 'dv'), leaves, base):
    assert_same_bits(leaf.grad, want, name)
  for name, leaf, want in zip(('drel_emb', 'drel_bias'), (te, tb), base[3:]):
    assert_same_bits(leaf.grad, want.to(leaf.dtype), name)


def test_backward_refuses_grads_out_of_other_strides():
  """`relative_attention_backward(grads_out=...)` writes the caller's buffers or raises: buffers whose strides (or shape
  or dtype) differ from q, k, v are an error, never silently replaced by fresh tensors."""
  import mmt_amd
  p = problem('A', 'bf16')
  t = p.t
  out, lse = contiguous_forward('A', 'bf16', '0')
  base = contiguous_backward('A', 'bf16', '0')
  args = (t['dout'], t['q'], t['k'], t['v'], t['emb'], t['bias'], out, lse)
  good = tuple(torch.zeros_like(t[n]) for n in 'qkv')
  grads = mmt_amd.relative_attention_backward(*args, grads_out=good, **p.kw)
  for got, buf, want in zip(grads, good, base):
    assert got is buf
    assert_same_bits(buf, want, 'grads_out')
  for i in range(3):
    bad = list(torch.zeros_like(t[n]) for n in 'qkv')
    bad[i], storage = strided_view(torch.zeros_like(t['q']), 'head_major')
    with pytest.raises(ValueError, match='grads_out'):
      mmt_amd.relative_attention_backward(*args, grads_out=tuple(bad), **p.kw)
    torch.cuda.synchronize()
    assert not bad[i].any()                                   # and nothing was written
  with pytest.raises(ValueError, match='grads_out'):
    mmt_amd.relative_attention_backward(*args, grads_out=(good[0].float(), good[1], good[2]), **p.kw)


# ---- offsets at the documented limit (bf16) ---------------------------------------------------------------------------
LIMIT_STRIDE_S = (1 << 21) - 8  # 1024 * stride_s = 2 147 475 456 < 2^31 elements: the largest 16-byte-aligned stride the library takes at S = 1000


@pytest.mark.parametrize('operand', ['q', 'k', 'v'])
def test_row_stride_near_the_limit(operand):
  """Case A's pattern, one plane, S = 1000, one of q / k / v (and its gradient) with the largest row stride the library
  takes, 2 097 144 elements, in a NaN-poisoned storage: the byte offsets of real rows pass 2^31, those of the tail rows
  1000 .. 1023 of the last 32-row tile stay just below 2^32 and beyond the descriptor's range.  Forward on the default,
  per-wave, window, plane-walk and sliding-window routes, backward on the default and the recomputing route: finite,
  within the oracle tolerances, bit for bit the contiguous call's, gaps untouched.  The storages span the 1024 rows of
  whole tiles; about 9 GiB of device memory, freed at the end.

  At the limit documented until now (S * stride_s < 2^31: stride_s = 2 147 480) the kernels' own 32-bit products
  `(k0 + 8 * u) * ks1b` of the rows 1001 .. 1023 pass 2^32 and wrap to offsets INSIDE the descriptor's range, 7 296
  bytes in front of rows 1 .. 23: the tail rows read the gap between rows, not zeros, and a NaN there reaches the output
  through P * V although the score is masked.  check_desc therefore counts S in whole tiles and refuses that stride
  (tests/test_c_abi.py holds the boundary); this test sits at the new limit."""
  import mmt_amd
  case, dt = 'A1000', 'bf16'
  p = problem(case, dt)
  S, D = p.cfg['S'], p.cfg['D']
  rows = 32 * ((S + 31) // 32)
  geometry = ((rows * LIMIT_STRIDE_S, LIMIT_STRIDE_S, D), 0, rows * LIMIT_STRIDE_S)
  assert rows * LIMIT_STRIDE_S < 1 << 31 <= rows * (LIMIT_STRIDE_S + 8) and (S - 1) * LIMIT_STRIDE_S * 2 > 1 << 31
  t = dict(p.t)
  view, storage = strided_view(p.t[operand], geometry)
  gview, gstorage = strided_view(torch.zeros_like(p.t[operand]), geometry)
  t[operand] = view
  try:
    for tuning in ('0', 'FWD_NO_WIN', 'FWD_FORCE_WIN', 'FWD_WALK', 'FWD_PWIN'):
      base_out, base_lse = contiguous_forward(case, dt, tuning)
      out, lse = mmt_amd.relative_attention_forward(t['q'], t['k'], t['v'], t['emb'], t['bias'], tuning=_tuning(tuning), **p.kw)
      torch.cuda.synchronize()
      what = f'{operand} at the stride limit, forward {tuning}'
      p.check_forward(out, lse, what)
      assert_same_bits(out, base_out, what + ' out')
      assert_same_bits(lse, base_lse, what + ' lse')
    for tuning in ('0', 'BWD_NO_HANDOVER'):
      base = contiguous_backward(case, dt, tuning)
      out, lse = contiguous_forward(case, dt, tuning)
      gouts = tuple(gview if n == operand else torch.zeros_like(p.t[n]) for n in 'qkv')
      grads = mmt_amd.relative_attention_backward(t['dout'], t['q'], t['k'], t['v'], t['emb'], t['bias'], out, lse,
                                                  grads_out=gouts, tuning=_tuning(tuning), **p.kw)
      torch.cuda.synchronize()
      what = f'{operand} at the stride limit, backward {tuning}'
      p.check_grads(grads, what)
      for name, got, want in zip(GRAD_NAMES, grads, base):
        assert_same_bits(got, want, f'{what} {name}')
      assert_gaps_untouched(gstorage, gview)
    assert_gaps_untouched(storage, view)
  finally:
    del view, storage, gview, gstorage, t
    torch.cuda.empty_cache()


BIG = (1 << 31) + 64            # a batch / head stride beyond 2^31 elements


@pytest.mark.parametrize('which', ['batch', 'head'])
@pytest.mark.parametrize('case', ['A', 'C'])
def test_batch_and_head_strides_beyond_2_31_elements(case, which):
  """q, k, v as views of ONE poisoned storage (about 4.3 GiB), the gradients in a second one: batch stride 2^31 + 64
  elements with B = 2, N = 2, or the head stride at that value with B = 1 (rows then D apart, as in the head-major
  layout).  Forward and backward on the default route of case A and of case C (bf16); the same assertions."""
  import mmt_amd
  dt = 'bf16'
  p = problem(case, dt)
  B, S, N, D = p.t['q'].shape
  sel = slice(None) if which == 'batch' else slice(0, 1)
  if which == 'batch':
    plane = S * N * D + 41 * 8                      # one example's [S,N,D] block, poison after it
    strides = (BIG, N * D, D)
    numel = (B - 1) * BIG + 3 * plane
  else:
    plane = S * D + 41 * 8                          # one head's [S,D] block
    strides = (2 * BIG, D, BIG)
    numel = (N - 1) * BIG + 3 * plane
  kw = dict(p.kw)
  if which == 'head' and kw.get('valid_len') is not None:
    kw['valid_len'] = kw['valid_len'][:1].contiguous()
  try:
    storages = [torch.empty(numel, dtype=torch.bfloat16, device='cuda') for _ in range(2)]
    for s in storages:
      _int_view(s).fill_(0x7FE5)
    shape = (B if which == 'batch' else 1, S, N, D)
    ins, gouts = ([s.as_strided(shape, strides + (1,), i * plane) for i in range(3)] for s in storages)
    cont = [p.t[n][sel].contiguous() for n in 'qkv']
    dout = p.t['dout'][sel].contiguous()
    for view, x in zip(ins, cont):
      view.copy_(x)
    for view in gouts:
      view.zero_()
    for s, views in zip(storages, (ins, gouts)):
      assert_gaps_untouched(s, views)
    base_out, base_lse = mmt_amd.relative_attention_forward(*cont, p.t['emb'], p.t['bias'], **kw)
    base = mmt_amd.relative_attention_backward(dout, *cont, p.t['emb'], p.t['bias'], base_out, base_lse, **kw)
    out, lse = mmt_amd.relative_attention_forward(*ins, p.t['emb'], p.t['bias'], **kw)
    grads = mmt_amd.relative_attention_backward(dout, *ins, p.t['emb'], p.t['bias'], out, lse, grads_out=tuple(gouts), **kw)
    torch.cuda.synchronize()
    what = f'{case}: {which} stride 2^31 + 64'
    if which == 'batch':                            # the whole case: the shared oracle applies
      p.check_forward(out, lse, what)
      p.check_grads(grads, what)
    else:                                           # its first example
      assert torch.isfinite(out.float()).all() and all(torch.isfinite(g.float()).all() for g in grads)
      tol = BF16_TOL
      err = np.abs(out.float().cpu().numpy() - p.ref['out'][:1]).max()
      lerr = np.abs(lse.cpu().numpy() - p.ref['lse'][:1]).max()
      assert err < tol and lerr < tol, (err, lerr)
      for name, g in zip(('dq', 'dk', 'dv'), grads):
        want = p.ref[name][:1]
        e = grad_error(g.float().cpu().numpy(), want, torch.bfloat16)
        assert e < BF16_GRAD_TOL, f'{name}: {e}'
    assert_same_bits(out, base_out, what + ' out')
    assert_same_bits(lse, base_lse, what + ' lse')
    for name, got, want in zip(GRAD_NAMES, grads, base):
      assert_same_bits(got, want, f'{what} {name}')
    for s, views in zip(storages, (ins, gouts)):
      assert_gaps_untouched(s, views)
  finally:
    storages = ins = gouts = grads = None
    torch.cuda.empty_cache()
