"""Loss, row, GELU and embedding kernels (csrc/xent.hip, fused_layer.hip, embed.hip) at the shapes where their
dispatch changes: every built tiling, the persistent row loop's second and third trip, the widest instantiations,
strided / misaligned logits, and -inf logits.

References and tolerances are those of tests/test_gpu_fused_layer.py and tests/test_gpu_embed.py: the fp64 numpy
oracle (oracle/layer_ops.py) on bf16-rounded inputs; row kernels 1e-4 (fp32) / 3e-2 (bf16); loss 1e-5 / 2e-5 relative,
loss gradient 1e-6 / one bf16 ulp."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import layer_ops as lo
from tests import test_gpu_embed as embed_base
from tests import test_gpu_fused_layer as layer_base
from tests._cases import bf16_round
from tests._layer_cases import XENT_INF_LABEL_ROW, first_argmax, xent_neg_inf_case

pytestmark = pytest.mark.gpu

DT = layer_base.DT
DT_IDS = ['f32', 'bf16']
XDT = [torch.float32, torch.bfloat16]
_dev = layer_base._dev


# ---- 1. loss kernels ---------------------------------------------------------------------------------------------
def _loss_tol(dtype, want_loss):
  fin = np.abs(want_loss[np.isfinite(want_loss)])
  return (1e-5 if dtype == torch.float32 else 2e-5) * max(1.0, fin.max() if fin.size else 0.0)


def _grad_tol(dtype, want_d):
  return (1e-6 if dtype == torch.float32 else 2.0 ** -8 * max(1e-3, np.abs(want_d).max())) + 1e-7


def _stored(x, dtype):
  """fp32 numpy logits as the device stores them in `dtype` (rounded for bf16; -inf, +inf and NaN survive)."""
  return bf16_round(x) if dtype == torch.bfloat16 else x


def _in_buffer(x, dtype, pad, offset=0, fill=float('inf')):
  """The [rows, C] logits as the column slice [offset, offset + C) of a [rows, C + pad] buffer filled with `fill`
  (a leaf for autograd that keeps the slice's stride and storage offset)."""
  rows, C = x.shape
  buf = torch.full((rows, C + pad), fill, dtype=dtype, device='cuda')
  buf[:, offset:offset + C] = _dev(x, dtype)
  view = buf[:, offset:offset + C].detach()
  assert view.stride() == (C + pad, 1) and view.data_ptr() == buf.data_ptr() + offset * buf.element_size()
  return view.requires_grad_(True)


def _xent_run(logits, labels, coef):
  """(loss, dlogits, argmax) of the fused kernels for a leaf `logits`."""
  from mmt_amd import fused
  lab = torch.from_numpy(labels).cuda()
  loss = fused.softmax_cross_entropy(logits, lab)
  (loss * torch.from_numpy(coef).cuda()).sum().backward()
  with torch.no_grad():
    _, amax = fused.weighted_softmax_cross_entropy(logits.detach(), lab, torch.ones(len(labels), device='cuda'),
                                                   return_argmax=True)
  return loss.detach(), logits.grad, amax


def _assert_xent_matches_oracle(got, x_stored, labels, coef, dtype, inf_rows=()):
  loss, grad, amax = got
  want_loss, want_d = lo.softmax_xent(x_stored, labels)
  want_d = want_d * coef[:, None]
  got_loss = loss.cpu().numpy()
  print('loss', got_loss, 'want', want_loss)
  fin = np.isfinite(want_loss)
  assert fin.sum() == len(labels) - len(inf_rows)
  assert np.isfinite(got_loss[fin]).all(), got_loss
  assert np.abs(got_loss[fin] - want_loss[fin]).max() < _loss_tol(dtype, want_loss)
  for r in inf_rows:
    assert want_loss[r] == np.inf and got_loss[r] == np.inf
  got_d = grad.float().cpu().numpy()
  assert np.isfinite(got_d).all()
  err = np.abs(got_d - want_d).max()
  print('grad err', err, 'tol', _grad_tol(dtype, want_d))
  assert err <= _grad_tol(dtype, want_d)
  assert np.array_equal(amax.cpu().numpy().astype(np.int64), first_argmax(x_stored))


@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
@pytest.mark.parametrize('layout', ['contiguous', 'slice-of-1002'])
def test_xent_neg_inf_logits_count_as_zero_probability(layout, dtype):
  """A -inf logit contributes exp(-inf) = 0: loss, gradient and arg-max of the oracle, +inf loss where the label sits on
  a -inf column.  `slice-of-1002`: even row stride with odd C, so bf16 rows take the 4-byte loads and the odd tail.

  On the kernel before the fix (`OnlineLse::add` computed exp(-inf - -inf) for a thread whose first element is -inf)
  this test fails with NaN losses: rows 0, 1 and 4 of the contiguous logits, rows 0 to 3 of the bf16 slice."""
  x, labels, coef = xent_neg_inf_case()
  xs = _stored(x, dtype)
  logits = _dev(xs, dtype).requires_grad_(True) if layout == 'contiguous' else _in_buffer(xs, dtype, pad=1)
  _assert_xent_matches_oracle(_xent_run(logits, labels, coef), xs, labels, coef, dtype, inf_rows=(XENT_INF_LABEL_ROW,))


@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
def test_xent_nan_logit_poisons_its_own_row_only(dtype):
  from mmt_amd import fused
  x, labels, coef = xent_neg_inf_case(label_on_inf=False)
  x[5, 5] = np.nan
  xs = _stored(x, dtype)
  loss = fused.softmax_cross_entropy(_dev(xs, dtype), torch.from_numpy(labels).cuda()).cpu().numpy()
  want, _ = lo.softmax_xent(xs[:5], labels[:5])
  assert np.isnan(loss[5])
  assert np.isfinite(loss[:5]).all()
  assert np.abs(loss[:5] - want).max() < _loss_tol(dtype, want)


@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
def test_weighted_loss_fused_and_fallback_agree_on_neg_inf_logits(dtype):
  """`layers.weighted_sparse_categorical_crossentropy_loss`: the fused path (GPU tensors) and the F.cross_entropy
  fallback (here: CPU tensors) give the oracle's weighted loss and gradient for -inf logits (tolerances of
  test_weighted_loss_one_launch_matches_oracle)."""
  from mmt_amd import layers
  x, labels, coef = xent_neg_inf_case(label_on_inf=False)
  xs = _stored(x, dtype)
  w = np.abs(coef)
  rows_loss, d_unit = lo.softmax_xent(xs, labels)
  want, wcoef = lo.weighted_loss(rows_loss, w)
  want_d = d_unit * wcoef[:, None]
  for device in ('cuda', 'cpu'):
    lg = torch.from_numpy(xs).to(device).to(dtype).requires_grad_(True)
    loss = layers.weighted_sparse_categorical_crossentropy_loss(lg, torch.from_numpy(labels).to(device),
                                                                torch.from_numpy(w).to(device))
    loss.backward()
    print(device, float(loss.detach()), want)
    assert abs(float(loss.detach()) - want) <= 2e-5 * max(1.0, abs(want)), device
    got_d = lg.grad.float().cpu().numpy()
    tol = 1e-6 if dtype == torch.float32 else 2.0 ** -8 * max(1e-6, np.abs(want_d).max())
    assert np.abs(got_d - want_d).max() <= tol + 1e-9, device


def _strided_case(rows, C, dtype):
  rng = np.random.default_rng(rows * 31 + C)
  x = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
  labels = rng.integers(0, C, size=rows)
  if C == 1001:                       # row maximum and label on the odd last column: the tail decides loss and arg-max
    x[:, C - 1] = np.abs(x).max(-1) + 1.0
    labels[:] = C - 1
    x[1, 400] = x[1, C - 1]           # one tie: the earlier index wins
  coef = (rng.standard_normal(rows) + 2.0).astype(np.float32)
  return _stored(x, dtype), labels, coef


_XENT_REF = {}


def _contiguous_ref(rows, C, dtype):
  """The contiguous run of a strided case: computed once and shared by its layouts."""
  key = (rows, C, dtype)
  if key not in _XENT_REF:
    xs, labels, coef = _strided_case(rows, C, dtype)
    got = _xent_run(_dev(xs, dtype).requires_grad_(True), labels, coef)
    _assert_xent_matches_oracle(got, xs, labels, coef, dtype)
    _XENT_REF[key] = got
  return _XENT_REF[key]


@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
@pytest.mark.parametrize('pad,offset', [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1)],
                         ids=['ld=C+1', 'ld=C+2', 'ld=C+3', 'ld=C+1,base+1', 'ld=C+2,base+1'])
@pytest.mark.parametrize('rows,C', [(5, 1001), (5, 1000), (3, 7)])
def test_xent_row_stride_and_alignment_change_nothing(rows, C, pad, offset, dtype):
  """Logits as a column slice of a wider buffer whose gap columns hold +inf: loss, arg-max and gradient are bit for
  bit those of the contiguous copy (which itself matches the oracle).  bf16: C + pad even and offset 0 is the 4-byte
  load path (with the odd tail for C = 1001 and 7), C + pad odd or offset 1 (a 2-byte-aligned base) the 2-byte loads."""
  xs, labels, coef = _strided_case(rows, C, dtype)
  ref = _contiguous_ref(rows, C, dtype)
  logits = _in_buffer(xs, dtype, pad, offset)
  got = _xent_run(logits, labels, coef)
  assert got[1].is_contiguous()                     # empty_like of a column slice: ldd = C while ld = C + pad
  for name, a, b in zip(('loss', 'grad', 'argmax'), got, ref):
    assert torch.equal(a, b), name


@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
def test_xent_bwd_leaves_the_gap_of_a_strided_gradient_untouched(dtype):
  """C ABI: `mmt_xent_bwd` with ldd = C + 3 into a sentinel-filled buffer -- the gradient columns equal the contiguous
  call's, the three gap columns keep their bits."""
  from mmt_amd import _lib
  L = _lib.lib()
  rows, C = 5, 1001
  xs, labels, coef = _strided_case(rows, C, dtype)
  code = _lib.MMT_F32 if dtype == torch.float32 else _lib.MMT_BF16
  logits, lab = _dev(xs, dtype), torch.from_numpy(labels.astype(np.int32)).cuda()
  loss, lse = torch.empty(rows, device='cuda'), torch.empty(rows, device='cuda')
  cf = torch.from_numpy(coef).cuda()
  st = torch.cuda.current_stream().cuda_stream
  _lib.check(L.mmt_xent_fwd(rows, C, code, logits.data_ptr(), C, lab.data_ptr(), loss.data_ptr(), lse.data_ptr(), st))
  dense = torch.empty(rows, C, dtype=dtype, device='cuda')
  _lib.check(L.mmt_xent_bwd(rows, C, code, logits.data_ptr(), C, lab.data_ptr(), lse.data_ptr(), cf.data_ptr(),
                            dense.data_ptr(), C, st))
  sentinel = -1234.5
  wide = torch.full((rows, C + 3), sentinel, dtype=dtype, device='cuda')
  _lib.check(L.mmt_xent_bwd(rows, C, code, logits.data_ptr(), C, lab.data_ptr(), lse.data_ptr(), cf.data_ptr(),
                            wide.data_ptr(), C + 3, st))
  torch.cuda.synchronize()
  assert torch.equal(wide[:, :C], dense)
  ints = torch.int32 if dtype == torch.float32 else torch.int16
  assert torch.equal(wide[:, C:].contiguous().view(ints), torch.full((rows, 3), sentinel, dtype=dtype, device='cuda').view(ints))
  _, want_d = lo.softmax_xent(xs, labels)
  want_d = want_d * coef[:, None]
  assert np.abs(dense.float().cpu().numpy() - want_d).max() <= _grad_tol(dtype, want_d)
  assert L.mmt_xent_bwd(rows, C, code, logits.data_ptr(), C, lab.data_ptr(), lse.data_ptr(), cf.data_ptr(),
                        wide.data_ptr(), C - 1, st) != 0              # ldd < C is refused


def _row_limit_case(rows):
  rng = np.random.default_rng(rows)
  x = (rng.standard_normal((rows, 3)) * 3).astype(np.float32)
  labels = rng.integers(0, 3, size=rows)
  return x, labels, rng


def test_xent_takes_65535_rows():
  """The backward's grid holds the rows in gridDim.y: 65535 is the most it takes.  Coefficients in [-1, 1]: the
  gradient entries stay below 1 in magnitude, the scale the absolute 1e-6 is meant for."""
  from mmt_amd import fused
  rows = 65535
  x, labels, rng = _row_limit_case(rows)
  coef = rng.uniform(-1.0, 1.0, size=rows).astype(np.float32)
  logits = _dev(x).requires_grad_(True)
  loss = fused.softmax_cross_entropy(logits, torch.from_numpy(labels).cuda())
  (loss * torch.from_numpy(coef).cuda()).sum().backward()
  want_loss, want_d = lo.softmax_xent(x, labels)
  want_d = want_d * coef[:, None]
  assert np.abs(loss.detach().cpu().numpy() - want_loss).max() < _loss_tol(torch.float32, want_loss)
  assert np.abs(logits.grad.cpu().numpy() - want_d).max() <= _grad_tol(torch.float32, want_d)


def test_xent_65536_rows_are_refused_and_the_loss_falls_back():
  from mmt_amd import fused, layers
  rows = 65536
  x, labels, rng = _row_limit_case(rows)
  logits = _dev(x).requires_grad_(True)
  lab = torch.from_numpy(labels).cuda()
  with pytest.raises(ValueError):
    fused.softmax_cross_entropy(logits, lab)
  with pytest.raises(ValueError):
    fused.weighted_softmax_cross_entropy(logits, lab, torch.ones(rows, device='cuda'))
  w = (rng.random(rows) + 0.5).astype(np.float32)
  loss = layers.weighted_sparse_categorical_crossentropy_loss(logits, lab, torch.from_numpy(w).cuda())
  (loss * float(rows)).backward()                       # upstream factor: per-row coefficients of O(1)
  rows_loss, d_unit = lo.softmax_xent(x, labels)
  want, wcoef = lo.weighted_loss(rows_loss, w)
  assert abs(float(loss.detach()) - want) <= 2e-5 * max(1.0, abs(want))
  want_d = d_unit * (wcoef * rows)[:, None]
  assert np.abs(logits.grad.cpu().numpy() - want_d).max() <= _grad_tol(torch.float32, want_d)


# ---- 2. row kernels: every tiling of row_tiling() ------------------------------------------------------------------
# H -> (chunk width W, chunks per lane) and the lanes that are live in the LAST chunk set (of 64); the dead lanes of
# that set hold zeros, which is what keeps them out of the mean, the variance and the column sums:
#     H      W  chunks  live lanes in the last set
#     8      4    1       2
#     248    4    1      62
#     256    4    1      64
#     264    8    1      33
#     512    8    1      64
#     520    4    3       2
#     776    8    2      33
#     1032   8    4       1      (chunk sets 3 and 4 of 4: one lane, none)
#     1536   8    4      64      (chunk set 4 of 4 entirely dead)
#     2056   --   refused (the row no longer fits 4 chunks of 8 per lane)
TILINGS = [(248, '4x1'), (256, '4x1-full'), (264, '8x1'), (512, '8x1-full'), (520, '4x3'), (776, '8x2'), (1032, '8x4'),
           (1536, '8x4-3-of-4-sets')]
TILING_IDS = [f'H{h}-{t}' for h, t in TILINGS]
TILING_ROWS = 9                      # two full blocks of four waves and one lone wave


def _mk(rows, H, seed, dtype, scale=1.0):
  """layer_base._mk with the activations scaled: `scale` = 0.5 keeps millions of bf16 outputs below 8, where one
  bf16 rounding is still inside the 3e-2 the row tests allow."""
  o, x, dxn, dh, bias, gamma, beta = layer_base._mk(rows, H, seed, dtype)
  if scale != 1.0:
    o, x = o * scale, x * scale
    if dtype == torch.bfloat16:
      o, x = bf16_round(o.astype(np.float32)), bf16_round(x.astype(np.float32))
  return o, x, dxn, dh, bias, gamma, beta


def _param(t, preset):
  """fp32 parameter; `preset`: an nn.Parameter whose .grad already holds 0.25 (the kernels then ADD to it)."""
  if preset is None:
    return _dev(t).requires_grad_(True)
  prm = torch.nn.Parameter(_dev(t))
  prm.grad = torch.full_like(prm, preset)
  return prm


def _pgrad(prm, preset):
  g = prm.grad.cpu().numpy().astype(np.float64)
  return g if preset is None else g - preset


def _check_residual_block(rows, H, p, has_ln, dtype, tol, preset=None, scale=1.0):
  """The body of test_gpu_fused_layer.test_residual_block, with optionally preset parameter gradients."""
  from mmt_amd import fused
  o, x, dxn, dh, bias, gamma, beta = _mk(rows, H, rows + H, dtype, scale)
  seed = 0x1234_5678_9ABC + rows
  keep, inv_keep = lo.dropout_keep_mask(rows, H, p, seed) if p else (None, 1.0)
  to, tx = _dev(o, dtype).requires_grad_(True), _dev(x, dtype).requires_grad_(True)
  tb = _param(bias, preset)
  tg = _param(gamma, preset) if has_ln else None
  tbt = _param(beta, preset) if has_ln else None
  x_new, h = fused.residual_block(to, tb, tx, tg, tbt, 1e-12, p, seed)
  want_x, _ = lo.residual_block_fwd(o, bias, x, gamma if has_ln else None, beta, keep, inv_keep)
  got_x = x_new.detach().float().cpu().numpy()
  if p:   # exact mask check: dropped positions are exactly x
    got_keep = got_x != _dev(x, dtype).float().cpu().numpy()
    assert not (got_keep & ~keep).any()         # a dropped position is never modified
    assert (got_keep == keep).mean() > 0.99     # kept positions may round back to x in bf16
    assert abs(keep.mean() - (1 - p)) < 0.02 + 2.0 / np.sqrt(rows * H)
  assert np.abs(got_x - want_x).max() < tol
  loss_terms = [(x_new, _dev(dxn, dtype))]
  if has_ln:
    want_h = lo.layer_norm(got_x.astype(np.float64), gamma, beta)[0]      # LN sees the stored (rounded) x_new
    assert np.abs(h.detach().float().cpu().numpy() - want_h).max() < tol
    loss_terms.append((h, _dev(dh, dtype)))
  sum((a.float() * b.float()).sum() for a, b in loss_terms).backward()
  torch.cuda.synchronize()
  w_do, w_dx, w_db, w_dg, w_dbt = lo.residual_block_bwd(
      dxn.astype(np.float64), dh.astype(np.float64) if has_ln else None, got_x.astype(np.float64),
      gamma if has_ln else None, keep, inv_keep)
  scale_of = lambda w: max(1.0, np.abs(w).max())
  assert np.abs(to.grad.float().cpu().numpy() - w_do).max() / scale_of(w_do) < tol
  assert np.abs(tx.grad.float().cpu().numpy() - w_dx).max() / scale_of(w_dx) < tol
  assert np.abs(_pgrad(tb, preset) - w_db).max() / scale_of(w_db) < tol
  if has_ln:
    assert np.abs(_pgrad(tg, preset) - w_dg).max() / scale_of(w_dg) < tol
    assert np.abs(_pgrad(tbt, preset) - w_dbt).max() / scale_of(w_dbt) < tol


def _check_layer_norm(rows, H, dtype, tol, preset=None):
  """The body of test_gpu_fused_layer.test_layer_norm, with optionally preset parameter gradients."""
  from mmt_amd import fused
  _, x, _, dy, _, gamma, beta = _mk(rows, H, 3 * rows + H, dtype)
  tx = _dev(x, dtype).requires_grad_(True)
  tg, tb = _param(gamma, preset), _param(beta, preset)
  y = fused.layer_norm(tx, tg, tb, 1e-12)
  assert np.abs(y.detach().float().cpu().numpy() - lo.layer_norm(x.astype(np.float64), gamma, beta)[0]).max() < tol
  y.backward(_dev(dy, dtype))
  torch.cuda.synchronize()
  dx, dg, db = lo.layer_norm_bwd(dy.astype(np.float64), x.astype(np.float64), gamma)
  assert np.abs(tx.grad.float().cpu().numpy() - dx).max() < tol * max(1, np.abs(dx).max())
  assert np.abs(_pgrad(tg, preset) - dg).max() < tol * max(1, np.abs(dg).max())
  assert np.abs(_pgrad(tb, preset) - db).max() < tol * max(1, np.abs(db).max())


@pytest.mark.parametrize('dtype,tol', DT, ids=DT_IDS)
@pytest.mark.parametrize('H', [h for h, _ in TILINGS], ids=TILING_IDS)
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('has_ln', [True, False])
def test_residual_block_every_tiling(H, p, has_ln, dtype, tol):
  _check_residual_block(TILING_ROWS, H, p, has_ln, dtype, tol)


@pytest.mark.parametrize('dtype,tol', DT, ids=DT_IDS)
@pytest.mark.parametrize('H', [h for h, _ in TILINGS], ids=TILING_IDS)
def test_layer_norm_every_tiling(H, dtype, tol):
  _check_layer_norm(TILING_ROWS, H, dtype, tol)


def test_row_kernels_refuse_a_row_wider_than_the_widest_tiling():
  from mmt_amd import fused
  from mmt_amd._lib import MmtError
  H = 2056
  x = torch.zeros(4, H, device='cuda')
  ones, zeros = torch.ones(H, device='cuda'), torch.zeros(H, device='cuda')
  with pytest.raises(MmtError):
    fused.layer_norm(x, ones, zeros)
  with pytest.raises(MmtError):
    fused.residual_block(x, zeros, x, ones, zeros)
  with pytest.raises(MmtError):
    fused.residual_block(x, zeros, x)


# ---- persistent loop: 1024 blocks of four waves walk rows 4096 apart ----------------------------------------------
LOOP_ROWS = [4096 + 7, 2 * 4096 + 4 * 300 + 1]
LOOP_IDS = ['2nd-trip-for-7-waves', '3rd-trip-ragged']


@pytest.mark.parametrize('dtype,tol', DT, ids=DT_IDS)
@pytest.mark.parametrize('H', [264, 8], ids=['H264-8x1', 'H8-4x1'])
@pytest.mark.parametrize('rows', LOOP_ROWS, ids=LOOP_IDS)
@pytest.mark.parametrize('has_ln', [True, False])
def test_residual_block_rows_beyond_one_trip(rows, H, has_ln, dtype, tol):
  """More rows than waves in the grid: the forward's prefetch of the next row and the backward's column-sum
  accumulators live across trips.  The parameter gradients are ADDED to preset values."""
  _check_residual_block(rows, H, 0.1, has_ln, dtype, tol, preset=0.25, scale=0.5)


@pytest.mark.parametrize('dtype,tol', DT, ids=DT_IDS)
@pytest.mark.parametrize('H', [264, 8], ids=['H264-8x1', 'H8-4x1'])
@pytest.mark.parametrize('rows', LOOP_ROWS, ids=LOOP_IDS)
def test_layer_norm_rows_beyond_one_trip(rows, H, dtype, tol):
  _check_layer_norm(rows, H, dtype, tol, preset=0.25)


# ---- GELU ----------------------------------------------------------------------------------------------------------
# forward grid: a multiple of nch / gcd(nch, 256) blocks, nch = H / 8.  H = 8184: nch = 1023, unit 1023 (the largest
# odd one); H = 8192: nch = 1024, unit 4, the widest row; H = 136: nch = 17, unit 17 -- with 3 rows fewer chunks than
# threads, with 700 rows every thread runs the four-chunk main loop and the single-chunk tail.
@pytest.mark.parametrize('dtype,tol', DT, ids=DT_IDS)
@pytest.mark.parametrize('rows,H', [(5, 8184), (5, 8192), (3, 136), (700, 136)])
def test_bias_gelu_width_limits(rows, H, dtype, tol):
  layer_base.test_bias_gelu(rows, H, dtype, tol)


def test_bias_gelu_refuses_more_than_8192_columns():
  from mmt_amd import fused
  from mmt_amd._lib import MmtError
  with pytest.raises(MmtError):
    fused.bias_gelu(torch.zeros(2, 8200, device='cuda'), torch.zeros(8200, device='cuda'))


@pytest.mark.parametrize('dtype,tol', DT, ids=DT_IDS)
def test_bias_gelu_saturates_cleanly(dtype, tol):
  """u + bias from -30 to 30: 2^(2a log2 e) overflows to +inf and underflows to 0 long before; the exp2 / rcp form of
  tanh must give exactly +-1 there, in the packed form (the forward's main loop) and the scalar one (its tail, the
  backward).  70 x 512: every forward thread runs four packed rounds and one scalar chunk."""
  from mmt_amd import fused
  rows, H = 70, 512
  rng = np.random.default_rng(30)
  z = np.linspace(-30.0, 30.0, rows * H).astype(np.float32)
  u = rng.permutation(z).reshape(rows, H)
  bias = (rng.standard_normal(H) * 0.5).astype(np.float32)
  u = (u - bias).astype(np.float32)
  dy = rng.standard_normal((rows, H)).astype(np.float32)
  if dtype == torch.bfloat16:
    u, dy = bf16_round(u), bf16_round(dy)
  zz = u.astype(np.float64) + bias
  assert zz.min() < -29.5 and zz.max() > 29.5
  tu, tb = _dev(u, dtype).requires_grad_(True), _dev(bias).requires_grad_(True)
  y = fused.bias_gelu(tu, tb)
  y.backward(_dev(dy, dtype))
  got_y, got_du, got_db = y.detach().float().cpu().numpy(), tu.grad.float().cpu().numpy(), tb.grad.cpu().numpy()
  assert np.isfinite(got_y).all() and np.isfinite(got_du).all() and np.isfinite(got_db).all()
  ref = lo.gelu_tanh(zz)
  assert (np.abs(got_y - ref) / np.maximum(1.0, np.abs(ref))).max() < tol
  du = dy * lo.gelu_tanh_grad(zz)
  assert (np.abs(got_du - du) / np.maximum(1.0, np.abs(du))).max() < tol
  assert np.abs(got_db - du.sum(0)).max() < tol * max(1.0, np.abs(du.sum(0)).max())


# ---- 3. embedding ----------------------------------------------------------------------------------------------------
# H <= 512 / <= 1024 / <= 2048 -> 1 / 2 / 4 chunks of 8 per lane; the 4-chunk kernels are the only ones whose LDS
# slab is 32 KB.  1032: one live lane in chunk set 3, none in 4; 1536: set 4 dead; 2048: every lane live.
@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
@pytest.mark.parametrize('kw', [
    dict(B=2, S=40, H=1032, V=50, Vs=4, n_patch=9),
    dict(B=2, S=40, H=1536, V=50, Vs=4, n_patch=9, repeat_id=0, repeat_n=70, pos=True),      # a run across the 32-cut
    dict(B=2, S=40, H=2048, V=50, Vs=4, n_patch=9),
], ids=['H1032', 'H1536+pos+repeats', 'H2048'])
def test_embed_four_chunks_per_lane(kw, dtype):
  embed_base.test_embed_assemble_matches_oracle(kw, dtype)


def test_embed_refuses_more_than_2048_columns():
  from mmt_amd._lib import MmtError
  c = embed_base.make_case(B=1, S=8, H=2056, V=5, Vs=2, n_patch=0, seed=1)
  with pytest.raises(MmtError):
    embed_base.run_gpu(c, torch.float32)


@pytest.mark.parametrize('dtype', XDT, ids=DT_IDS)
@pytest.mark.parametrize('kw', [
    dict(B=9, S=512, H=64, V=7, Vs=3, n_patch=20, bad_ids=True),       # runs hundreds long: many cuts, across trips
    dict(B=9, S=512, H=64, V=5000, Vs=3, n_patch=20),                  # mostly runs of one
], ids=['V7-long-runs+bad-ids', 'V5000-short-runs'])
def test_embed_rows_beyond_one_trip(kw, dtype):
  """4608 rows on 1024 blocks of four waves: 512 waves take a second row / sorted position (forward, backward and the
  run-summing launch).  The word-table gradient is a fixed-order sum: two runs agree bit for bit."""
  embed_base.test_embed_assemble_matches_oracle(kw, dtype)
  c = embed_base.make_case(seed=11, **kw)
  _, g1 = embed_base.run_gpu(c, dtype, 0.25, 0x1234567890ABCDEF)
  _, g2 = embed_base.run_gpu(c, dtype, 0.25, 0x1234567890ABCDEF)
  for k in ('word_table', 'gamma', 'beta'):
    assert torch.equal(g1[k], g2[k]), k
