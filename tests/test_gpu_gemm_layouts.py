"""Weight-gradient and feed-forward GEMM kernels (csrc/wgrad_gemm.hip, csrc/ffn_gemm.hip) with every operand a column
slice of a wider buffer: the kernels take the callers' row strides, so a gap must neither be read into a result nor
written.  Input gaps hold a quiet NaN (one read poisons the tile), output gaps a recognisable bit pattern that is
compared bit for bit afterwards (tests/_cases.POISON_BITS).

Tolerances are those of tests/test_gpu_fused_layer.py: 2e-5 relative to the largest entry for the weight gradients,
2^-8 |ref| + 2e-3 for the bf16 feed-forward outputs, against fp64 products of the stored operands; where the sums run in
a fixed order the strided call equals the contiguous one bit for bit."""
import numpy as np
import pytest
import torch

from oracle import layer_ops as lo
from tests._cases import _int_view, _poison_int

pytestmark = pytest.mark.gpu


def _sliced(x, width, offset=0):
  """(view, buffer): the 2-D tensor `x` as columns [offset, offset + x.shape[1]) of a poison-filled [rows, width]."""
  rows, cols = x.shape
  buf = torch.empty(rows, width, dtype=x.dtype, device=x.device)
  _int_view(buf).fill_(_poison_int(x.dtype))
  buf[:, offset:offset + cols] = x
  view = buf[:, offset:offset + cols]
  assert view.stride() == (width, 1) and not view.is_contiguous()
  return view, buf


def _gap_untouched(buf, cols, offset=0):
  """Every column of `buf` outside [offset, offset + cols) still holds the poison bits."""
  iv, want = _int_view(buf), _poison_int(buf.dtype)
  return bool((iv[:, :offset] == want).all()) and bool((iv[:, offset + cols:] == want).all())


def _stream():
  return torch.cuda.current_stream().cuda_stream


# ---- dW += dY^T X ------------------------------------------------------------------------------------------------------
# M = 128: the 128-row tile kernel; K = 96: three whole 32-row steps, one K slice (plain read-add-store epilogue);
# K = 152: a ragged last step; K = 512: two K slices -- fp32 slabs + the reduce kernel (which walks dw by ldw) with a
# workspace, float atomics without.
@pytest.mark.parametrize('K', [96, 3 * 49 + 5, 512], ids=['K96', 'K152-ragged', 'K512-split'])
@pytest.mark.parametrize('with_bias', [True, False], ids=['dbias', 'no-dbias'])
@pytest.mark.parametrize('use_ws', [True, False], ids=['workspace', 'atomics'])
def test_wgrad_accumulate_takes_column_slices(K, with_bias, use_ws):
  from mmt_amd import _lib, fused
  M, N = 128, 256
  torch.manual_seed(K + M)
  dy_c = torch.randn(K, M, device='cuda').to(torch.bfloat16)
  x_c = torch.randn(K, N, device='cuda').to(torch.bfloat16)
  dw0 = torch.randn(M, N, device='cuda')
  db0 = torch.randn(M, device='cuda')
  dy, _ = _sliced(dy_c, 384, 128)
  x, _ = _sliced(x_c, 264)
  dw, dw_buf = _sliced(dw0, 260)
  db = db0.clone() if with_bias else None

  def run(dw_, dy_, x_, db_):
    if use_ws:
      assert fused.wgrad_accumulate_(dw_, dy_, x_, db_)
    else:
      _lib.check(_lib.lib().mmt_wgrad_bias_accumulate(dw_.data_ptr(), dw_.stride(0), None if db_ is None else db_.data_ptr(),
                                                      dy_.data_ptr(), dy_.stride(0), x_.data_ptr(), x_.stride(0), M, N, K,
                                                      None, 0, _stream()))
  run(dw, dy, x, db)
  torch.cuda.synchronize()
  assert _gap_untouched(dw_buf, N)
  want = dw0.double() + dy_c.double().t() @ x_c.double()
  err = float((dw.double() - want).abs().max()) / float(want.abs().max())
  assert err < 2e-5, err
  if with_bias:
    want_b = db0.double() + dy_c.double().sum(0)
    err_b = float((db.double() - want_b).abs().max()) / float(want_b.abs().max())
    assert err_b < 2e-5, err_b
  if use_ws or K < 256:                    # slabs summed in slice order, or one slice: the same bits as contiguous
    dw_c, db_c = dw0.clone(), (db0.clone() if with_bias else None)
    run(dw_c, dy_c, x_c, db_c)
    assert torch.equal(dw, dw_c)
    if with_bias:
      assert torch.equal(db, db_c)


def test_wgrad_accumulate_declines_a_stride_it_cannot_load():
  """Row stride 260 (not a multiple of 8 bf16 = 16 bytes): `wgrad_accumulate_` returns False and dw keeps its bits."""
  from mmt_amd import fused
  K, M, N = 96, 128, 256
  torch.manual_seed(1)
  dy = torch.randn(K, M, device='cuda').to(torch.bfloat16)
  x, _ = _sliced(torch.randn(K, N, device='cuda').to(torch.bfloat16), 260)
  dw0 = torch.randn(M, N, device='cuda')
  dw, dw_buf = _sliced(dw0, 260)
  before = dw_buf.clone()
  assert not fused.wgrad_accumulate_(dw, dy, x)
  assert not fused.wgrad_accumulate_(dw, dy, x, torch.zeros(M, device='cuda'))
  torch.cuda.synchronize()
  assert torch.equal(_int_view(dw_buf), _int_view(before))


def _group_problems(K, strided, seed=0):
  """Two 256 x 256 products over K rows (the first with a bias gradient); `strided`: every matrix a column slice."""
  from mmt_amd import _lib
  M = N = 256
  torch.manual_seed(seed)
  probs, keep = (_lib.WgradProblem * 2)(), []
  for i, q in enumerate(probs):
    dy_c = torch.randn(K, M, device='cuda').to(torch.bfloat16)
    x_c = torch.randn(K, N, device='cuda').to(torch.bfloat16)
    dw0 = torch.randn(M, N, device='cuda')
    db0 = torch.randn(M, device='cuda') if i == 0 else None
    if strided:
      dy, _ = _sliced(dy_c, M + 256, 128)
      x, _ = _sliced(x_c, N + 8)
      dw, dw_buf = _sliced(dw0, N + 4)
    else:
      dy, x, dw, dw_buf = dy_c, x_c, dw0.clone(), None
    db = None if db0 is None else db0.clone()
    q.dw, q.ldw, q.dbias = dw.data_ptr(), dw.stride(0), (None if db is None else db.data_ptr())
    q.dy, q.ldy, q.x, q.ldx, q.M, q.N = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), M, N
    keep.append(dict(dy=dy, x=x, dw=dw, dw_buf=dw_buf, db=db, dy_c=dy_c, x_c=x_c, dw0=dw0, db0=db0))
  return probs, keep


def _run_group(probs, K):
  from mmt_amd import _lib
  L = _lib.lib()
  need = L.mmt_wgrad_group_workspace_bytes(2, probs, K)
  ws = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
  _lib.check(L.mmt_wgrad_grouped(2, probs, K, ws.data_ptr(), ws.numel(), _stream()))
  torch.cuda.synchronize()
  return need


# The grouped kernel steps K by 64 rows and refuses any other K (96 among them, see the refusal test below): 128 is the
# smallest K with more than one step; 512 is split into two slices with slabs and the grouped reduce.
@pytest.mark.parametrize('K', [128, 512], ids=['K128-one-slice', 'K512-split'])
def test_wgrad_grouped_takes_column_slices(K):
  from mmt_amd import fused
  probs, keep = _group_problems(K, strided=True)
  need = _run_group(probs, K)
  assert (need > 0) == (K == 512)
  probs_c, keep_c = _group_problems(K, strided=False)
  _run_group(probs_c, K)
  for t, c in zip(keep, keep_c):
    assert _gap_untouched(t['dw_buf'], 256)
    want = t['dw0'].double() + t['dy_c'].double().t() @ t['x_c'].double()
    assert float((t['dw'].double() - want).abs().max()) / float(want.abs().max()) < 2e-5
    assert torch.equal(t['dw'], c['dw'])                              # the contiguous grouped call
    if t['db'] is not None:
      want_b = t['db0'].double() + t['dy_c'].double().sum(0)
      assert float((t['db'].double() - want_b).abs().max()) / float(want_b.abs().max()) < 2e-5
      assert torch.equal(t['db'], c['db'])
    if K == 128:                                                      # one slice: also the single-problem call's bits
      dw1, db1 = t['dw0'].clone(), (None if t['db0'] is None else t['db0'].clone())
      assert fused.wgrad_accumulate_(dw1, t['dy_c'], t['x_c'], db1)
      assert torch.equal(t['dw'], dw1)
      if db1 is not None:
        assert torch.equal(t['db'], db1)


def test_wgrad_grouped_refuses_k_that_is_no_multiple_of_64():
  from mmt_amd import _lib
  L = _lib.lib()
  probs, keep = _group_problems(96, strided=True)
  before = [t['dw_buf'].clone() for t in keep]
  assert L.mmt_wgrad_group_workspace_bytes(2, probs, 96) == 0
  assert L.mmt_wgrad_grouped(2, probs, 96, None, 0, _stream()) != 0
  torch.cuda.synchronize()
  for t, b in zip(keep, before):
    assert torch.equal(_int_view(t['dw_buf']), _int_view(b))


# ---- feed-forward GEMMs with the GELU in the epilogue -------------------------------------------------------------------
def _close(got, ref):
  return bool((np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + 2e-3).all())          # one bf16 rounding


def _ffn_fwd_case():
  M, N, K = 256, 256, 64
  torch.manual_seed(M + N + K)
  x = torch.randn(M, K, device='cuda').to(torch.bfloat16)
  w = (torch.randn(N, K, device='cuda') * (2.0 / np.sqrt(K))).to(torch.bfloat16)
  b = torch.randn(N, device='cuda')
  return M, N, K, x, w, b


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'no-bias'])
def test_ffn_gelu_gemm_takes_column_slices(with_bias):
  from mmt_amd import fused
  M, N, K, x_c, w_c, b = _ffn_fwd_case()
  b = b if with_bias else None
  x, _ = _sliced(x_c, 192, 64)
  w, _ = _sliced(w_c, 72)
  out = fused.ffn_gelu_gemm(x, w, b)
  assert out is not None
  u, g = (t.float().cpu().numpy() for t in out)
  u_ref = x_c.double().cpu().numpy() @ w_c.double().cpu().numpy().T + (0 if b is None else b.double().cpu().numpy())
  assert _close(u, u_ref)
  assert _close(g, lo.gelu_tanh(u.astype(np.float64)))            # gelu of the STORED (rounded) u
  ref = fused.ffn_gelu_gemm(x_c, w_c, b)
  assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
  bad, _ = _sliced(w_c, 68)                                        # row stride 68: not 16-byte rows
  assert fused.ffn_gelu_gemm(x, bad, b) is None


def test_ffn_gelu_gemm_leaves_the_gaps_of_strided_outputs_untouched():
  """C ABI: u and g with row stride N + 8 inside poisoned buffers."""
  from mmt_amd import _lib, fused
  M, N, K, x_c, w_c, b = _ffn_fwd_case()
  x, _ = _sliced(x_c, 192, 64)
  w, _ = _sliced(w_c, 72)
  blank = torch.zeros(M, N, device='cuda', dtype=torch.bfloat16)
  (u, u_buf), (g, g_buf) = _sliced(blank, N + 8), _sliced(blank, N + 8)
  _lib.check(_lib.lib().mmt_ffn_gelu_gemm(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), u.data_ptr(),
                                          u.stride(0), g.data_ptr(), g.stride(0), M, N, K, _stream()))
  torch.cuda.synchronize()
  ref = fused.ffn_gelu_gemm(x_c, w_c, b)
  assert torch.equal(u, ref[0]) and torch.equal(g, ref[1])
  assert _gap_untouched(u_buf, N) and _gap_untouched(g_buf, N)


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'no-bias'])
def test_ffn_dgelu_gemm_takes_column_slices(with_bias):
  from mmt_amd import _lib, fused
  M, N, K = 256, 256, 64
  torch.manual_seed(M + 3 * N + K)
  dy_c = torch.randn(M, K, device='cuda').to(torch.bfloat16)
  w_c = (torch.randn(K, N, device='cuda') * (2.0 / np.sqrt(K))).to(torch.bfloat16)
  u_c = (torch.randn(M, N, device='cuda') * 2).to(torch.bfloat16)
  b = torch.randn(N, device='cuda') if with_bias else None
  dy, _ = _sliced(dy_c, K + 64)
  w, _ = _sliced(w_c, N + 8)
  u, _ = _sliced(u_c, N + 8)
  du = fused.ffn_dgelu_gemm(dy, w, u, b)
  assert du is not None
  z = u_c.double().cpu().numpy() + (0 if b is None else b.double().cpu().numpy())
  ref = (dy_c.double().cpu().numpy() @ w_c.double().cpu().numpy()) * lo.gelu_tanh_grad(z)
  assert _close(du.float().cpu().numpy(), ref)
  assert torch.equal(du, fused.ffn_dgelu_gemm(dy_c, w_c, u_c, b))
  # C ABI: du with row stride N + 8 inside a poisoned buffer
  out, out_buf = _sliced(torch.zeros(M, N, device='cuda', dtype=torch.bfloat16), N + 8)
  _lib.check(_lib.lib().mmt_ffn_dgelu_gemm(dy.data_ptr(), dy.stride(0), w.data_ptr(), w.stride(0), u.data_ptr(), u.stride(0),
                                           None if b is None else b.data_ptr(), out.data_ptr(), out.stride(0), M, N, K,
                                           _stream()))
  torch.cuda.synchronize()
  assert torch.equal(out, du) and _gap_untouched(out_buf, N)
