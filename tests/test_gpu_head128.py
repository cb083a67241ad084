"""Head size 128 on the GPU: forward and backward of the general structured kernels and of the dense operator against
the dense oracle (fp32 and bf16), the structured route against the dense operator under dropout, every kernel-selection
switch, strided views of a fused qkv tensor, one config-3-shaped call and a train step of a tiny model.

Tolerances: the standing bars of tests/_cases.py; test_gpu_encoder.py's for the encoder."""
import numpy as np
import pytest
import torch

from oracle import attention as oa
from tests._cases import BF16_GRAD_TOL, BF16_TOL, DTYPES, dense_side_inputs, grad_error, grad_tol, out_tol, parity_inputs
from tests._parity import (ACCUM_SEED, assert_structured_equals_dense_under_dropout, assert_train_step_matches_oracle,
                           check_against, dense_inputs_cpu, device_call, make_pattern, oracle_call, tiny_experiment, to_dev,
                           tuning_bits)

pytestmark = pytest.mark.gpu

D = 128


def _pattern(radius, g0, ng, id_mode, m, P, r, a):
  return make_pattern(radius=radius, g0=g0, ng=ng, id_mode=id_mode, m=m, P=P, r=r, a=a, g=2 if a else 0)


def run(B, S, N, R, dtype, *, radius=1 << 30, g0=0, ng=0, id_mode=1, m=12, P=0, r=0, a=0, valid=None, seed=0,
        tuning=0, dense=False, no_bias=False, scale_before_add=False, accum=False, oracle=True):
  """One D = 128 call (structured pattern, or the dense operator fed the oracle's [B,S,S] side inputs), forward and
  backward through autograd, against the dense oracle.  Returns the device results for comparisons between calls."""
  if R == 0:
    id_mode = 0
  arrays = parity_inputs(B, S, N, R, dtype, seed, D=D, use_bias=not no_bias)
  mask, ids = dense_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P or 1, r, a=a)
  if dense:
    kw = dict(att_mask=to_dev(mask, torch.int32), relative_att_ids=to_dev(ids, torch.int32))
  else:
    vl = None if valid is None else torch.tensor(valid, dtype=torch.int32, device='cuda:0')
    kw = dict(pattern=_pattern(radius, g0, ng, id_mode, m, P, r, a), valid_len=vl)
  got = device_call(arrays, dtype, accum=accum, tuning=tuning, scale_before_add=scale_before_add, **kw)
  assert got['out'].shape == (B, S, N, D)
  if oracle:
    ref = oracle_call(arrays, mask, ids, scale_before_add=scale_before_add)
    check_against(got, ref, dtype, seed_grads=ACCUM_SEED if accum else None)
  return got


CASES = [
    # full attention, no relative term
    dict(B=1, S=160, N=2, R=0),
    # 1-D ids with the permuted table (R >= 2m + 1), band + 8 globals not at position 0, ragged, S = 200
    dict(B=2, S=200, N=2, R=32, m=12, radius=32, g0=70, ng=8, valid=[200, 131]),
    # 1-D ids, generic (R < 2m + 1), band only
    dict(B=1, S=192, N=2, R=9, m=12, radius=16),
    # 2-D ids, Rp = 64
    dict(B=1, S=256, N=2, R=49, id_mode=2, m=12, P=12, r=2, radius=24, g0=144, ng=8),
    # 2-D ids with more core layers: 65-128 ids (Rp = 128, the dQ pass's staged tile)
    dict(B=2, S=288, N=1, R=100, id_mode=2, m=12, P=12, r=4, radius=40, g0=150, ng=8, valid=[288, 250]),
    # band + 8 globals with split row / key items at S = 512, radius 64
    dict(B=1, S=512, N=2, R=32, m=12, radius=64, g0=0, ng=8),
    # image grid, a = 1 and a = 2
    dict(B=1, S=200, N=2, R=32, m=12, P=12, a=1, radius=8, g0=146, ng=8),
    dict(B=1, S=160, N=1, R=49, id_mode=2, m=12, P=10, r=2, a=2, radius=4),
]
CASE_IDS = ['full-R0', '1d-perm-g8-ragged', '1d-generic', '2d-Rp64', '2d-Rp128', 'split-S512', 'grid-a1', 'grid-a2']


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('cfg', CASES, ids=CASE_IDS)
def test_head128_forward_backward_against_oracle(cfg, dtype):
  run(dtype=dtype, **cfg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('cfg', [CASES[1], CASES[4]], ids=['1d', '2d-Rp128'])
def test_head128_dense_operator_against_oracle(cfg, dtype):
  run(dtype=dtype, dense=True, **cfg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_head128_flags_and_no_bias(dtype):
  run(dtype=dtype, scale_before_add=True, accum=True, **CASES[1])
  run(dtype=dtype, no_bias=True, **CASES[3])


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_head128_structured_equals_dense_operator_under_dropout(dtype):
  import mmt_amd
  B, S, N, R = 2, 320, 2, 32
  arrays = parity_inputs(B, S, N, R, dtype, seed=7, D=D)
  valid = torch.tensor([320, 250], dtype=torch.int32, device='cuda:0')
  pat = _pattern(radius=24, g0=146, ng=8, id_mode=1, m=12, P=12, r=0, a=0)
  si_ = mmt_amd.side_inputs(pat, valid, torch.zeros_like(valid), S, materialize_pattern=True, want_segment_ids=False)
  assert_structured_equals_dense_under_dropout(arrays, dtype, dict(pattern=pat, valid_len=valid),
                                               dict(att_mask=si_['att_mask'], relative_att_ids=si_['relative_att_ids']))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_head128_every_tuning_bit_gives_the_default_bitwise(dtype):
  """Every switch routes head size 128 to the same general kernels: outputs and gradients equal bit for bit."""
  bits = tuning_bits()
  assert bits
  cfg = dict(B=2, S=288, N=2, R=32, m=12, radius=64, g0=146, ng=8, valid=[288, 200])
  base = run(dtype=dtype, **cfg)
  for name, bit in sorted(bits.items()):
    got = run(dtype=dtype, tuning=bit, oracle=False, **cfg)
    assert got.keys() == base.keys()
    for g in base:
      assert torch.equal(got[g], base[g]), (name, g)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_head128_strided_views_of_fused_qkv(dtype):
  import mmt_amd
  B, S, N, R = 2, 200, 2, 32
  q, k, v, emb, bias, dout = parity_inputs(B, S, N, R, dtype, seed=3, D=D)
  qkv = torch.from_numpy(np.stack([q, k, v], axis=2)).cuda().to(dtype).requires_grad_(True)   # [B,S,3,N,128]
  te, tb = (torch.from_numpy(x).cuda().to(dtype).requires_grad_(True) for x in (emb, bias))
  pat = _pattern(radius=32, g0=70, ng=8, id_mode=1, m=12, P=0, r=0, a=0)
  out = mmt_amd.relative_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], te, tb, pattern=pat)
  out.backward(torch.from_numpy(dout).cuda().to(dtype))
  torch.cuda.synchronize()
  mask, ids = dense_side_inputs(B, S, None, 32, 70, 8, 1, 12)
  ref, _ = oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids)
  assert np.abs(out.detach().float().cpu().numpy() - ref).max() < out_tol(dtype)
  want = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids)
  g = qkv.grad.float().cpu().numpy()
  for i, name in enumerate(('dq', 'dk', 'dv')):
    e = grad_error(g[:, :, i], want[name], dtype)
    assert e < grad_tol(dtype), (name, e)


def test_head128_config3_shape():
  """BASELINE config 3's attention shape at head size 128 (B = 1, S = 4096, N = 6, radius 64, 8 globals, 1-D ids,
  bf16): two heads against the oracle, every head finite."""
  import mmt_amd
  B, S, N, R = 1, 4096, 6, 32
  q, k, v, emb, bias, dout = parity_inputs(B, S, N, R, torch.bfloat16, seed=11, D=D)
  pat = _pattern(radius=64, g0=3971, ng=8, id_mode=1, m=12, P=0, r=0, a=0)
  dev = lambda x: torch.from_numpy(x).cuda().to(torch.bfloat16).requires_grad_(True)
  ts = [dev(x) for x in (q, k, v, emb, bias)]
  out = mmt_amd.relative_attention(*ts, pattern=pat)
  out.backward(torch.from_numpy(dout).cuda().to(torch.bfloat16))
  torch.cuda.synchronize()
  assert torch.isfinite(out).all() and all(torch.isfinite(t.grad).all() for t in ts)
  mask, ids = dense_side_inputs(B, S, None, 64, 3971, 8, 1, 12)
  hs = [0, 5]
  sl = lambda x: np.ascontiguousarray(x[:, :, hs])
  ref, _ = oa.relative_attention_fwd(sl(q), sl(k), sl(v), emb[:, hs], bias[:, hs], mask, ids)
  assert np.abs(out.detach().float().cpu().numpy()[:, :, hs] - ref).max() < BF16_TOL
  want = oa.relative_attention_bwd(sl(dout), sl(q), sl(k), sl(v), emb[:, hs], bias[:, hs], mask, ids)
  for name, t in (('dq', ts[0]), ('dk', ts[1]), ('dv', ts[2])):
    got = t.grad.float().cpu().numpy()[:, :, hs]
    assert np.abs(got - want[name]).max() / max(1.0, np.abs(want[name]).max()) < BF16_GRAD_TOL, name
  for name, t in (('drel_emb', ts[3]), ('drel_bias', ts[4])):
    got = t.grad.float().cpu().numpy()[:, hs]
    assert np.abs(got - want[name]).max() / max(1.0, np.abs(want[name]).max()) < BF16_GRAD_TOL, name


def _head128_experiment():
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': {'model': {'encoder': {'mmt': dict(hidden_size=256, num_attention_heads=2)},
                                   'cls_heads': [{'inner_dim': 256, 'num_classes': 2, 'name': 'itm'}]}}})
  return exp


def test_head128_encoder_train_step_against_oracle_autograd():
  import mmt_amd
  exp = _head128_experiment()
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(1)
  model = task.build_model().cuda()
  assert all(tuple(p.shape)[1:] == (2, 128) for n, p in model.named_parameters() if n.endswith('relative_emb_table'))
  inputs, labels = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2, ragged=True))
  out = model(**inputs, training=False)
  loss = task.build_losses(labels, out)
  loss.backward()
  assert_train_step_matches_oracle(model, loss, dense_inputs_cpu(inputs, exp.task.train_data), labels)


def test_head128_graphed_train_step_equals_eager():
  """The train step of a hidden-size-256, two-head model replayed as a HIP graph (mmt_amd/graphed.py) against the
  eager step: identical losses and parameters after two steps each way."""
  import bench
  from mmt_amd import benchmarks
  cfg = dict(bench.config3(), S=256, P=14, B=2, g0=2 + 14 * 14, ng=8, D=128, N=2, H=256)
  res = {}
  for graph in (False, True):
    step = benchmarks.make_train_step_bench(cfg, torch.device('cuda:0'), 0, 1, dtype=torch.bfloat16, graph=graph)[0]
    losses = [float(step()['loss']) for _ in range(2)]
    params = torch.cat([s['param'] for s in step.optimizer.slabs])
    res[graph] = (losses, params.clone())
    step.close()
  assert all(np.isfinite(res[False][0]))
  assert res[False][0] == res[True][0]
  assert torch.equal(res[False][1], res[True][1])
