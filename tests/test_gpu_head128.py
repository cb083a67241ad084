"""Head size 128 on the GPU: forward and backward of the general structured kernels and of the dense operator against
the dense oracle (fp32 and bf16), the structured route against the dense operator under dropout, every kernel-selection
switch, strided views of a fused qkv tensor, one config-3-shaped call and a train step of a tiny model.

Tolerances as test_gpu_attention_fwd.py / test_gpu_attention_bwd.py / test_gpu_encoder.py."""
import numpy as np
import pytest
import torch

from oracle import attention as oa
from tests._cases import attention_inputs, bf16_round
from tests.test_gpu_image_grid import grid_side_inputs

pytestmark = pytest.mark.gpu

D = 128
F32_TOL = 1e-3
BF16_TOL = 2e-2
DTYPES = [torch.float32, torch.bfloat16]


def _inputs(B, S, N, R, dtype, seed):
  q, k, v, emb, bias = attention_inputs(B, S, N, R, seed, D=D)
  dout = np.random.default_rng(seed + 100).standard_normal(q.shape).astype(np.float32)
  if dtype == torch.bfloat16:
    q, k, v, dout = (bf16_round(x) for x in (q, k, v, dout))
    emb = None if emb is None else bf16_round(emb)
    bias = None if bias is None else bf16_round(bias)
  return q, k, v, emb, bias, dout


def _pattern(radius, g0, ng, id_mode, m, P, r, a):
  import mmt_amd
  return mmt_amd.AttentionPattern(local_radius=radius, global_start=g0, n_global=ng, id_mode=id_mode, max_dist=m,
                                  patches_per_row=P, core_layers=r, grid_radius=a, grid_start=2 if a else 0)


def run(B, S, N, R, dtype, *, radius=1 << 30, g0=0, ng=0, id_mode=1, m=12, P=0, r=0, a=0, valid=None, seed=0,
        backward=True, tuning=0, dense=False, no_bias=False, scale_before_add=False, accum=False, oracle=True):
  """One D = 128 call (structured pattern, or the dense operator fed the oracle's [B,S,S] side inputs) against the
  dense oracle.  Returns (out, grads) as numpy arrays for comparisons between calls."""
  import mmt_amd
  if R == 0:
    id_mode = 0
  q, k, v, emb, bias, dout = _inputs(B, S, N, R, dtype, seed)
  if no_bias:
    bias = None
  mask, ids = grid_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P or 1, r, a)
  dev = lambda x, dt=dtype: None if x is None else torch.from_numpy(x).cuda().to(dt).contiguous()
  tq, tk, tv, te, tb = (None if x is None else dev(x).requires_grad_(True) for x in (q, k, v, emb, bias))
  vl = None if valid is None else torch.tensor(valid, dtype=torch.int32, device='cuda:0')
  if dense:
    kw = dict(att_mask=torch.from_numpy(mask).cuda(),
              relative_att_ids=None if ids is None else torch.from_numpy(ids).cuda())
  else:
    kw = dict(pattern=_pattern(radius, g0, ng, id_mode, m, P, r, a), valid_len=vl)
  kw.update(tuning=tuning, scale_before_add=scale_before_add)
  seed_grads = {}
  if backward:
    out = mmt_amd.relative_attention(tq, tk, tv, te, tb, **kw)
    if accum and R:                              # MMT_FLAG_ACCUM_REL_GRADS: added onto what the buffers hold
      seed_grads = {'drel_emb': np.full(emb.shape, 0.25, np.float32)}
      if bias is not None:
        seed_grads['drel_bias'] = np.full(bias.shape, -0.5, np.float32)
      demb = torch.from_numpy(seed_grads['drel_emb']).cuda()
      dbias = torch.from_numpy(seed_grads['drel_bias']).cuda() if bias is not None else None
      lse = mmt_amd.relative_attention_forward(tq.detach(), tk.detach(), tv.detach(), te.detach(),
                                               None if tb is None else tb.detach(), **kw)[1]
      mmt_amd.relative_attention_backward(dev(dout), tq.detach(), tk.detach(), tv.detach(), te.detach(),
                                          None if tb is None else tb.detach(), out.detach(), lse,
                                          rel_grads_accum=(demb, dbias), **kw)
    out.backward(dev(dout))
  else:
    out, _ = mmt_amd.relative_attention_forward(tq, tk, tv, te, tb, **kw)
  torch.cuda.synchronize()
  got_out = out.detach().float().cpu().numpy()
  assert got_out.shape == (B, S, N, D)
  grads = {}
  if backward:
    for name, t in (('dq', tq), ('dk', tk), ('dv', tv), ('drel_emb', te), ('drel_bias', tb)):
      if t is not None:
        grads[name] = t.grad.float().cpu().numpy()
    if seed_grads:
      grads['drel_emb'] = demb.cpu().numpy()
      if dbias is not None:
        grads['drel_bias'] = dbias.cpu().numpy()
  if not oracle:
    return got_out, grads
  ref, _ = oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids, scale_after_add=not scale_before_add)
  tol = F32_TOL if dtype == torch.float32 else BF16_TOL
  assert np.isfinite(got_out).all()
  err = np.abs(got_out - ref).max()
  assert err < tol, f'max |out - oracle| = {err}'
  if backward:
    want = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids, scale_after_add=not scale_before_add)
    for name, got in grads.items():
      w = want[name] + seed_grads.get(name, 0.0)
      assert np.isfinite(got).all(), name
      if dtype == torch.float32:
        e = np.abs(got - w).max()
        assert e < 2e-3, f'{name}: max abs err {e}'
      else:
        e = np.abs(got - w).max() / max(1.0, np.abs(w).max())
        assert e < 3e-2, f'{name}: max err relative to max |grad| = {e}'
  return got_out, grads


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
  cfg = dict(radius=24, g0=146, ng=8, id_mode=1, m=12, P=12, r=0, a=0)
  q, k, v, emb, bias, dout = _inputs(B, S, N, R, dtype, seed=7)
  valid = torch.tensor([320, 250], dtype=torch.int32, device='cuda:0')
  pat = _pattern(**cfg)
  si_ = mmt_amd.side_inputs(pat, valid, torch.zeros_like(valid), S, materialize_pattern=True, want_segment_ids=False)
  results = []
  for dense in (False, True):
    ts = [torch.from_numpy(x).cuda().to(dtype).requires_grad_(True) for x in (q, k, v, emb, bias)]
    kw = dict(att_mask=si_['att_mask'], relative_att_ids=si_['relative_att_ids']) if dense else \
        dict(pattern=pat, valid_len=valid)
    out = mmt_amd.relative_attention(*ts, dropout_p=0.1, dropout_seed=1234, **kw)
    out.backward(torch.from_numpy(dout).cuda().to(dtype))
    results.append([out.detach().float()] + [t.grad.float() for t in ts])
  torch.cuda.synchronize()
  for name, a_, b_ in zip(('out', 'dq', 'dk', 'dv', 'drel_emb', 'drel_bias'), *results):
    scale = max(1.0, float(b_.abs().max()))
    err = float((a_ - b_).abs().max()) / scale
    assert err < (2e-3 if dtype == torch.float32 else 3e-2), (name, err)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_head128_every_tuning_bit_gives_the_default_bitwise(dtype):
  """Every switch routes head size 128 to the same general kernels: outputs and gradients equal bit for bit."""
  from mmt_amd import _lib
  bits = {n: getattr(_lib, n) for n in dir(_lib) if n.startswith('MMT_TUNE_')}
  assert bits
  cfg = dict(B=2, S=288, N=2, R=32, m=12, radius=64, g0=146, ng=8, valid=[288, 200])
  base_out, base_grads = run(dtype=dtype, **cfg)
  for name, bit in sorted(bits.items()):
    out, grads = run(dtype=dtype, tuning=bit, oracle=False, **cfg)
    assert np.array_equal(out, base_out), name
    for g in base_grads:
      assert np.array_equal(grads[g], base_grads[g]), (name, g)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_head128_strided_views_of_fused_qkv(dtype):
  import mmt_amd
  B, S, N, R = 2, 200, 2, 32
  q, k, v, emb, bias, dout = _inputs(B, S, N, R, dtype, seed=3)
  qkv = torch.from_numpy(np.stack([q, k, v], axis=2)).cuda().to(dtype).requires_grad_(True)   # [B,S,3,N,128]
  te, tb = (torch.from_numpy(x).cuda().to(dtype).requires_grad_(True) for x in (emb, bias))
  pat = _pattern(radius=32, g0=70, ng=8, id_mode=1, m=12, P=0, r=0, a=0)
  out = mmt_amd.relative_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], te, tb, pattern=pat)
  out.backward(torch.from_numpy(dout).cuda().to(dtype))
  torch.cuda.synchronize()
  from tests._cases import dense_side_inputs
  mask, ids = dense_side_inputs(B, S, None, 32, 70, 8, 1, 12)
  ref, _ = oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids)
  tol = F32_TOL if dtype == torch.float32 else BF16_TOL
  assert np.abs(out.detach().float().cpu().numpy() - ref).max() < tol
  want = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids)
  g = qkv.grad.float().cpu().numpy()
  for i, name in enumerate(('dq', 'dk', 'dv')):
    e = np.abs(g[:, :, i] - want[name]).max() / (1.0 if dtype == torch.float32 else max(1.0, np.abs(want[name]).max()))
    assert e < (2e-3 if dtype == torch.float32 else 3e-2), (name, e)


def test_head128_config3_shape():
  """BASELINE config 3's attention shape at head size 128 (B = 1, S = 4096, N = 6, radius 64, 8 globals, 1-D ids,
  bf16): two heads against the oracle, every head finite."""
  import mmt_amd
  B, S, N, R = 1, 4096, 6, 32
  q, k, v, emb, bias, dout = _inputs(B, S, N, R, torch.bfloat16, seed=11)
  pat = _pattern(radius=64, g0=3971, ng=8, id_mode=1, m=12, P=0, r=0, a=0)
  dev = lambda x: torch.from_numpy(x).cuda().to(torch.bfloat16).requires_grad_(True)
  ts = [dev(x) for x in (q, k, v, emb, bias)]
  out = mmt_amd.relative_attention(*ts, pattern=pat)
  out.backward(torch.from_numpy(dout).cuda().to(torch.bfloat16))
  torch.cuda.synchronize()
  assert torch.isfinite(out).all() and all(torch.isfinite(t.grad).all() for t in ts)
  from tests._cases import dense_side_inputs
  mask, ids = dense_side_inputs(B, S, None, 64, 3971, 8, 1, 12)
  hs = [0, 5]
  sl = lambda x: np.ascontiguousarray(x[:, :, hs])
  ref, _ = oa.relative_attention_fwd(sl(q), sl(k), sl(v), emb[:, hs], bias[:, hs], mask, ids)
  assert np.abs(out.detach().float().cpu().numpy()[:, :, hs] - ref).max() < BF16_TOL
  want = oa.relative_attention_bwd(sl(dout), sl(q), sl(k), sl(v), emb[:, hs], bias[:, hs], mask, ids)
  for name, t in (('dq', ts[0]), ('dk', ts[1]), ('dv', ts[2])):
    got = t.grad.float().cpu().numpy()[:, :, hs]
    assert np.abs(got - want[name]).max() / max(1.0, np.abs(want[name]).max()) < 3e-2, name
  for name, t in (('drel_emb', ts[3]), ('drel_bias', ts[4])):
    got = t.grad.float().cpu().numpy()[:, hs]
    assert np.abs(got - want[name]).max() / max(1.0, np.abs(want[name]).max()) < 3e-2, name


def _head128_experiment():
  from tests.test_gpu_encoder import tiny_experiment
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': {'model': {'encoder': {'mmt': dict(hidden_size=256, num_attention_heads=2)},
                                   'cls_heads': [{'inner_dim': 256, 'num_classes': 2, 'name': 'itm'}]}}})
  return exp


def test_head128_encoder_train_step_against_oracle_autograd():
  import mmt_amd
  from oracle import encoder as oenc
  from tests.test_gpu_encoder import dense_inputs_cpu
  exp = _head128_experiment()
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(1)
  model = task.build_model().cuda()
  assert all(tuple(p.shape)[1:] == (2, 128) for n, p in model.named_parameters() if n.endswith('relative_emb_table'))
  inputs, labels = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2, ragged=True))
  out = model(**inputs, training=False)
  loss = task.build_losses(labels, out)
  loss.backward()
  sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
  cpu_in = dense_inputs_cpu(inputs, exp.task.train_data)
  cpu_lab = {k: v.cpu() for k, v in labels.items()}
  ref_loss = oenc.pretraining_loss(sd, model.encoder.get_config(), cpu_in, cpu_lab)
  ref_loss.backward()
  assert abs(float(loss) - float(ref_loss.detach())) < 1e-3
  for name, p in model.named_parameters():
    want = sd[name].grad
    if want is None:
      assert p.grad is None or float(p.grad.abs().max()) == 0, name
      continue
    got = p.grad.detach().cpu().double()
    err = float((got - want).abs().max()) / max(1e-3, float(want.abs().max()))
    assert err < 2e-3, (name, err)


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
