"""Image-grid term of the structured pattern (SURVEY.md App. A.5 `grid_radius`) on the GPU: the materialised side
inputs, forward and backward of the general structured kernels against the dense oracle fed
`sparse_pattern_mask(...) | (grid & seg)`, the structured route against the dense operator on the materialised mask
(dropout on), every kernel-selection switch, one head at config 3's shape, and one train step of a tiny model.

Tolerances as test_gpu_attention_fwd.py / test_gpu_attention_bwd.py / test_gpu_encoder.py."""
import numpy as np
import pytest
import torch

from oracle import attention as oa
from oracle import side_inputs as si
from tests._cases import attention_inputs, bf16_round
from tests.test_image_grid_host import grid_mask

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3
BF16_TOL = 2e-2
DTYPES = [torch.float32, torch.bfloat16]


def grid_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P, r, a, g=2, gidx=None):
  """Dense [B,S,S] mask + ids of a grid pattern: the oracle's band / global mask ORed with grid & segmented."""
  valid = valid if valid is not None else [S] * B
  gm = grid_mask(S, g, P, a)
  masks = []
  for vl in valid:
    ex = np.arange(S) < vl
    seg = ex[:, None] == ex[None, :]
    masks.append(si.sparse_pattern_mask(S, vl, min(radius, S), g0, ng, gidx) | (gm & seg))
  mask = np.stack(masks).astype(np.int32)
  ids = None
  if id_mode:
    ids = np.broadcast_to(si.relative_ids_from_desc(S, id_mode, m, P, r), (B, S, S)).astype(np.int32).copy()
  return mask, ids


def _pattern(radius, g0, ng, id_mode, m, P, r, a, g=2):
  import mmt_amd
  return mmt_amd.AttentionPattern(local_radius=radius, global_start=g0, n_global=ng, id_mode=id_mode, max_dist=m,
                                  patches_per_row=P, core_layers=r, grid_radius=a, grid_start=g)


def _inputs(B, S, N, R, dtype, seed):
  q, k, v, emb, bias = attention_inputs(B, S, N, R, seed)
  dout = np.random.default_rng(seed + 100).standard_normal(q.shape).astype(np.float32)
  if dtype == torch.bfloat16:
    q, k, v, dout = (bf16_round(x) for x in (q, k, v, dout))
    emb = None if emb is None else bf16_round(emb)
    bias = None if bias is None else bf16_round(bias)
  return q, k, v, emb, bias, dout


def run_grid(B, S, N, R, dtype, *, a, P, radius=1 << 30, g0=0, ng=0, id_mode=1, m=3, r=0, g=2, valid=None, seed=0,
             backward=True, tuning=0, accum=False, oracle=True):
  """Structured grid call (forward, and backward through autograd) against the dense oracle.  Returns the device
  results (out, grads) for comparisons between calls."""
  import mmt_amd
  if R == 0:
    id_mode = 0
  q, k, v, emb, bias, dout = _inputs(B, S, N, R, dtype, seed)
  dev = lambda x, dt=dtype: None if x is None else torch.from_numpy(x).cuda().to(dt).contiguous()
  tq, tk, tv, te, tb = (None if x is None else dev(x).requires_grad_(True) for x in (q, k, v, emb, bias))
  pat = _pattern(radius, g0, ng, id_mode, m, P, r, a, g)
  vl = None if valid is None else torch.tensor(valid, dtype=torch.int32, device='cuda:0')
  if backward:
    out = mmt_amd.relative_attention(tq, tk, tv, te, tb, pattern=pat, valid_len=vl, tuning=tuning)
    seed_grads = {}
    if accum and R:                              # MMT_FLAG_ACCUM_REL_GRADS: added onto what the buffers hold
      seed_grads = {'drel_emb': np.full(emb.shape, 0.25, np.float32), 'drel_bias': np.full(bias.shape, -0.5, np.float32)}
      demb, dbias = (torch.from_numpy(seed_grads[n]).cuda() for n in ('drel_emb', 'drel_bias'))
      lse = mmt_amd.relative_attention_forward(tq.detach(), tk.detach(), tv.detach(), te.detach(), tb.detach(),
                                               pattern=pat, valid_len=vl, tuning=tuning)[1]
      mmt_amd.relative_attention_backward(dev(dout), tq.detach(), tk.detach(), tv.detach(), te.detach(), tb.detach(),
                                          out.detach(), lse, pattern=pat, valid_len=vl, tuning=tuning,
                                          rel_grads_accum=(demb, dbias))
    out.backward(dev(dout))
  else:
    out, _ = mmt_amd.relative_attention_forward(tq, tk, tv, te, tb, pattern=pat, valid_len=vl, tuning=tuning)
  torch.cuda.synchronize()
  got_out = out.detach().float().cpu().numpy()
  grads = {}
  if backward:
    for name, t in (('dq', tq), ('dk', tk), ('dv', tv), ('drel_emb', te), ('drel_bias', tb)):
      if t is not None:
        grads[name] = t.grad.float().cpu().numpy()
    if accum and R:
      grads['drel_emb'], grads['drel_bias'] = demb.cpu().numpy(), dbias.cpu().numpy()
  if not oracle:
    return got_out, grads
  mask, ids = grid_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P, r, a, g)
  ref, _ = oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids)
  tol = F32_TOL if dtype == torch.float32 else BF16_TOL
  assert np.isfinite(got_out).all()
  err = np.abs(got_out - ref).max()
  assert err < tol, f'max |out - oracle| = {err}'
  if backward:
    want = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids)
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
    # no relative term; P < 32: several image rows per 32-row tile
    dict(B=1, S=96, N=2, R=0, P=8, a=1, radius=4),
    # 1-D ids, 8 global tokens right after the image (2 + 144), ragged, the block 128..159 straddles the image's end
    dict(B=2, S=192, N=2, R=32, m=12, P=12, a=2, radius=8, g0=146, ng=8, valid=[192, 131]),
    # 2-D ids, radius 0 (only the diagonal of the band), a = 3
    dict(B=1, S=200, N=2, R=49, id_mode=2, m=12, P=10, r=2, a=3, radius=0),
    # radius smaller than a, 1-D ids with a vocabulary below 2m + 1 (generic id path)
    dict(B=1, S=64, N=2, R=5, m=3, P=6, a=3, radius=2),
    # P = 40: not a tile multiple; 8 globals after the image, a block straddling its end, ragged
    dict(B=2, S=1700, N=1, R=32, m=12, P=40, a=1, radius=0, g0=1602, ng=8, valid=[1700, 1650]),
    # P = 65 > 64: the grid intervals are disjoint from the band
    dict(B=1, S=4300, N=1, R=32, m=12, P=65, a=2, radius=16),
]
CASE_IDS = ['none-P8', '1d-P12-g8', '2d-P10-r0', 'W<a', 'P40-g8', 'P65']


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('cfg', CASES, ids=CASE_IDS)
def test_grid_forward_against_oracle(cfg, dtype):
  run_grid(dtype=dtype, backward=False, **cfg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('cfg', CASES, ids=CASE_IDS)
def test_grid_backward_against_oracle(cfg, dtype):
  run_grid(dtype=dtype, **cfg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_grid_backward_accumulates_table_gradients(dtype):
  run_grid(dtype=dtype, accum=True, **CASES[1])


@pytest.mark.parametrize('form', ['range', 'listed'])
@pytest.mark.parametrize('id_mode', [1, 2], ids=['1d', '2d'])
def test_side_inputs_materialise_the_grid(form, id_mode):
  """mmt_side_inputs(materialize_pattern = 1) with a grid equals the numpy restatement bit for bit (both branches of
  the kernel: the range through pattern_mask, a listed global set by hand); the ids do not change."""
  import mmt_amd
  B, S, P, m, r, a, radius = 3, 160, 10, 6, 2 if id_mode == 2 else 0, 2, 5
  img = torch.tensor([102, 102, 102], dtype=torch.int32, device='cuda:0')
  txt = torch.tensor([58, 20, 0], dtype=torch.int32, device='cuda:0')
  valid = [160, 122, 102]
  gidx = (0, 50, 103, 140) if form == 'listed' else None
  g0, ng = (102, 6) if form == 'range' else (0, 4)
  pat = mmt_amd.AttentionPattern(local_radius=radius, global_start=g0, n_global=ng, id_mode=id_mode, max_dist=m,
                                 patches_per_row=P, core_layers=r, global_index=gidx, grid_radius=a, grid_start=2)
  got = mmt_amd.side_inputs(pat, img, txt, S, materialize_pattern=True)
  want_mask, want_ids = grid_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P, r, a, 2, gidx)
  assert (got['att_mask'].cpu().numpy() == want_mask).all()
  assert (got['relative_att_ids'].cpu().numpy() == want_ids).all()
  import dataclasses
  plain = mmt_amd.side_inputs(dataclasses.replace(pat, grid_radius=0), img, txt, S, materialize_pattern=True)
  assert torch.equal(plain['relative_att_ids'], got['relative_att_ids'])
  assert torch.equal(plain['segment_ids'], got['segment_ids'])
  assert int((got['att_mask'] - plain['att_mask']).min()) == 0 and int((got['att_mask'] != plain['att_mask']).sum()) > 0


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_structured_grid_equals_dense_operator_under_dropout(dtype):
  """App. A.5's dense-vs-sparse equivalence: the grid call on the structured kernels and the dense operator on the
  materialised mask draw the same keep mask and agree in forward and backward."""
  import mmt_amd
  B, S, N, R = 2, 320, 2, 32
  cfg = dict(radius=6, g0=146, ng=8, id_mode=1, m=12, P=12, r=0, a=1)
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


def _tuning_bits():
  from mmt_amd import _lib
  return {n: getattr(_lib, n) for n in dir(_lib) if n.startswith('MMT_TUNE_')}


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_every_tuning_bit_honours_the_grid(dtype):
  """A tuning bit may change which kernel runs, never whether the grid is honoured: one grid case under each switch
  the existing tests flip gives the oracle's output and gradients, and the same as the defaults."""
  cfg = dict(B=2, S=288, N=2, R=32, m=12, P=12, a=1, radius=16, g0=146, ng=8, valid=[288, 200])
  base_out, base_grads = run_grid(dtype=dtype, **cfg)
  tol = 2e-3 if dtype == torch.float32 else 3e-2
  for name, bit in sorted(_tuning_bits().items()):
    out, grads = run_grid(dtype=dtype, tuning=bit, oracle=False, **cfg)
    assert np.abs(out - base_out).max() < tol, name
    for g in base_grads:
      assert np.abs(grads[g] - base_grads[g]).max() / max(1.0, np.abs(base_grads[g]).max()) < tol, (name, g)


def test_config3_shape_grid_against_oracle():
  """One head at BASELINE config 3's shape (S=4096, P=63, radius 64, 8 globals after the image, 1-D ids m=12, bf16)
  with a = 1: forward and every gradient against the dense fp64 oracle."""
  run_grid(1, 4096, 1, 32, torch.bfloat16, a=1, P=63, radius=64, g0=3971, ng=8, m=12, seed=5)


def test_encoder_train_step_structured_equals_dense_side_inputs():
  """A tiny pretraining model with image_grid_radius = 1: one step on the structured path and one on the dense side
  inputs `synthetic_batch(dense_side_inputs=True)` materialises -- loss, outputs and every parameter gradient agree."""
  import mmt_amd
  from tests.test_gpu_encoder import tiny_experiment
  exp = tiny_experiment(S=256, image=192, radius=8)
  exp.task.train_data.image_grid_radius = 1
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(3)
  model = task.build_model().cuda()
  runs = []
  for dense in (False, True):
    inputs, labels = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2, ragged=True,
                                            dense_side_inputs=dense))
    if not dense:
      pat = inputs['attention_pattern']
      assert (pat.grid_radius, pat.grid_start, pat.patches_per_row) == (1, 2, 12)
    else:
      assert 'attention_pattern' not in inputs and inputs['att_mask'].shape == (2, 256, 256)
    model.zero_grad(set_to_none=True)
    out = model(**inputs, training=False)
    loss = task.build_losses(labels, out)
    loss.backward()
    seq = out['sequence_output'] if isinstance(out, dict) and 'sequence_output' in out else None
    runs.append((float(loss), None if seq is None else seq.detach().float().cpu(),
                 {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}))
  (l0, s0, g0), (l1, s1, g1) = runs
  assert abs(l0 - l1) < 1e-3
  if s0 is not None:
    assert float((s0 - s1).abs().max()) < 1e-3
  assert g0.keys() == g1.keys()
  for name in g0:
    err = float((g0[name] - g1[name]).abs().max()) / max(1e-3, float(g1[name].abs().max()))
    assert err < 2e-3, (name, err)
