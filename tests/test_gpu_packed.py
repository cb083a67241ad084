"""Packed examples on the structured kernels (`example_ids=`, `MMT_FLAG_EXAMPLE_IDS`) on the GPU.

The oracle mask is `sparse_pattern_mask(S, S, radius, g0, ng) & make_segmented_att_mask(ids)` fed to the dense fp64
oracle; tolerances are the standing bars of tests/_cases.py."""
import numpy as np
import pytest
import torch

from tests._cases import DTYPES, dense_side_inputs, grad_error, grad_tol, out_tol, parity_inputs
from tests._parity import (ACCUM_SEED, GRAD_NAMES, assert_structured_equals_dense_under_dropout,
                           assert_train_step_matches_oracle, check_against, device_call, make_pattern, oracle_call,
                           tiny_experiment, tuning_bits)

pytestmark = pytest.mark.gpu


def ids_from_lengths(lengths, S):
  import mmt_amd
  return mmt_amd.example_ids_from_lengths(lengths, S).numpy()


def packed_side_inputs(ids, radius, g0, ng, id_mode, m, P=0, r=0, gidx=None, a=0):
  """Dense [B,S,S] mask + relative ids of a packed pattern: band / global (/ grid) mask, no length, ANDed with the
  segmented mask of the example ids."""
  B, S = ids.shape
  return dense_side_inputs(B, S, None, radius, g0, ng, id_mode, m, P, r, gidx, a, example_ids=ids)


def run_packed(N, R, dtype, *, ids, radius=1 << 30, g0=0, ng=0, id_mode=1, m=3, P=0, r=0, D=64, seed=0, tuning=0,
               accum=False, scale_before_add=False, oracle=True, a=0, gidx=None):
  """Structured call with example ids (forward, backward through autograd) against the dense oracle.  Returns the
  device results for comparisons between calls."""
  if R == 0:
    id_mode = 0
  ids = np.asarray(ids, np.int32)
  B, S = ids.shape
  arrays = parity_inputs(B, S, N, R, dtype, seed, D)
  pat = make_pattern(radius=radius, g0=g0, ng=ng, id_mode=id_mode, m=m, P=P, r=r, a=a, gidx=gidx)
  got = device_call(arrays, dtype, accum=accum, pattern=pat, example_ids=torch.from_numpy(ids).cuda(), tuning=tuning,
                    scale_before_add=scale_before_add)
  if oracle:
    mask, rel = packed_side_inputs(ids, radius, g0, ng, id_mode, m, P, r, gidx, a)
    ref = oracle_call(arrays, mask, rel, scale_before_add=scale_before_add)
    check_against(got, ref, dtype, seed_grads=ACCUM_SEED if accum else None)
  return got


def _alternating(S, period=2):
  return (np.arange(S) % period + 1).astype(np.int32)


CASES = {
    # no relative term, radius 0 (the diagonal only), uneven lengths that are no tile multiples, a padding tail
    'none-r0': dict(N=2, R=0, radius=0, ids=lambda: ids_from_lengths([[13, 50, 20]], 96)),
    # 1-D ids, small radius, S no multiple of 32, 8 globals inside the second example of row 0 and straddling two
    # examples of row 1 (rows packed differently), row 1 with a padding tail
    '1d-r8-g8': dict(N=2, R=32, m=12, radius=8, g0=100, ng=8,
                     ids=lambda: ids_from_lengths([[70, 130, 100], [33, 71, 64, 90]], 300)),
    # 2-D ids, radius >= S: full attention inside each example
    '2d-full': dict(N=2, R=49, id_mode=2, m=12, P=10, r=2, ids=lambda: ids_from_lengths([[101, 60, 39]], 200)),
    # non-contiguous ids [1,2,1,2,...] (row 0) and [1,2,3,1,2,3,...] (row 1): no tile can be left out; a vocabulary
    # below 2m + 1 (the generic id path); globals
    'alternating': dict(N=1, R=5, m=3, radius=5, g0=40, ng=8,
                        ids=lambda: np.stack([_alternating(130), _alternating(130, 3)])),
    # radius >= S with 8 globals, examples that do and do not contain them
    '1d-full-g8': dict(N=2, R=32, m=12, g0=64, ng=8, ids=lambda: ids_from_lengths([[60, 100, 97]], 257)),
    # scale applied before the relative term is added
    'scale-before-add': dict(N=2, R=32, m=12, radius=16, g0=30, ng=8, scale_before_add=True,
                             ids=lambda: ids_from_lengths([[50, 77, 40]], 192)),
    # head size 128
    'd128': dict(N=2, R=32, m=12, radius=16, g0=70, ng=8, D=128, ids=lambda: ids_from_lengths([[64, 51, 45]], 160)),
    'd128-2d': dict(N=1, R=49, id_mode=2, m=12, P=8, r=2, radius=40, D=128, ids=lambda: ids_from_lengths([[90, 38]], 128)),
    # S = 1100: 35 key tiles = 5 chunks of the global rows' partials; the globals live in the second example, so the
    # chunks inside the first and the third example hand the combine EMPTY partials (max = -inf, sum = 0)
    'chunks': dict(N=1, R=32, m=12, radius=32, g0=310, ng=8, ids=lambda: ids_from_lengths([[300, 420, 250]], 1100)),
}


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_packed_forward_and_backward_against_oracle(name, dtype):
  cfg = dict(CASES[name])
  run_packed(dtype=dtype, ids=cfg.pop('ids')(), **cfg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_packed_backward_accumulates_table_gradients(dtype):
  cfg = dict(CASES['1d-r8-g8'])
  run_packed(dtype=dtype, accum=True, ids=cfg.pop('ids')(), **cfg)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('radius,ng', [(16, 8), (1 << 30, 0)], ids=['band-g8', 'full'])
def test_single_breakpoint_equals_valid_len(radius, ng, dtype):
  """The ids of one breakpoint at vl - 1 (1 on [0, vl), 0 after) against the same call with valid_len = vl, on the
  same (general) kernels: fp32 runs them for both calls, and the results are asserted BITWISE equal there -- the visited
  tiles see the same operations in the same order, and a tile the ids leave out would only have added exact zeros.
  In bf16 the valid_len call takes the lean kernels (another summation order), so the standing tolerances apply."""
  import mmt_amd
  B, S, N, R = 2, 300, 2, 32
  vl = [300, 171]
  ids = np.stack([(np.arange(S) < v).astype(np.int32) for v in vl])
  bp = np.zeros((B, S), np.int32)
  bp[np.arange(B), np.array(vl) - 1] = 1
  assert (mmt_amd.example_ids_from_breakpoints(torch.from_numpy(bp)).numpy() == ids).all()
  q, k, v, emb, bias, dout = parity_inputs(B, S, N, R, dtype, seed=3)
  pat = make_pattern(radius=radius, g0=120, ng=ng, id_mode=1, m=12)
  results = []
  for packed in (True, False):
    ts = [torch.from_numpy(x).cuda().to(dtype).requires_grad_(True) for x in (q, k, v, emb, bias)]
    kw = dict(example_ids=torch.from_numpy(ids).cuda()) if packed else \
        dict(valid_len=torch.tensor(vl, dtype=torch.int32, device='cuda:0'))
    out = mmt_amd.relative_attention(*ts, pattern=pat, **kw)
    out.backward(torch.from_numpy(dout).cuda().to(dtype))
    results.append([out.detach().float()] + [t.grad.float() for t in ts])
  torch.cuda.synchronize()
  for name, a_, b_ in zip(('out',) + GRAD_NAMES, *results):
    err = float((a_ - b_).abs().max()) / max(1.0, float(b_.abs().max()))
    print(f'{name}: max |ids - valid_len| = {err:.3e}')
    if dtype == torch.float32:
      assert torch.equal(a_, b_), (name, err)
    else:
      assert err < (out_tol(dtype) if name == 'out' else grad_tol(dtype)), (name, err)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('radius', [64, 1 << 30], ids=['r64', 'full'])
def test_packed_equals_separate_calls(radius, dtype):
  """Four examples of 256 packed into S = 1024 against four S = 256 calls (1-D ids are translation-invariant, so a
  packed example sees the ids it would see alone), output and dq / dk / dv; no globals, no dropout.  The separate
  calls may take other kernels (bf16: the lean ones), so the standing tolerances apply."""
  import mmt_amd
  N, R, L, n = 2, 32, 256, 4
  S = L * n
  q, k, v, emb, bias, dout = parity_inputs(1, S, N, R, dtype, seed=11)
  pat = make_pattern(radius=radius, id_mode=1, m=12)
  cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)
  ts = [cu(x).requires_grad_(True) for x in (q, k, v)]
  ids = torch.from_numpy(ids_from_lengths([[L] * n], S)).cuda()
  out = mmt_amd.relative_attention(*ts, cu(emb), cu(bias), pattern=pat, example_ids=ids)
  out.backward(cu(dout))
  packed = [out.detach().float()] + [t.grad.float() for t in ts]
  for e in range(n):
    sl = slice(e * L, (e + 1) * L)
    te = [cu(x[:, sl]).requires_grad_(True) for x in (q, k, v)]
    o = mmt_amd.relative_attention(*te, cu(emb), cu(bias), pattern=pat)
    o.backward(cu(dout[:, sl]))
    torch.cuda.synchronize()
    for name, a_, b_ in zip(('out', 'dq', 'dk', 'dv'), [x[:, sl] for x in packed], [o.detach().float()] + [t.grad.float() for t in te]):
      a_, b_ = a_.cpu().numpy(), b_.cpu().numpy()
      err = np.abs(a_ - b_).max() if name == 'out' else grad_error(a_, b_, dtype)
      print(f'example {e} {name}: |packed - separate| = {err:.3e}')
      assert err < (out_tol(dtype) if name == 'out' else grad_tol(dtype)), (e, name, err)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_structured_packed_equals_dense_operator_under_dropout(dtype):
  """The packed call on the structured kernels and the dense operator on the materialised mask draw the same keep
  mask (dropout 0.1, same seed) and agree in forward and backward."""
  N, R = 2, 32
  ids = ids_from_lengths([[100, 140, 80], [51, 200, 40]], 320)
  B, S = ids.shape
  cfg = dict(radius=6, g0=146, ng=8, id_mode=1, m=12)
  arrays = parity_inputs(B, S, N, R, dtype, seed=7)
  mask, rel = packed_side_inputs(ids, **cfg)
  assert_structured_equals_dense_under_dropout(
      arrays, dtype, dict(pattern=make_pattern(**cfg), example_ids=torch.from_numpy(ids).cuda()),
      dict(att_mask=torch.from_numpy(mask).cuda(), relative_att_ids=torch.from_numpy(rel).cuda()))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('ng', [0, 8], ids=['g0', 'g8'])
def test_every_tuning_bit_gives_the_bitwise_result_of_the_defaults(ng, dtype):
  """With example ids every lean / window / plane-walk / sliding-window / hand-over path declines: each MMT_TUNE_*
  bit runs the kernels `tuning = 0` runs, bit for bit."""
  cfg = dict(N=2, R=32, m=12, radius=16, g0=146, ng=ng, ids=ids_from_lengths([[100, 120, 68], [288]], 288))
  base = run_packed(dtype=dtype, **cfg)
  for name, bit in sorted(tuning_bits().items()):
    got = run_packed(dtype=dtype, tuning=bit, oracle=False, **cfg)
    assert got.keys() == base.keys()
    for g in base:
      assert torch.equal(got[g], base[g]), (name, g)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('form', ['grid', 'listed'])
def test_grid_or_listed_globals_with_example_ids_take_the_dense_route(form, dtype):
  """Patterns the structured kernels refuse with example ids -- an image grid, a listed global set -- are served
  through the dense operator on the materialised mask ANDed with the ids' segmented mask, and match the oracle."""
  S = 192
  ids = ids_from_lengths([[80, 70, 42], [150, 30]], S)
  if form == 'grid':
    run_packed(2, 32, dtype, ids=ids, radius=4, g0=146, ng=8, m=12, P=12, a=1)
  else:
    gidx = (0, 50, 103, 140)
    run_packed(2, 32, dtype, ids=ids, radius=4, g0=0, ng=4, m=12, gidx=gidx)


def test_config3_shape_packed_against_oracle():
  """One head at BASELINE config 3's shape (S = 4096, radius 64, 8 globals at 3971, 1-D ids m = 12, bf16) packed with
  16 uneven examples: forward and every gradient against the dense fp64 oracle."""
  lengths = [301, 17, 256, 480, 33, 512, 129, 200, 77, 640, 95, 300, 411, 250, 160, 235]
  assert len(lengths) == 16 and sum(lengths) == 4096
  run_packed(1, 32, torch.bfloat16, ids=ids_from_lengths([lengths], 4096), radius=64, g0=3971, ng=8, m=12, seed=5)


def test_tiny_encoder_train_step_with_example_ids_matches_oracle():
  """A tiny pretraining model (2 layers, fused path, radius 32, 8 globals) fed `example_ids` instead of `valid_len`:
  loss and every parameter gradient against the float64 dense CPU oracle fed the dense mask of the same ids."""
  import mmt_amd
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(1)
  model = task.build_model().cuda()
  inputs, labels = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2, ragged=True))
  S = 256
  pat = inputs['attention_pattern']
  # the image part [0, 198) + text to the row's valid length as example one, then two more "examples" in what was padding /
  # text: the attention path only -- what the rows mean to the losses is out of scope here
  vl = inputs.pop('valid_len').cpu().tolist()
  ids = np.stack([ids_from_lengths([[v - 20, 12, S - v + 8 - 5]], S)[0] for v in vl])
  inputs['example_ids'] = torch.from_numpy(ids).cuda()
  out = model(**inputs, training=False)
  loss = task.build_losses(labels, out)
  loss.backward()
  cpu_in = {k: v.detach().cpu() for k, v in inputs.items() if torch.is_tensor(v)}
  mask, rel = packed_side_inputs(ids, pat.local_radius, pat.global_start, pat.n_global, pat.id_mode, pat.max_dist,
                                 pat.patches_per_row, pat.core_layers)
  cpu_in['att_mask'] = torch.from_numpy(mask)
  cpu_in['relative_att_ids'] = torch.from_numpy(rel)
  assert_train_step_matches_oracle(model, loss, cpu_in, labels)
