"""Image-grid term of the structured pattern (SURVEY.md App. A.5 `grid_radius`) on the GPU: the materialised side
inputs, forward and backward of the general structured kernels against the dense oracle fed
`sparse_pattern_mask(...) | (grid & seg)`, the structured route against the dense operator on the materialised mask
(dropout on), every kernel-selection switch, one head at config 3's shape, and one train step of a tiny model.

Tolerances: the standing bars of tests/_cases.py; test_gpu_encoder.py's for the encoder."""
import numpy as np
import pytest
import torch

from tests._cases import DTYPES, dense_side_inputs, grad_tol, parity_inputs
from tests._parity import (ACCUM_SEED, assert_runs_agree, assert_structured_equals_dense_under_dropout, check_against,
                           device_call, make_pattern, oracle_call, tiny_experiment, tuning_bits)

pytestmark = pytest.mark.gpu


def run_grid(B, S, N, R, dtype, *, a, P, radius=1 << 30, g0=0, ng=0, id_mode=1, m=3, r=0, g=2, valid=None, seed=0,
             backward=True, tuning=0, accum=False, oracle=True):
  """Structured grid call (forward, and backward through autograd) against the dense oracle.  Returns the device
  results for comparisons between calls."""
  if R == 0:
    id_mode = 0
  arrays = parity_inputs(B, S, N, R, dtype, seed)
  pat = make_pattern(radius=radius, g0=g0, ng=ng, id_mode=id_mode, m=m, P=P, r=r, a=a, g=g)
  vl = None if valid is None else torch.tensor(valid, dtype=torch.int32, device='cuda:0')
  got = device_call(arrays, dtype, backward=backward, accum=accum, pattern=pat, valid_len=vl, tuning=tuning)
  if not backward:
    del got['lse']                                 # the grid cases compare the output alone
  if oracle:
    mask, ids = dense_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P, r, a=a, g=g)
    ref = oracle_call(arrays, mask, ids, backward=backward)
    check_against(got, ref, dtype, seed_grads=ACCUM_SEED if accum else None)
  return got


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
  want_mask, want_ids = dense_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P, r, gidx, a, 2)
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
  arrays = parity_inputs(B, S, N, R, dtype, seed=7)
  valid = torch.tensor([320, 250], dtype=torch.int32, device='cuda:0')
  pat = make_pattern(radius=6, g0=146, ng=8, id_mode=1, m=12, P=12, r=0, a=1)
  si_ = mmt_amd.side_inputs(pat, valid, torch.zeros_like(valid), S, materialize_pattern=True, want_segment_ids=False)
  assert_structured_equals_dense_under_dropout(arrays, dtype, dict(pattern=pat, valid_len=valid),
                                               dict(att_mask=si_['att_mask'], relative_att_ids=si_['relative_att_ids']))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_every_tuning_bit_honours_the_grid(dtype):
  """A tuning bit may change which kernel runs, never whether the grid is honoured: one grid case under each switch
  the existing tests flip gives the oracle's output and gradients, and the same as the defaults."""
  cfg = dict(B=2, S=288, N=2, R=32, m=12, P=12, a=1, radius=16, g0=146, ng=8, valid=[288, 200])
  base = {n: t.cpu().numpy() for n, t in run_grid(dtype=dtype, **cfg).items()}
  tol = grad_tol(dtype)
  for name, bit in sorted(tuning_bits().items()):
    got = run_grid(dtype=dtype, tuning=bit, oracle=False, **cfg)
    assert got.keys() == base.keys()
    assert np.abs(got['out'].cpu().numpy() - base['out']).max() < tol, name
    for g in base.keys() - {'out'}:
      assert np.abs(got[g].cpu().numpy() - base[g]).max() / max(1.0, np.abs(base[g]).max()) < tol, (name, g)


def test_config3_shape_grid_against_oracle():
  """One head at BASELINE config 3's shape (S=4096, P=63, radius 64, 8 globals after the image, 1-D ids m=12, bf16)
  with a = 1: forward and every gradient against the dense fp64 oracle."""
  run_grid(1, 4096, 1, 32, torch.bfloat16, a=1, P=63, radius=64, g0=3971, ng=8, m=12, seed=5)


def test_encoder_train_step_structured_equals_dense_side_inputs():
  """A tiny pretraining model with image_grid_radius = 1: one step on the structured path and one on the dense side
  inputs `synthetic_batch(dense_side_inputs=True)` materialises -- loss, outputs and every parameter gradient agree."""
  import mmt_amd
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
  assert_runs_agree(runs)
