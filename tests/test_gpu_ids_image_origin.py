"""2-D relative ids at the image's position (`MMT_IDS_2D_IMAGE`, id_mode 3) on the GPU.

Expected ids are written from the definition (tests/_cases.py: image_origin_ids -- the oracle's 2-D generator for the
image x image block placed at [g, g + P^2), the two part ids across, the 1-D clipped id elsewhere); expected attention
is the dense fp64 oracle fed those ids and the materialised mask.  Ids and masks are bit-exact.  Tolerances are the
standing bars of tests/_cases.py, and test_gpu_encoder.py's for the encoder."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import side_inputs as si
from tests._cases import DTYPES, composed, dense_side_inputs, image_origin_ids, parity_inputs
from tests._parity import (assert_runs_agree, assert_structured_equals_dense_under_dropout, check_against, device_call,
                           make_pattern, oracle_call, tiny_experiment, tuning_bits)

pytestmark = pytest.mark.gpu

DROP_SEED = 4321
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'feature_utils_golden.json')))


def _pattern(id_mode=3, **kw):
  return make_pattern(id_mode=id_mode, **kw)


def _device_ids(pat, S, B=1, **kw):
  import mmt_amd
  dev = torch.device('cuda:0')
  out = mmt_amd.side_inputs(pat, torch.full((B,), S, dtype=torch.int32, device=dev),
                            torch.zeros(B, dtype=torch.int32, device=dev), S, want_segment_ids=False, **kw)
  torch.cuda.synchronize()
  return out


# ---- 1. ids from mmt_side_inputs, bit-exact ------------------------------------------------------------------------
@pytest.mark.parametrize('P,r,m,g,S', [(2, 1, 12, 0, 9), (2, 1, 12, 2, 9), (6, 1, 4, 2, 96), (6, 2, 4, 32, 96),
                                       (6, 1, 4, 45, 96), (8, 2, 12, 2, 128)])
def test_side_inputs_ids_are_the_definition(P, r, m, g, S):
  got = _device_ids(_pattern(m=m, P=P, r=r, g=g), S, B=2)['relative_att_ids'].cpu().numpy()
  want = image_origin_ids(S, m, P, r, g)
  for b in range(2):
    np.testing.assert_array_equal(got[b], want)
  if g == 0:
    two = _device_ids(_pattern(2, m=m, P=P, r=r), S, B=2)['relative_att_ids'].cpu().numpy()
    np.testing.assert_array_equal(got, two)              # origin 0 is MMT_IDS_2D, bit for bit
  else:
    assert (want != si.relative_ids_from_desc(S, 2, m, P, r)).any()


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=lambda c: c['name'])
def test_origin_zero_gives_the_reference_golden_matrices(case):
  S = case['seq_len']
  kw = dict(m=case['text_relative_pos_max_distance'], P=case['num_patch_per_row'], r=case['num_core_layers'])
  got = _device_ids(_pattern(g=0, **kw), S)['relative_att_ids'].cpu().numpy()
  np.testing.assert_array_equal(got, np.array(case['expected']))
  two = _device_ids(_pattern(2, **kw), S)['relative_att_ids'].cpu().numpy()
  np.testing.assert_array_equal(got, two)


# ---- shared runner ---------------------------------------------------------------------------------------------------
def expected_side_inputs(B, S, valid, radius, g0, ng, m, P, r, g, a=0):
  """Dense [B,S,S] mask (band / global / segmented, ORed with grid & segmented when a > 0) and the ids of id_mode 3."""
  return dense_side_inputs(B, S, valid, radius, g0, ng, 3, m, P, r, a=a, g=g)


def drop_kw(dropout):
  return dict(dropout_p=dropout, dropout_seed=DROP_SEED) if dropout else {}


# ---- 2. forward and every gradient against the oracle ----------------------------------------------------------------
# P = 6 (36 image positions), S = 96 (three 32-row tiles): the image ends mid-tile for every g and starts mid-tile for
# g = 2 and 45; the global tokens sit behind the image (8: the peeled path, 12: the split-rows path); R = 49 with
# r = 2, m = 12 as the standing 2-D cases (part ids 69 / 70 >= R contribute 0).
@pytest.mark.parametrize('D', [64, 128], ids=['d64', 'd128'])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('ng', [8, 12], ids=['ng8', 'ng12'])
@pytest.mark.parametrize('radius', [8, 1 << 30], ids=['r8', 'full'])
@pytest.mark.parametrize('g', [2, 32, 45])
def test_forward_and_backward_against_oracle(g, radius, ng, dtype, D):
  B, S, N, R, P, r, m = 2, 96, 2, 49, 6, 2, 12
  valid = [96, 90]
  arrays = parity_inputs(B, S, N, R, dtype, seed=g + ng, D=D)
  mask, ids = expected_side_inputs(B, S, valid, radius, g + P * P, ng, m, P, r, g)
  pat = _pattern(radius=radius, g0=g + P * P, ng=ng, m=m, P=P, r=r, g=g)
  vl = torch.tensor(valid, dtype=torch.int32, device='cuda:0')
  for dropout in (0.0, 0.1):
    ref = oracle_call(arrays, mask, ids, dropout=(dropout, DROP_SEED) if dropout else None)
    for name, bit in [('default', 0)] + sorted(tuning_bits().items()):
      got = device_call(arrays, dtype, pattern=pat, valid_len=vl, tuning=bit, **drop_kw(dropout))
      check_against(got, ref, dtype, f'[{name} p={dropout}]')


# ---- 3. the lean look-up path: all-image tiles with an origin off the tile boundary ---------------------------------
LEAN = dict(S=1152, N=1, R=49, P=32, r=2, m=12, radius=64)      # r = 2: table width 64; the test below runs r = 1 (width 32) too


@pytest.fixture(scope='module')
def lean_case():
  c = LEAN
  arrays = parity_inputs(1, c['S'], c['N'], c['R'], torch.bfloat16, seed=11)
  return arrays


@pytest.mark.parametrize('r', [2, 1], ids=['r2-width64', 'r1-width32'])
def test_lean_lookup_tiles_against_oracle(lean_case, r):
  """P = 32, g = 2, bf16, D = 64: the tiles [32 t, 32 t + 32), t = 1..31, lie wholly inside the image [2, 1026) and take
  the look-up table with grid coordinates formed from position - 2; tiles 0 and 32 hold an end of the image and take
  the general column.  Both table widths of the lean kernels; the dK/dV pass in its three forms."""
  c = dict(LEAN, r=r)
  S, g = c['S'], 2
  assert g % 32 and g + 31 < 32 + 31 and 32 * 31 + 31 < g + c['P'] ** 2 < S     # all-image tiles exist, both ends are mixed
  mask, ids = expected_side_inputs(1, S, None, c['radius'], 0, 0, c['m'], c['P'], c['r'], g)
  ref = oracle_call(lean_case, mask, ids)
  pat = _pattern(radius=c['radius'], m=c['m'], P=c['P'], r=c['r'], g=g)
  from mmt_amd import _lib
  for form, bit in (('handover-window', 0), ('handover-wave', _lib.MMT_TUNE_BWD_HO_PER_WAVE), ('recompute', _lib.MMT_TUNE_BWD_NO_HANDOVER)):
    check_against(device_call(lean_case, torch.bfloat16, pattern=pat, tuning=bit), ref, torch.bfloat16, f'[{form}]')


# ---- 4. structured equals dense --------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_structured_equals_dense_operator_on_materialised_side_inputs(dtype):
  import mmt_amd
  B, S, N, R, P, r, m, g = 2, 96, 2, 49, 6, 2, 12, 2
  arrays = parity_inputs(B, S, N, R, dtype, seed=7)
  valid = torch.tensor([96, 81], dtype=torch.int32, device='cuda:0')
  pat = _pattern(radius=8, g0=g + P * P, ng=8, m=m, P=P, r=r, g=g)
  si_ = mmt_amd.side_inputs(pat, valid, torch.zeros_like(valid), S, materialize_pattern=True, want_segment_ids=False)
  mask, ids = expected_side_inputs(B, S, valid.tolist(), 8, g + P * P, 8, m, P, r, g)
  assert np.array_equal(si_['att_mask'].cpu().numpy(), mask) and np.array_equal(si_['relative_att_ids'].cpu().numpy(), ids)
  assert_structured_equals_dense_under_dropout(      # the output: absolute; the gradients: the oracle cases' bars
      arrays, dtype, dict(pattern=pat, valid_len=valid),
      dict(att_mask=si_['att_mask'], relative_att_ids=si_['relative_att_ids']), seed=DROP_SEED, standing_bars=True)


# ---- 5. g = 0 is MMT_IDS_2D ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['general-f32', 'general-bf16-d128', 'lean'])
def test_origin_zero_equals_mode_2_bitwise(shape, lean_case):
  if shape == 'lean':
    c, dtype, arrays, vl = LEAN, torch.bfloat16, lean_case, None
    kw = dict(radius=c['radius'], g0=1100, ng=8, m=c['m'], P=c['P'], r=c['r'])
  else:
    dtype = torch.float32 if shape == 'general-f32' else torch.bfloat16
    arrays = parity_inputs(2, 96, 2, 49, dtype, seed=3, D=64 if shape == 'general-f32' else 128)
    kw = dict(radius=8, g0=40, ng=8, m=12, P=6, r=2)
    vl = torch.tensor([96, 77], dtype=torch.int32, device='cuda:0')
  a = device_call(arrays, dtype, pattern=_pattern(3, g=0, **kw), valid_len=vl, **drop_kw(0.1))
  b = device_call(arrays, dtype, pattern=_pattern(2, **kw), valid_len=vl, **drop_kw(0.1))
  assert a.keys() == b.keys() and len(b) == 6
  for n in b:
    assert torch.equal(a[n], b[n]), n


# ---- 6. with the grid term: ids and grid read one origin ------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_with_the_grid_term_against_oracle(dtype):
  B, S, N, R, P, r, m, g = 2, 96, 2, 49, 6, 2, 12, 2
  valid = [96, 70]
  arrays = parity_inputs(B, S, N, R, dtype, seed=5)
  mask, ids = expected_side_inputs(B, S, valid, 4, g + P * P, 8, m, P, r, g, a=1)
  assert (mask != expected_side_inputs(B, S, valid, 4, g + P * P, 8, m, P, r, g)[0]).any()      # the grid adds pairs
  pat = _pattern(radius=4, g0=g + P * P, ng=8, m=m, P=P, r=r, g=g, a=1)
  vl = torch.tensor(valid, dtype=torch.int32, device='cuda:0')
  check_against(device_call(arrays, dtype, pattern=pat, valid_len=vl), oracle_call(arrays, mask, ids), dtype)


# ---- 7. packed multimodal rows: every example's image at its own g --------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('radius', [8, 1 << 30], ids=['r8', 'full'])
def test_packed_rows_each_example_sees_its_own_image(radius, dtype):
  import mmt_amd
  S, N, R, P, r, m, g = 128, 2, 49, 6, 2, 12, 2
  lengths = [[50, 70], [77, 45]]                         # second examples start off the tile boundaries; tails of 8 and 6
  ex_ids, starts, _, _ = mmt_amd.packed_example_layout(lengths, [[True, True]] * 2, S)
  mask, rel = composed(lengths, S, radius, 3, m, P, r, g=g)      # every run alone, its image at its own g
  # not what MMT_IDS_2D composes (image at local 0), and not the row-aligned ids either
  assert (rel[0, :50, :50] != si.relative_ids_from_desc(50, 2, m, P, r)).any()
  assert ((rel[0, 50:120, 50:120] != image_origin_ids(S, m, P, r, g)[50:120, 50:120]) & (mask[0, 50:120, 50:120] != 0)).any()
  arrays = parity_inputs(2, S, N, R, dtype, seed=9)
  pat = _pattern(radius=radius, m=m, P=P, r=r, g=g)
  got = device_call(arrays, dtype, pattern=pat, example_ids=ex_ids.cuda(), example_starts=starts.cuda())
  check_against(got, oracle_call(arrays, mask, rel), dtype)


# ---- 8. encoder level -------------------------------------------------------------------------------------------------
def test_encoder_structured_equals_dense_side_inputs():
  """Config-1 shape (L2 / H128 / N2, S = 256 = 2 + 14^2 + 58) with `relative_att_align_image: true`: the encoder with
  the structured pattern and the encoder fed the dense side inputs agree, forward and parameter gradients."""
  import mmt_amd
  from mmt_amd import _lib
  exp = tiny_experiment(S=256, core=2, R=49)
  exp.task.train_data.relative_att_align_image = True
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(3)
  model = task.build_model().cuda()
  runs = []
  for dense in (False, True):
    inputs, labels = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2, ragged=True,
                                            dense_side_inputs=dense))
    if not dense:
      pat = inputs['attention_pattern']
      assert (pat.id_mode, pat.grid_start, pat.patches_per_row, pat.core_layers) == (_lib.MMT_IDS_2D_IMAGE, 2, 14, 2)
    else:
      assert 'attention_pattern' not in inputs
      assert np.array_equal(inputs['relative_att_ids'][0].cpu().numpy(), image_origin_ids(256, 12, 14, 2, 2))
    model.zero_grad(set_to_none=True)
    enc_in = {k: v for k, v in inputs.items() if k not in ('mlm_positions', 'mpp_positions')}
    with torch.no_grad():                                  # the encoder's own output, as test_gpu_encoder.py reads it
      seq = model.encoder(**enc_in, training=False)['sequence_output']
    out = model(**inputs, training=False)
    loss = task.build_losses(labels, out)
    loss.backward()
    runs.append((float(loss.detach()), seq.float().cpu(),
                 {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}))
  assert runs[0][1].shape == (2, 256, 128)
  assert_runs_agree(runs)
