"""The parity harness itself (tests/_cases.py, tests/_parity.py), without a GPU: on one tiny problem the oracle's own
output and gradients stand in for the device's, and `check_against` must pass on them, fail just above each bar, on a
non-finite value and on a missing or an unexpected tensor; the one side-input builder must equal its terms written out;
`oracle_call` must feed the oracle the keep mask of the documented seed rule."""
import numpy as np
import pytest
import torch

from oracle import attention as oa
from oracle import side_inputs as si
from tests import _cases as tc
from tests._cases import DTYPES, DTYPE_IDS, dense_side_inputs, grid_mask, image_origin_ids, parity_inputs
from tests._parity import ACCUM_SEED, GRAD_NAMES, check_against, oracle_call

B, S, N, R = 1, 40, 1, 9
NAMES = ('out', 'lse') + GRAD_NAMES


@pytest.fixture(scope='module', params=DTYPES, ids=DTYPE_IDS)
def problem(request):
  arrays = parity_inputs(B, S, N, R, request.param, seed=1)
  mask, ids = dense_side_inputs(B, S, [33], 6, 20, 3, 1, 3)
  return request.param, arrays, mask, ids, oracle_call(arrays, mask, ids)


def bar_of(name, want, dtype):
  """The largest error of one element that passes, from the definitions in tests/_cases.py."""
  if name in ('out', 'lse'):
    return tc.out_tol(dtype)
  return tc.grad_tol(dtype) * (1.0 if dtype == torch.float32 else max(1.0, np.abs(want).max()))


def test_the_bars_are_the_standing_ones():
  assert (tc.F32_TOL, tc.BF16_TOL, tc.F32_GRAD_TOL, tc.BF16_GRAD_TOL, tc.F32_PAIR_TOL, tc.BF16_PAIR_TOL) == \
      (1e-3, 2e-2, 2e-3, 3e-2, 2e-3, 3e-2)


def test_inputs_are_seeded_and_rounded(problem):
  dtype, arrays, _, _, ref = problem
  assert [x.shape for x in arrays] == [(B, S, N, 64)] * 3 + [(R, N, 64), (R, N), (B, S, N, 64)]
  assert all(np.array_equal(x, y) for x, y in zip(arrays, parity_inputs(B, S, N, R, dtype, seed=1)))
  if dtype == torch.bfloat16:
    assert all(np.array_equal(x, tc.bf16_round(x)) for x in arrays)
  assert parity_inputs(B, S, N, R, dtype, seed=1, use_bias=False)[4] is None and parity_inputs(B, S, N, 0, dtype, 1)[3] is None
  assert set(ref) == set(NAMES)


def test_oracle_results_pass(problem):
  dtype, _, _, _, ref = problem
  errs = check_against(dict(ref), ref, dtype)
  assert set(errs) == set(NAMES) and max(errs.values()) == 0
  no_lse = {n: x for n, x in ref.items() if n != 'lse'}
  assert set(check_against(no_lse, ref, dtype)) == set(NAMES) - {'lse'}      # the autograd path returns no lse
  check_against({n: torch.from_numpy(np.asarray(x)) for n, x in ref.items()}, ref, dtype)      # tensors or arrays


@pytest.mark.parametrize('name', NAMES)
def test_one_element_above_its_bar_fails_and_below_passes(problem, name):
  dtype, _, _, _, ref = problem
  for factor, passes in ((0.5, True), (1.5, False), (-1.5, False)):
    got = {n: np.array(x, np.float64) for n, x in ref.items()}
    got[name].flat[got[name].size // 2] += factor * bar_of(name, ref[name], dtype)
    if passes:
      check_against(got, ref, dtype)
    else:
      with pytest.raises(AssertionError, match=name):
        check_against(got, ref, dtype)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('name', NAMES)
def test_a_non_finite_value_fails(problem, name, bad):
  dtype, _, _, _, ref = problem
  got = {n: np.array(x, np.float64) for n, x in ref.items()}
  got[name].flat[0] = bad
  with pytest.raises(AssertionError, match='not finite'):
    check_against(got, ref, dtype)


def test_the_compared_set_is_the_expected_set(problem):
  dtype, arrays, mask, ids, ref = problem
  for name in ('out',) + GRAD_NAMES:                           # a tensor the call should have produced is absent
    with pytest.raises(AssertionError, match='compared'):
      check_against({n: x for n, x in ref.items() if n != name}, ref, dtype)
  with pytest.raises(AssertionError, match='compared'):        # a forward-only result against a forward-backward oracle
    check_against({n: ref[n] for n in ('out', 'lse')}, ref, dtype)
  no_bias = oracle_call(arrays[:4] + (None,) + arrays[5:], mask, ids)
  assert set(no_bias) == set(NAMES) - {'drel_bias'}
  check_against(dict(no_bias), no_bias, dtype)
  with pytest.raises(AssertionError, match='compared'):        # the call had no bias, yet a bias gradient came back
    check_against(dict(no_bias, drel_bias=ref['drel_bias']), no_bias, dtype)
  no_table = oracle_call(arrays[:3] + (None, None) + arrays[5:], mask, None)
  assert set(no_table) == set(NAMES) - {'drel_emb', 'drel_bias'}
  forward = oracle_call(arrays, mask, ids, backward=False)
  assert set(forward) == {'out', 'lse'} and np.array_equal(forward['out'], ref['out'])


def test_seed_grads_are_added_to_the_expectation(problem):
  _, _, _, _, ref = problem
  seeded = dict(ref, drel_emb=ref['drel_emb'] + 0.25, drel_bias=ref['drel_bias'] - 0.5)
  assert ACCUM_SEED == {'drel_emb': 0.25, 'drel_bias': -0.5}
  check_against(seeded, ref, torch.float32, seed_grads=ACCUM_SEED)
  with pytest.raises(AssertionError, match='drel_emb'):
    check_against(dict(ref), ref, torch.float32, seed_grads=ACCUM_SEED)
  with pytest.raises(AssertionError, match='drel_emb'):
    check_against(seeded, ref, torch.float32)


def test_scale_before_add_reaches_the_oracle(problem):
  _, arrays, mask, ids, ref = problem
  q, k, v, emb, bias, dout = arrays
  got = oracle_call(arrays, mask, ids, scale_before_add=True)
  assert np.array_equal(got['out'], oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids, scale_after_add=False)[0])
  assert np.array_equal(got['dq'], oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids, scale_after_add=False)['dq'])
  assert not np.array_equal(got['out'], ref['out'])


# ---- the side-input builder against its terms, written out -------------------------------------------------------------
def _seg(valid):
  ex = np.arange(S) < valid
  return ex[:, None] == ex[None, :]


def test_builder_ragged_valid():
  mask, ids = dense_side_inputs(2, S, [S, 23], 5, 30, 4, 0, 0)
  assert ids is None and mask.dtype == np.int32
  for b, vl in enumerate([S, 23]):
    assert np.array_equal(mask[b], si.sparse_pattern_mask(S, vl, 5, 30, 4))
  full, _ = dense_side_inputs(2, S, None, 1 << 30, 0, 0, 0, 0)      # no lengths, a radius beyond the row: everything
  assert full.shape == (2, S, S) and full.all()


def test_builder_example_ids():
  ex_ids = np.stack([np.repeat([1, 2, 0], [17, 15, 8]), np.arange(S) % 2 + 1]).astype(np.int32)
  mask, _ = dense_side_inputs(2, S, None, 4, 10, 3, 0, 0, example_ids=ex_ids)
  for b in range(2):
    assert np.array_equal(mask[b], si.sparse_pattern_mask(S, S, 4, 10, 3) & si.make_segmented_att_mask(ex_ids[b]))
  assert mask[0, 16, 17] == 0 and mask[0, 17, 18] == 1 and mask[1, 0, 1] == 0 and mask[1, 0, 2] == 1


def test_builder_listed_global_set():
  gidx = (3, 4, 21, 39)
  mask, _ = dense_side_inputs(1, S, [31], 2, 0, 0, 0, 0, gidx=gidx)
  assert np.array_equal(mask[0], si.sparse_pattern_mask(S, 31, 2, 0, 0, gidx))
  assert mask[0, 0, 21] == 1 and mask[0, 0, 22] == 0 and mask[0, 0, 39] == 0      # 39 lies beyond the valid length


def test_builder_grid_term():
  P, a, g = 5, 1, 3
  mask, _ = dense_side_inputs(2, S, [S, 20], 1, 30, 2, 0, 0, P, a=a, g=g)
  for b, vl in enumerate([S, 20]):
    assert np.array_equal(mask[b], si.sparse_pattern_mask(S, vl, 1, 30, 2) | (grid_mask(S, g, P, a) & _seg(vl)))
  assert mask[0, g, g + P + 1] == 1 and mask[0, g, g + 2] == 0      # the diagonal neighbour in the image; not two columns on
  assert mask[1, 13, 13 + P] == 1 and mask[1, 16, 16 + P] == 0      # 21 lies beyond the second row's length
  packed = dense_side_inputs(1, S, None, 1, 30, 2, 0, 0, P, a=a, g=g, example_ids=np.repeat([1, 2], [12, 28])[None])[0]
  want = (si.sparse_pattern_mask(S, S, 1, 30, 2) | grid_mask(S, g, P, a)) & si.make_segmented_att_mask(np.repeat([1, 2], [12, 28]))
  assert np.array_equal(packed[0], want) and packed[0, 8, 13] == 0 and mask[0, 8, 13] == 1


@pytest.mark.parametrize('id_mode', [1, 2, 3])
def test_builder_id_modes(id_mode):
  m, P, r, g = 3, 4, 1, 5
  _, ids = dense_side_inputs(2, S, [S, 9], 3, 0, 0, id_mode, m, P, r, g=g)
  want = {1: lambda: si.relative_ids_from_desc(S, 1, m), 2: lambda: si.relative_ids_from_desc(S, 2, m, P, r),
          3: lambda: image_origin_ids(S, m, P, r, g)}[id_mode]()
  assert ids.dtype == np.int32 and ids.shape == (2, S, S)
  assert np.array_equal(ids[0], want) and np.array_equal(ids[1], want)
  if id_mode == 3:                                             # the image block of mode 2, moved to g
    two = si.relative_ids_from_desc(S, 2, m, P, r)
    assert np.array_equal(ids[0, g:g + P * P, g:g + P * P], two[:P * P, :P * P]) and not np.array_equal(ids[0], two)


# ---- dropout: the restated keep mask under the documented seed rule ----------------------------------------------------
@pytest.mark.parametrize('seed,epoch,mixed', [(4321, 0, 4321), (4321, 7, 4328), (2**64 - 3, 5, 2)])
def test_oracle_call_feeds_the_keep_mask_of_the_seed_rule(problem, monkeypatch, seed, epoch, mixed):
  from mmt_amd import step_scalars
  _, arrays, mask, ids, ref = problem
  q, k, v, emb, bias, dout = arrays
  monkeypatch.setattr(step_scalars, 'host_epoch', lambda device=None: epoch)
  got = oracle_call(arrays, mask, ids, dropout=(0.25, seed))
  keep, keep_prob = oa.dropout_keep_mask(B, N, S, 0.25, mixed)
  assert keep.shape == (B, N, S, S) and 0.6 < keep.mean() < 0.9
  out, lse = oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids, keep_mask=keep, keep_prob=keep_prob)
  want = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids, keep_mask=keep, keep_prob=keep_prob)
  assert np.array_equal(got['out'], out) and np.array_equal(got['lse'], lse)
  assert all(np.array_equal(got[n], want[n]) for n in GRAD_NAMES)
  assert not np.array_equal(got['out'], ref['out'])
  if epoch:
    other = oa.dropout_keep_mask(B, N, S, 0.25, seed)[0]
    assert not np.array_equal(other, keep)                     # the epoch enters the mask
  monkeypatch.setattr(step_scalars, 'epoch_ptr', lambda device=None: 1234)      # a device-resident epoch: no host rule
  with pytest.raises(AssertionError):
    oracle_call(arrays, mask, ids, dropout=(0.25, seed))
