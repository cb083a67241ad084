"""`random_item_masking(kernel=True)` on CPU tensors -- `mmt_item_masking_host`, the functions of csrc/item_masking.h that
the kernel runs, as plain loops -- against `kernel=False`, the torch ops that define it: every output bit for bit.  The
cases are tests/_item_masking_cases.py; tests/test_gpu_item_masking.py runs the same list through the kernel."""
import os

import numpy as np
import pytest
import torch

from tests import _item_masking_cases as MC


@pytest.fixture(scope='module', autouse=True)
def _built():
  from mmt_amd import _lib
  _lib.build()


@pytest.mark.parametrize('mode', MC.WORD_MODES)
@pytest.mark.parametrize('T', MC.SIZES)
def test_host_variant_equals_the_torch_ops(T, mode):
  for name, ins, kw in MC.variants(T, mode, seed=100 + T):
    MC.assert_same(ins, kw, 'cpu', f'T={T} {mode} {name}')


def test_the_cases_reach_their_corners():
  """The list is only worth its name if something is chosen, ties and the special keys decide, and all three values occur."""
  seen = set()
  for name, ins, kw in MC.variants(257, 'whole-word', seed=357):
    masked, positions, n_masked, labels = MC.run(ins, kw, 'cpu', True)
    tok = torch.from_numpy(ins['token_ids'])
    if name in ('plain', 'ties', 'inf-nan-zero', 'thresholds', 'rate-1.0', 'max-below', 'max-above'):
      assert int(n_masked.max()) > 0, name
    if name in ('all-unselectable', 'rate-0.0', 'max-zero'):
      assert int(n_masked.max()) == 0 and torch.equal(masked, tok), name
    assert int(n_masked[0]) == 0                                   # the row with n_tokens 0
    changed = masked != tok
    if bool((masked == MC.MASK).any()):
      seen.add('mask')
    if bool((changed & (masked != MC.MASK)).any()):
      seen.add('random')
    for b in range(tok.shape[0]):
      k = int(n_masked[b])
      p = positions[b, :k].long()
      assert bool((p[1:] > p[:-1]).all()) and not positions[b, k:].any() and not labels[b, k:].any(), name
      assert torch.equal(labels[b, :k], tok[b][p]) and bool((p < int(ins['n_tokens'][b])).all()), name
      if k and not bool(changed[b][p].all()):
        seen.add('kept')
  assert seen == {'mask', 'random', 'kept'}


def test_selection_count_follows_the_float32_product():
  """0.15 at 20 selectable items: float32(0.15) is above 0.15, but 20 times it rounds to 3.0 in float32 and the ceiling is 3
  (4 if the product were kept wider, or rounded up).  One fp32 product, rounded once, as numpy and torch take it."""
  ins, kw = MC.rounding_case()
  _, _, n_masked, _ = MC.assert_same(ins, kw, 'cpu', 'rounding')
  want = np.ceil(ins['n_tokens'].astype(np.float32) * np.float32(0.15)).astype(np.int64)
  assert n_masked.tolist() == want.tolist() and int(n_masked[0]) == 3 and 20 * float(np.float32(0.15)) > 3.0


def test_hostile_n_tokens_are_clamped():
  ins, kw = MC.base_case(65, 'whole-word', seed=5)
  for n in ([-1, -(1 << 40), 66, 1 << 40, 1 << 31], [0, 65, 64, 1, 2]):
    ins['n_tokens'] = np.array(n, np.int64)
    MC.assert_same(ins, kw, 'cpu', f'n_tokens {n}')
  ins['n_tokens'] = np.array([-5, 70, 3, 0, 65], np.int32)
  MC.assert_same(ins, kw, 'cpu', 'int32 n_tokens')


def test_limits_fall_back_under_none_and_raise_under_true():
  from mmt_amd import _lib
  ins, kw = MC.base_case(8193, 'whole-word', seed=9, B=2)
  want = MC.run(ins, kw, 'cpu', False)
  for w, g in zip(want, MC.run(ins, kw, 'cpu', None)):
    assert torch.equal(w, g)
  with pytest.raises(_lib.MmtError, match='MMT_MASK_MAX_TOKENS'):
    MC.run(ins, kw, 'cpu', True)
  ins, kw = MC.base_case(64, 'whole-word', seed=9, B=2)
  kw['unselectable_ids'] = list(range(101, 110))
  want = MC.run(ins, kw, 'cpu', False)
  for w, g in zip(want, MC.run(ins, kw, 'cpu', None)):
    assert torch.equal(w, g)
  with pytest.raises(_lib.MmtError, match='MMT_MASK_MAX_UNSELECTABLE') as e:
    MC.run(ins, kw, 'cpu', True)
  assert e.value.code == -2
  kw['unselectable_ids'] = list(range(101, 109))                 # 8 ids are served
  MC.assert_same(ins, kw, 'cpu', '8 ids')
  ins, kw = MC.base_case(8192, 'whole-word', seed=10, lengths=[8192])       # and so is the longest row
  MC.assert_same(ins, kw, 'cpu', 'T=8192')


# ---- make_mlm_and_mpp_features with the switch either way ----------------------------------------------------------------
def test_make_mlm_and_mpp_features_is_the_same_with_the_switch_either_way():
  want = MC.feature_outputs('cpu', False)
  assert any(int(o['mlm_label_weights'].sum()) > 0 for o in want) and any(int(o['mpp_label_weights'].sum()) > 0 for o in want)
  MC.assert_feature_outputs_equal(want, MC.feature_outputs('cpu', True))
  MC.assert_feature_outputs_equal(want, MC.feature_outputs('cpu', None))


def test_sanitizer_program_of_the_masking_host_stage():
  """`make asan-mask` (csrc/Makefile): the argument checks and mmt_item_masking_host under AddressSanitizer + UBSan, driven
  by a C program with its own main in exact-size heap blocks.  CPU only; nothing is loaded into Python."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  csrc = os.path.join(root, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-mask'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'mask asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
