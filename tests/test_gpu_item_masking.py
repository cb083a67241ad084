"""`mmt_item_masking` on the GPU: the one-launch route of `random_item_masking` against the torch ops of the same process
(`kernel=False`) on the same device tensors, every output bit for bit.  The corner list is tests/_item_masking_cases.py,
which tests/test_item_masking_host.py runs through the host variant; beside it the long rows (config 3's patch row, the
limit) and the fine-tuning batch, where a lane owns more than one position."""
import numpy as np
import pytest
import torch

from tests import _item_masking_cases as MC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('mode', MC.WORD_MODES)
@pytest.mark.parametrize('T', MC.SIZES)
def test_kernel_equals_the_torch_ops(T, mode):
  for name, ins, kw in MC.variants(T, mode, seed=100 + T):
    MC.assert_same(ins, kw, 'cuda', f'T={T} {mode} {name}')


def test_kernel_equals_the_host_variant_and_follows_the_float32_product():
  ins, kw = MC.rounding_case()
  dev = MC.assert_same(ins, kw, 'cuda', 'rounding')
  for d, h in zip(dev, MC.run(ins, kw, 'cpu', True)):
    assert torch.equal(d.cpu(), h)
  ins, kw = MC.base_case(65, 'whole-word', seed=5)
  ins['n_tokens'] = np.array([-1, -(1 << 40), 66, 1 << 40, 1 << 31], np.int64)
  MC.assert_same(ins, kw, 'cuda', 'hostile n_tokens')
  ins['n_tokens'] = np.array([-5, 70, 3, 0, 65], np.int32)
  MC.assert_same(ins, kw, 'cuda', 'int32 n_tokens')


@pytest.mark.parametrize('T', [3971, 8192])
def test_one_long_row(T):
  """A lane owns 4 and 8 consecutive positions; at 8192 the row takes 97 KiB of LDS.  Every token an item (the patch row),
  and whole words."""
  for mode in ('every-token', 'whole-word'):
    ins, kw = MC.base_case(T, mode, seed=T, lengths=[T])
    got = MC.assert_same(ins, dict(kw, selection_rate=0.5, max_selections=T), 'cuda', f'T={T} {mode}')
    assert int(got[2][0]) > T // 8
    ins['item_keys'] = (np.random.default_rng(T).integers(0, 16, ins['item_keys'].shape) / 16).astype(np.float32)
    MC.assert_same(ins, dict(kw, selection_rate=0.15, max_selections=T // 4), 'cuda', f'T={T} {mode} ties')
    # inf, NaN, -0 and +0 among the keys of a long row: the kernel, torch's sort on the GPU at this size and the host variant agree
    rng = np.random.default_rng(T + 1)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 0.25], np.float32)
    pick = rng.random(ins['item_keys'].shape) < 0.7
    ins['item_keys'][pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    got = MC.assert_same(ins, dict(kw, selection_rate=0.6, max_selections=T), 'cuda', f'T={T} {mode} special keys')
    for d, h in zip(got, MC.run(ins, dict(kw, selection_rate=0.6, max_selections=T), 'cpu', True)):
      assert torch.equal(d.cpu(), h)


def test_fine_tuning_batch_with_whole_words():
  rng = np.random.default_rng(64)
  B, T = 64, 256
  ins, kw = MC.base_case(T, 'whole-word', seed=64, lengths=rng.integers(0, T + 1, B))
  got = MC.assert_same(ins, dict(kw, max_selections=12), 'cuda', '[64,256]')
  assert int(got[2].max()) >= 12 and int(got[2].min()) < 12        # (12 items: at least 12 tokens)


def test_limits_fall_back_under_none_and_raise_under_true():
  from mmt_amd import _lib
  ins, kw = MC.base_case(8193, 'whole-word', seed=9, B=2)
  for w, g in zip(MC.run(ins, kw, 'cuda', False), MC.run(ins, kw, 'cuda', None)):
    assert torch.equal(w, g)
  with pytest.raises(_lib.MmtError, match='MMT_MASK_MAX_TOKENS'):
    MC.run(ins, kw, 'cuda', True)
  ins, kw = MC.base_case(64, 'whole-word', seed=9, B=2)
  kw['unselectable_ids'] = list(range(101, 110))
  for w, g in zip(MC.run(ins, kw, 'cuda', False), MC.run(ins, kw, 'cuda', None)):
    assert torch.equal(w, g)
  with pytest.raises(_lib.MmtError, match='MMT_MASK_MAX_UNSELECTABLE'):
    MC.run(ins, kw, 'cuda', True)
  torch.cuda.synchronize()


def test_make_mlm_and_mpp_features_is_the_same_with_the_switch_either_way():
  assert_feature_outputs_equal, feature_outputs = MC.assert_feature_outputs_equal, MC.feature_outputs
  want = feature_outputs('cuda', False)
  assert_feature_outputs_equal(want, feature_outputs('cuda', True))
  assert_feature_outputs_equal(want, feature_outputs('cuda', None))
  assert_feature_outputs_equal([{k: v.cpu() for k, v in o.items()} for o in want], feature_outputs('cpu', False))


@pytest.mark.parametrize('T', [257, 8192])
def test_the_call_records_into_a_graph_and_runs_on_a_side_stream(T):
  """One launch, no allocation inside the library, no host wait: the call replays from a HIP graph on fresh inputs, and on a
  stream of the caller's it orders with that stream's work.  At 8192 the launcher raises the kernel's dynamic-LDS limit
  inside the capture."""
  ins, kw = MC.base_case(T, 'whole-word', seed=77, lengths=[T, T // 3, 0])
  from mmt_amd import feature_pipeline as fp
  t = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in ins.items()}
  call = lambda kernel: fp.random_item_masking(t['token_ids'], t['n_tokens'], kernel=kernel, item_keys=t['item_keys'], value_u=t['value_u'],
                                               random_ids=t['random_ids'], word_start=t['word_start'], **kw)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    call(True)                                                     # warm-up off the capture
  torch.cuda.current_stream().wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    out = call(True)
  t['item_keys'].copy_(torch.rand_like(t['item_keys']))
  g.replay()
  want = call(False)
  for w, o in zip(want, out):
    assert torch.equal(w, o)
