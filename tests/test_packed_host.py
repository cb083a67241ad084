"""Packed examples (`MMT_FLAG_EXAMPLE_IDS`, the `example_ids=` keyword), host side: the flag and the ABI it must not
move, the library's argument errors (no GPU needed), the two id helpers against the reference's formula
(`cumsum(long_breakpoints, reverse=True)` + `make_segmented_att_mask`, src/data/data_utils.py:305-332) and the
Python-side argument checks."""
import ctypes
import re

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (sets sys.path)
from oracle import side_inputs as si


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


def _desc(lib, S=256):
  d = lib.AttnDesc()
  d.B, d.S, d.N, d.D, d.R = 1, S, 1, 64, 32
  d.dtype = lib.MMT_BF16
  for arr in (d.q_stride, d.k_stride, d.v_stride, d.o_stride):
    arr[:] = (S * 64, 64, 64)
  d.scale, d.mask_value = 0.125, -10000.0
  d.mask.local_radius, d.mask.id_mode, d.mask.max_dist = 16, lib.MMT_IDS_1D, 12
  return d


def test_flag_value_matches_the_header(lib):
  header = open(__graft_entry__.ROOT + '/include/mmt_attn.h').read()
  m = re.search(r'#define MMT_FLAG_EXAMPLE_IDS (\d+)u', header)
  assert m and int(m.group(1)) == lib.MMT_FLAG_EXAMPLE_IDS == 4
  flags = [lib.MMT_FLAG_SCALE_BEFORE_ADD, lib.MMT_FLAG_ACCUM_REL_GRADS, lib.MMT_FLAG_EXAMPLE_IDS]
  assert len({f for f in flags}) == 3 and all(f & (f - 1) == 0 for f in flags)       # distinct single bits


def test_abi_version_and_mask_desc_size_are_unchanged(lib):
  assert lib.MMT_ABI_VERSION == 4 and lib.lib().mmt_abi_version() == 4
  assert ctypes.sizeof(lib.MaskDesc) == 48
  assert lib.MaskDesc.valid_len.offset == 0 and lib.MaskDesc.global_index.offset == 40
  header = open(__graft_entry__.ROOT + '/include/mmt_attn.h').read()
  assert '#define MMT_ABI_VERSION 4' in header


def test_example_ids_argument_errors_without_gpu(lib):
  L = lib.lib()
  d = _desc(lib)
  assert L.mmt_workspace_bytes(d) > 0
  d.flags = lib.MMT_FLAG_EXAMPLE_IDS                        # the flag without the ids
  assert L.mmt_workspace_bytes(d) == 0
  assert b'example ids' in L.mmt_last_error()
  assert L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None) == -1
  assert b'example ids' in L.mmt_last_error() and b'NULL' in L.mmt_last_error()
  assert L.mmt_attn_bwd(d, 1, 1, 1, 1, None, None, None, 1, 1, 1, 1, 1, 1, 1, None, 1, 1 << 40, None) == -1
  d.mask.valid_len = 1                                      # ids with an image grid
  assert L.mmt_workspace_bytes(d) > 0
  d.mask.patches_per_row = 12
  d.mask.image_grid = lib.image_grid(1, 2)
  assert L.mmt_workspace_bytes(d) == 0
  assert L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None) == -2
  assert b'image grid' in L.mmt_last_error() and b'example ids' in L.mmt_last_error()
  assert L.mmt_attn_bwd(d, 1, 1, 1, 1, None, None, None, 1, 1, 1, 1, 1, 1, 1, None, 1, 1 << 40, None) == -2
  d.flags = 0                                               # the same grid without the flag is served
  assert L.mmt_workspace_bytes(d) > 0
  d.flags = lib.MMT_FLAG_EXAMPLE_IDS                        # a listed global set: refused as without the ids
  d.mask.image_grid = 0
  d.mask.global_index, d.mask.n_global = 1, 3
  assert L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None) == -2
  assert b'listed global-token set' in L.mmt_last_error()


def test_example_ids_from_breakpoints_is_the_reverse_cumsum():
  import mmt_amd
  rng = np.random.default_rng(0)
  for shape in [(17,), (3, 40), (2, 3, 9)]:
    bp = (rng.random(shape) < 0.2).astype(np.int32)
    got = mmt_amd.example_ids_from_breakpoints(torch.from_numpy(bp))
    assert got.dtype == torch.int32 and tuple(got.shape) == shape
    assert (got.numpy() == np.cumsum(bp[..., ::-1], -1)[..., ::-1]).all()
  assert (mmt_amd.example_ids_from_breakpoints([0, 1, 0, 0, 1, 0]).numpy() == [2, 2, 1, 1, 1, 0]).all()


@pytest.mark.parametrize('S,vl', [(16, 16), (16, 9), (40, 1), (33, 32)])
def test_single_breakpoint_is_valid_len(S, vl):
  """The reference's own pipeline sets one breakpoint, at seq_len - 1 of the example: its ids are 1 on [0, vl) and 0
  after, and their segmented mask is the `valid_len = vl` one."""
  import mmt_amd
  bp = np.zeros(S, np.int32)
  bp[vl - 1] = 1
  ids = mmt_amd.example_ids_from_breakpoints(torch.from_numpy(bp)).numpy()
  assert (ids == (np.arange(S) < vl)).all()
  inside = np.arange(S) < vl
  assert (si.make_segmented_att_mask(ids) == (inside[:, None] == inside[None, :])).all()
  assert (si.make_segmented_att_mask(ids) == si.sparse_pattern_mask(S, vl, S)).all()


def test_example_ids_from_lengths_round_trips():
  import mmt_amd
  S = 50
  lengths = [[7, 1, 20, 22], [50], [3, 3], []]
  ids = mmt_amd.example_ids_from_lengths(lengths, S)
  assert ids.dtype == torch.int32 and tuple(ids.shape) == (4, S)
  a = ids.numpy()
  for row, want in zip(a, lengths):
    assert row[0] == len(want)                                   # ids fall from the row's example count ...
    assert (np.diff(row) <= 0).all() and (np.diff(row) >= -1).all()
    back = [int((row == e).sum()) for e in range(len(want), 0, -1)]
    assert back == want                                          # ... one run per example, in order ...
    assert (row[sum(want):] == 0).all()                          # ... and the tail is 0
  assert (a[0, :7] == 4).all() and a[0, 7] == 3 and (a[0, 8:28] == 2).all() and (a[0, 28:] == 1).all()
  # the same as breakpoints at the examples' last positions
  bp = np.zeros((1, S), np.int32)
  bp[0, np.cumsum(lengths[0]) - 1] = 1
  assert (mmt_amd.example_ids_from_breakpoints(torch.from_numpy(bp)).numpy() == a[:1]).all()
  with pytest.raises(ValueError):
    mmt_amd.example_ids_from_lengths([[30, 30]], S)
  with pytest.raises(ValueError):
    mmt_amd.example_ids_from_lengths([[3, 0]], S)


class _OnDevice(torch.Tensor):
  """A CPU tensor that claims to be on the GPU: lets the argument checks of the host layer run without one (they
  come before anything touches device memory)."""

  @staticmethod
  def make(t):
    return t.as_subclass(_OnDevice)

  @property
  def is_cuda(self):
    return True


def test_python_argument_errors():
  import mmt_amd
  B, S, N, D = 2, 64, 1, 64
  q = _OnDevice.make(torch.zeros(B, S, N, D))
  ids = torch.ones(B, S, dtype=torch.int32)
  pat = mmt_amd.AttentionPattern(local_radius=8, id_mode=0)
  fwd = lambda **kw: mmt_amd.relative_attention_forward(q, q, q, pattern=pat, **kw)
  with pytest.raises(ValueError, match='example_ids'):
    fwd(example_ids=ids.long())                               # wrong dtype
  with pytest.raises(ValueError, match='example_ids'):
    fwd(example_ids=ids[:, :-1].contiguous())                 # wrong shape
  with pytest.raises(ValueError, match='example_ids'):
    fwd(example_ids=torch.ones(B, dtype=torch.int32))         # lengths are not ids
  with pytest.raises(ValueError, match='example_ids'):
    fwd(example_ids=ids.t().contiguous().t())                 # not contiguous
  with pytest.raises(ValueError, match='example_ids'):
    fwd(example_ids=ids.numpy())                              # not a tensor
  with pytest.raises(ValueError, match='not both'):
    fwd(example_ids=ids, valid_len=torch.full((B,), S, dtype=torch.int32))
  with pytest.raises(ValueError, match='example_ids'):
    mmt_amd.relative_attention_forward(q, q, q, att_mask=torch.ones(B, S, S, dtype=torch.int32), example_ids=ids)
  with pytest.raises(ValueError, match='example_ids'):
    mmt_amd.relative_attention_backward(q, q, q, q, None, None, q, torch.zeros(B, N, S), pattern=pat,
                                        example_ids=ids.long())
