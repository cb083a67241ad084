"""Image-grid term of the structured pattern (SURVEY.md App. A.5 `grid_radius`), host side: the numpy restatement the
GPU tests feed the oracle (tests/_cases.py `grid_mask`), the descriptor packing (`mmt_mask_desc.image_grid`, ABI 4), the library's argument errors
(no GPU needed) and the data-config plumbing."""
import ctypes
import itertools

import numpy as np
import pytest

import __graft_entry__  # noqa: F401  (sets sys.path)
from tests._cases import grid_mask


@pytest.mark.parametrize('S,g,P,a', [(40, 2, 5, 1), (64, 2, 7, 2), (50, 0, 7, 3), (30, 5, 4, 0), (100, 3, 9, 8)])
def test_grid_mask_matches_brute_force(S, g, P, a):
  got = grid_mask(S, g, P, a)
  want = np.zeros((S, S), bool)
  for q, k in itertools.product(range(S), range(S)):
    if a > 0 and g <= q < g + P * P and g <= k < g + P * P:
      rq, cq = divmod(q - g, P)
      rk, ck = divmod(k - g, P)
      want[q, k] = abs(rq - rk) <= a and abs(cq - ck) <= a
  assert (got == want).all()
  assert (got == got.T).all()                      # symmetric: the dK/dV pass walks the same tiles


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


def test_pattern_packs_image_grid(lib):
  import mmt_amd
  P = mmt_amd.AttentionPattern
  assert P(local_radius=8).to_desc(None).image_grid == 0               # default: off
  assert P(local_radius=8, grid_start=7).to_desc(None).image_grid == 0   # radius 0: off, whatever the start
  pat = P(local_radius=8, patches_per_row=12, grid_radius=3, grid_start=2)
  assert pat.to_desc(None).image_grid == 3 | (2 << 8)
  assert lib.image_grid(8, 4097) == 8 | (4097 << 8)
  assert pat.normalized() is pat
  listed = P(local_radius=8, patches_per_row=12, grid_radius=1, global_index=(40, 3, 17)).normalized()
  assert (listed.grid_radius, listed.grid_start, listed.patches_per_row) == (1, 2, 12)
  assert hash(pat) != hash(P(local_radius=8, patches_per_row=12, grid_radius=2, grid_start=2))    # cache key
  assert pat != P(local_radius=8, patches_per_row=12, grid_radius=3, grid_start=3)


def test_mask_desc_layout_keeps_the_padding_slot(lib):
  assert ctypes.sizeof(lib.MaskDesc) == 48
  assert lib.MaskDesc.image_grid.offset == 36
  assert lib.MaskDesc.global_index.offset == 40
  header = open(__graft_entry__.ROOT + '/include/mmt_attn.h').read()
  assert '#define MMT_IMAGE_GRID(a, g)' in header


def _desc(lib, S=256):
  d = lib.AttnDesc()
  d.B, d.S, d.N, d.D, d.R = 1, S, 1, 64, 32
  d.dtype = lib.MMT_BF16
  for arr in (d.q_stride, d.k_stride, d.v_stride, d.o_stride):
    arr[:] = (S * 64, 64, 64)
  d.scale, d.mask_value = 0.125, -10000.0
  d.mask.local_radius, d.mask.id_mode, d.mask.max_dist = 16, lib.MMT_IDS_1D, 12
  return d


def test_image_grid_argument_errors_without_gpu(lib):
  L = lib.lib()
  d = _desc(lib)
  d.mask.image_grid = lib.image_grid(1, 2)                 # a grid without patches_per_row
  assert L.mmt_workspace_bytes(d) == 0
  assert L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None) == -1
  assert b'patches_per_row' in L.mmt_last_error()
  d.mask.patches_per_row = 12
  d.mask.image_grid = lib.image_grid(9, 2)                 # radius above what is built
  assert L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None) == -2
  assert b'grid radius 9' in L.mmt_last_error() and b'up to 8' in L.mmt_last_error()
  d.mask.patches_per_row = 16
  d.mask.image_grid = lib.image_grid(1, 1)                 # 1 + 256 > S
  assert L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None) == -1
  assert b'image grid outside the sequence' in L.mmt_last_error()
  d.mask.image_grid = lib.image_grid(1, 0)                 # fits exactly
  assert L.mmt_workspace_bytes(d) > 0
  # the same checks in mmt_side_inputs, whatever the id mode
  m = lib.MaskDesc()
  m.local_radius, m.id_mode, m.image_grid = 4, lib.MMT_IDS_NONE, lib.image_grid(2, 2)
  assert L.mmt_side_inputs(m, 1, 64, None, None, 1, None, None, None, None) == -1
  assert b'patches_per_row' in L.mmt_last_error()
  m.patches_per_row = 8
  assert L.mmt_side_inputs(m, 1, 64, None, None, 1, None, None, None, None) == -1      # 2 + 64 > 64
  assert b'image grid outside the sequence' in L.mmt_last_error()
  m.image_grid = lib.image_grid(9, 0)
  assert L.mmt_side_inputs(m, 1, 64, None, None, 1, None, None, None, None) == -2
  assert b'up to 8' in L.mmt_last_error()


def test_patches_per_row_leaves_1d_ids_alone():
  """patches_per_row is read by the 2-D id generator only: with 1-D ids (what a grid pattern sets it for) the ids are
  the plain clipped ones -- restated here through the oracle the device generator is checked against."""
  from oracle import side_inputs as si
  S, m = 80, 6
  plain = si.relative_ids_from_desc(S, 1, m)
  assert (si.relative_ids_from_desc(S, 1, m, 8, 0) == plain).all()
  assert (si.relative_ids_from_desc(S, 1, m, 8, 2) == plain).all()


def test_attention_pattern_from_config_sets_the_grid(tmp_path):
  from mmt_amd import _lib, configs, input_utils
  data = configs.MmtPretrainDataConfig(max_seq_len=512, image_size=192, patch_size=16, relative_pos_max_distance=12,
                                       local_radius=32, num_global_tokens=8)
  base = input_utils.attention_pattern_from_config(data)
  assert (base.grid_radius, base.patches_per_row, base.id_mode) == (0, 0, _lib.MMT_IDS_1D)
  assert base.to_desc(None).image_grid == 0
  data.image_grid_radius = 2
  pat = input_utils.attention_pattern_from_config(data)
  assert (pat.grid_radius, pat.grid_start, pat.patches_per_row) == (2, 2, 12)
  assert pat.id_mode == _lib.MMT_IDS_1D and pat.core_layers == 0          # the id mode is unchanged
  assert pat.global_start == 2 + 144 and pat.n_global == 8
  data2d = configs.MmtPretrainDataConfig(max_seq_len=512, image_size=192, patch_size=16, relative_att_num_core_layers=2,
                                         image_grid_radius=1)
  pat2 = input_utils.attention_pattern_from_config(data2d)
  assert pat2.id_mode == _lib.MMT_IDS_2D and pat2.patches_per_row == 12 and pat2.grid_radius == 1
  # YAML and dotted overrides reach the key
  path = tmp_path / 'grid.yaml'
  path.write_text('task:\n  train_data:\n    image_grid_radius: 3\n')
  cfg = configs.parse_configuration('mmt/pretraining', [str(path)], strict=True)
  assert cfg.task.train_data.image_grid_radius == 3
  cfg = configs.parse_configuration('mmt/pretraining', params_override='task.train_data.image_grid_radius=1')
  assert cfg.task.train_data.image_grid_radius == 1
  assert configs.MmtDataConfig().image_grid_radius == 0
