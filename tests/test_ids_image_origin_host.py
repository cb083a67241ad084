"""2-D relative ids at the image's position (`MMT_IDS_2D_IMAGE`, id_mode 3), host side: the numpy restatement the GPU
tests feed the oracle (tests/_cases.py `image_origin_ids`), the library's argument checks (no GPU needed), the
descriptor packing and the data-config key."""
import ctypes
import glob
import itertools
import os
import warnings

import pytest

import __graft_entry__  # noqa: F401  (sets sys.path)
from oracle import side_inputs as si
from tests._cases import image_origin_ids


@pytest.mark.parametrize('S,m,P,r,g', [(9, 12, 2, 1, 2), (40, 3, 5, 2, 7), (30, 4, 4, 1, 14)])
def test_restatement_matches_brute_force(S, m, P, r, g):
  I = P * P
  ref = si.relative_ids_from_desc(max(S, 2 * I), 2, m, P, r)     # the reference's ids, image at 0
  one_d = si.relative_ids_from_desc(S, 1, m)
  got = image_origin_ids(S, m, P, r, g)
  for q, k in itertools.product(range(S), range(S)):
    qi, ki = g <= q < g + I, g <= k < g + I
    want = ref[q - g, k - g] if (qi and ki) else (I + 8 + 2 * m + 2 if qi else (I + 8 + 2 * m + 1 if ki else one_d[q, k]))
    assert got[q, k] == want, (q, k)


@pytest.mark.parametrize('S,m,P,r', [(9, 12, 2, 1), (50, 5, 6, 2)])
def test_restatement_at_origin_zero_is_the_reference(S, m, P, r):
  assert (image_origin_ids(S, m, P, r, 0) == si.relative_ids_from_desc(S, 2, m, P, r)).all()


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


def _desc(lib, S=96):
  d = lib.AttnDesc()
  d.B, d.S, d.N, d.D, d.R = 1, S, 1, 64, 49
  d.dtype = lib.MMT_BF16
  for arr in (d.q_stride, d.k_stride, d.v_stride, d.o_stride):
    arr[:] = (S * 64, 64, 64)
  d.scale, d.mask_value = 0.125, -10000.0
  d.mask.local_radius, d.mask.max_dist = 16, 12
  d.mask.patches_per_row, d.mask.core_layers = 6, 2
  return d


def _fwd(L, d):
  return L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None)


def test_abi_is_unchanged(lib):
  assert ctypes.sizeof(lib.MaskDesc) == 48
  assert lib.MMT_ABI_VERSION == 4 and lib.lib().mmt_abi_version() == 4
  assert (lib.MMT_IDS_2D, lib.MMT_IDS_2D_IMAGE) == (2, 3)
  header = open(os.path.join(__graft_entry__.ROOT, 'include', 'mmt_attn.h')).read()
  assert 'MMT_IDS_2D_IMAGE = 3' in header and '#define MMT_ABI_VERSION 4' in header


def test_library_accepts_id_mode_3_and_refuses_4(lib):
  L = lib.lib()
  d = _desc(lib)
  d.mask.id_mode = lib.MMT_IDS_2D_IMAGE
  d.mask.image_grid = lib.image_grid(0, 2)
  assert L.mmt_workspace_bytes(d) > 0                      # accepted; the size query succeeds
  d.mask.image_grid = 0                                    # origin 0
  assert L.mmt_workspace_bytes(d) > 0
  d.mask.image_grid = lib.image_grid(0, 60)                # fits exactly: 60 + 36 = 96
  assert L.mmt_workspace_bytes(d) > 0
  d.mask.id_mode = 4
  assert L.mmt_workspace_bytes(d) == 0
  assert _fwd(L, d) == -1 and b'bad id_mode' in L.mmt_last_error()
  m = lib.MaskDesc()
  m.id_mode, m.max_dist, m.patches_per_row, m.core_layers = 4, 12, 6, 2
  assert L.mmt_side_inputs(m, 1, 96, None, None, 0, None, None, None, None) == -1
  assert b'bad id_mode' in L.mmt_last_error()


def test_image_must_lie_inside_the_sequence_without_a_grid_radius(lib):
  L = lib.lib()
  d = _desc(lib)
  d.mask.id_mode = lib.MMT_IDS_2D_IMAGE
  d.mask.image_grid = lib.image_grid(0, 61)                # a = 0: 61 + 36 > 96
  assert L.mmt_workspace_bytes(d) == 0
  assert _fwd(L, d) == -1 and b'g + P*P > S' in L.mmt_last_error()
  d.mask.image_grid = lib.image_grid(1, 61)                # and with a grid radius
  assert _fwd(L, d) == -1 and b'g + P*P > S' in L.mmt_last_error()
  m = lib.MaskDesc()
  m.id_mode, m.max_dist, m.patches_per_row, m.core_layers = lib.MMT_IDS_2D_IMAGE, 12, 6, 2
  m.image_grid = lib.image_grid(0, 61)
  assert L.mmt_side_inputs(m, 1, 96, None, None, 0, None, None, None, None) == -1
  assert b'g + P*P > S' in L.mmt_last_error()
  # the other id modes keep ignoring the word when its radius is 0
  for mode in (lib.MMT_IDS_1D, lib.MMT_IDS_2D):
    d.mask.id_mode = mode
    d.mask.image_grid = lib.image_grid(0, 61)
    assert L.mmt_workspace_bytes(d) > 0, mode


@pytest.mark.parametrize('bad', [dict(patches_per_row=0), dict(patches_per_row=-3), dict(core_layers=0), dict(core_layers=-1)],
                         ids=lambda b: '-'.join(f'{k}{v}' for k, v in b.items()))
def test_mode_3_refuses_what_mode_2_refuses(lib, bad):
  L = lib.lib()
  for mode in (lib.MMT_IDS_2D, lib.MMT_IDS_2D_IMAGE):
    d = _desc(lib)
    d.mask.id_mode = mode
    d.mask.image_grid = lib.image_grid(0, 2)
    for k, v in bad.items():
      setattr(d.mask, k, v)
    assert L.mmt_workspace_bytes(d) == 0, mode
    assert _fwd(L, d) == -1, mode
    m = lib.MaskDesc()
    m.id_mode, m.max_dist, m.patches_per_row, m.core_layers = mode, 12, 6, 2
    m.image_grid = lib.image_grid(0, 2)
    for k, v in bad.items():
      setattr(m, k, v)
    assert L.mmt_side_inputs(m, 1, 96, None, None, 0, None, None, None, None) == -1, mode


def test_packed_example_ids_do_not_take_the_origin_for_a_grid(lib):
  """`MMT_FLAG_EXAMPLE_IDS` refuses an image grid; a = 0 with g > 0 (the origin of the ids) is no grid."""
  L = lib.lib()
  d = _desc(lib)
  d.mask.id_mode = lib.MMT_IDS_2D_IMAGE
  d.mask.image_grid = lib.image_grid(0, 2)
  d.flags = lib.MMT_FLAG_EXAMPLE_IDS
  d.mask.valid_len = 1                                     # never read: host-only query
  assert L.mmt_workspace_bytes(d) > 0
  d.mask.image_grid = lib.image_grid(1, 2)
  assert L.mmt_workspace_bytes(d) == 0 and b'image grid' in L.mmt_last_error()


def test_pattern_packs_the_origin(lib):
  import mmt_amd
  P = mmt_amd.AttentionPattern
  pat = P(id_mode=3, patches_per_row=6, core_layers=2, grid_start=5)
  d = pat.to_desc(None)
  assert d.id_mode == 3 and d.image_grid == lib.image_grid(0, 5) == 5 << 8
  assert P(id_mode=3, patches_per_row=6, core_layers=2).to_desc(None).image_grid == 2 << 8     # default origin 2
  assert P(id_mode=3, patches_per_row=6, core_layers=2, grid_radius=1).to_desc(None).image_grid == 1 | (2 << 8)
  assert P(id_mode=2, patches_per_row=6, core_layers=2, grid_start=5).to_desc(None).image_grid == 0   # as before
  assert pat != P(id_mode=3, patches_per_row=6, core_layers=2, grid_start=4)                   # cache key


def test_config_key_reaches_the_pattern(tmp_path):
  from mmt_amd import _lib, configs, input_utils
  kw = dict(max_seq_len=256, image_size=224, patch_size=16, relative_pos_max_distance=12)
  data = configs.MmtPretrainDataConfig(relative_att_num_core_layers=2, relative_att_align_image=True, **kw)
  pat = input_utils.attention_pattern_from_config(data)
  assert (pat.id_mode, pat.grid_start, pat.grid_radius, pat.patches_per_row, pat.core_layers) == (_lib.MMT_IDS_2D_IMAGE, 2, 0, 14, 2)
  assert pat.to_desc(None).image_grid == 2 << 8
  data.image_grid_radius = 1                               # ids and grid share the origin
  pat = input_utils.attention_pattern_from_config(data)
  assert pat.id_mode == _lib.MMT_IDS_2D_IMAGE and pat.to_desc(None).image_grid == 1 | (2 << 8)
  # no effect without 2-D ids
  data1d = configs.MmtPretrainDataConfig(relative_att_align_image=True, **kw)
  assert input_utils.attention_pattern_from_config(data1d) == \
      input_utils.attention_pattern_from_config(configs.MmtPretrainDataConfig(**kw))
  # default off, in both config classes, settable from YAML and --params_override
  assert configs.MmtDataConfig().relative_att_align_image is False
  assert configs.MmtEncoderConfig().relative_att_align_image is False
  path = tmp_path / 'align.yaml'
  path.write_text('task:\n  train_data:\n    relative_att_num_core_layers: 1\n    relative_att_align_image: true\n')
  cfg = configs.parse_configuration('mmt/pretraining', [str(path)], strict=True)
  assert cfg.task.train_data.relative_att_align_image is True
  assert input_utils.attention_pattern_from_config(cfg.task.train_data).id_mode == _lib.MMT_IDS_2D_IMAGE
  cfg = configs.parse_configuration('mmt/pretraining', params_override='task.train_data.relative_att_align_image=true')
  assert cfg.task.train_data.relative_att_align_image is True


YAMLS = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'exp_yamls', '**', '*.yaml'), recursive=True))


@pytest.mark.parametrize('path', YAMLS, ids=lambda p: '/'.join(p.split(os.sep)[-3:]))
def test_golden_yamls_keep_their_pattern_with_the_key_off(path):
  """With `relative_att_align_image` off (the default) every golden experiment gives the pattern it gave before the key
  existed: id_mode 2 exactly where the data config sets core layers, 1 otherwise, and an all-zero image_grid word."""
  from mmt_amd import _lib, configs, input_utils
  exp_name = 'mmt/pretraining' if os.sep + 'pretrain' + os.sep in path else 'mmt/classification'
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')                        # keys the reference's own dataclasses lack (test_host_logic.py)
    cfg = configs.parse_configuration(exp_name, [path])
  data = cfg.task.train_data
  assert data.relative_att_align_image is False
  pat = input_utils.attention_pattern_from_config(data)
  r = data.relative_att_num_core_layers
  assert pat.id_mode == (_lib.MMT_IDS_2D if r > 0 else _lib.MMT_IDS_1D)
  P = data.image_size // data.patch_size
  want = input_utils.AttentionPattern(local_radius=1 << 30, global_start=0, n_global=0, id_mode=pat.id_mode,
                                      max_dist=data.relative_pos_max_distance, patches_per_row=P if r > 0 else 0,
                                      core_layers=r, grid_radius=0, grid_start=2)
  assert pat == want and pat.to_desc(None).image_grid == 0


def test_some_golden_yaml_has_2d_ids():
  from mmt_amd import configs
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    rs = [configs.parse_configuration('mmt/pretraining' if os.sep + 'pretrain' + os.sep in p else 'mmt/classification',
                                      [p]).task.train_data.relative_att_num_core_layers for p in YAMLS]
  assert len(YAMLS) >= 9 and any(r > 0 for r in rs)
