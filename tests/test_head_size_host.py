"""Head size 128 (hidden_size / num_attention_heads = 128), host side: the library sizes workspace for D = 128
descriptors of every kind the general kernels take, still refuses every other head size with the same message, and
the encoder builds its relative tables at that head size.  No GPU needed."""
import pytest

import __graft_entry__  # noqa: F401  (sets sys.path)


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


def _desc(lib, D, *, B=2, S=512, N=2, R=32, ng=0, radius=64, id_mode=None, grid=0, P=0, dtype=None):
  import mmt_amd
  d = lib.AttnDesc()
  d.B, d.S, d.N, d.D, d.R = B, S, N, D, R
  d.dtype = lib.MMT_BF16 if dtype is None else dtype
  for name in ('q_stride', 'k_stride', 'v_stride', 'o_stride'):
    st = getattr(d, name)
    st[0], st[1], st[2] = S * N * max(D, 8), N * max(D, 8), max(D, 8)
  d.scale, d.mask_value = 0.125, -10000.0
  pat = mmt_amd.AttentionPattern(local_radius=radius, global_start=S // 2 - ng // 2 if ng else 0, n_global=ng,
                                 id_mode=(1 if R else 0) if id_mode is None else id_mode, max_dist=12,
                                 patches_per_row=P, core_layers=1 if id_mode == 2 else 0, grid_radius=grid,
                                 grid_start=2 if grid else 0)
  d.mask = pat.to_desc(None)
  return d


@pytest.mark.parametrize('R', [0, 9, 49, 100])
@pytest.mark.parametrize('kind', ['band_globals', 'grid', 'dense', 'full'])
def test_workspace_sized_for_head_size_128(lib, kind, R):
  import ctypes
  kw = dict(band_globals=dict(ng=8), grid=dict(grid=1, P=16), dense=dict(radius=1 << 30), full=dict(radius=1 << 30))[kind]
  d = _desc(lib, 128, R=R, **kw)
  L = lib.lib()
  need = L.mmt_workspace_bytes(ctypes.byref(d))
  assert need > 0, L.mmt_last_error()
  d64 = _desc(lib, 64, R=R, **kw)
  need64 = L.mmt_workspace_bytes(ctypes.byref(d64))
  assert need64 > 0
  if kind == 'band_globals':
    # the global-row / global-key partials and the dE partials are D floats wide; the window, plane-walk and
    # hand-over regions (head size 64 only) are left out
    assert need != need64


@pytest.mark.parametrize('D', [0, 32, 96, 256])
def test_other_head_sizes_still_refused(lib, D):
  import ctypes
  L = lib.lib()
  d = _desc(lib, D)
  assert L.mmt_workspace_bytes(ctypes.byref(d)) == 0
  assert b'head size 64' in L.mmt_last_error()


def test_abi_version_unchanged(lib):
  assert lib.lib().mmt_abi_version() == 4 == lib.MMT_ABI_VERSION


def test_encoder_builds_head_size_128_tables():
  import mmt_amd
  from mmt_amd import configs
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {'model': {'encoder': {'mmt': dict(num_hidden_layers=1, hidden_size=256, num_attention_heads=2,
                                                           intermediate_size=512, vocab_size=1000,
                                                           relative_vocab_size=32)}}}})
  task = mmt_amd.tasks.get_task(exp.task)
  model = task.build_model()
  tables = {n: tuple(p.shape) for n, p in model.named_parameters() if n.endswith('relative_emb_table')}
  assert tables and all(s == (32, 2, 128) for s in tables.values()), tables
