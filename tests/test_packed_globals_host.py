"""Per-example global tokens on packed rows (`MMT_FLAG_EXAMPLE_GLOBALS`), host side: the flag's argument errors and the
workspace plan through the C ABI (no pointer is followed, no GPU needed), and what `mmt_amd.ops` makes of a pattern with
example starts and a global range."""
import re

import pytest
import torch

import __graft_entry__  # noqa: F401  (sets sys.path)


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


def _desc(lib, S=256, R=32):
  d = lib.AttnDesc()
  d.B, d.S, d.N, d.D, d.R = 2, S, 3, 64, R
  d.dtype = lib.MMT_BF16
  for arr in (d.q_stride, d.k_stride, d.v_stride, d.o_stride):
    arr[:] = (S * 3 * 64, 3 * 64, 64)
  d.scale, d.mask_value = 0.125, -10000.0
  d.mask.local_radius, d.mask.id_mode, d.mask.max_dist = 16, lib.MMT_IDS_1D, 12
  d.mask.valid_len = 1
  return d


def _calls(lib):
  L = lib.lib()
  fwd = lambda d: L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None)
  # a backward whose descriptor is accepted stops at its (empty) workspace: MMT_E_WORKSPACE, nothing is launched
  bwd = lambda d: L.mmt_attn_bwd(d, 1, 1, 1, 1, None, None, None, 1, 1, 1, 1, 1, 1, 1, None, None, 0, None)
  return L, fwd, bwd


def test_flag_value_matches_the_header(lib):
  header = open(__graft_entry__.ROOT + '/include/mmt_attn.h').read()
  m = re.search(r'#define MMT_FLAG_EXAMPLE_GLOBALS (\d+)u', header)
  assert m and int(m.group(1)) == lib.MMT_FLAG_EXAMPLE_GLOBALS == 16
  assert lib.MMT_ABI_VERSION == 4 and lib.lib().mmt_abi_version() == 4


def test_flag_with_both_packing_flags_is_served_without_rows_partials(lib):
  """The descriptor passes the checks of the workspace query and of the backward (which then stops at its empty
  workspace; the forward needs no workspace on this route, so an accepted forward would launch: it is the GPU suite's).
  The plan has no split rows: the workspace is that of n_global = 0 plus the [B*N, n_global, Rp] floats that move
  off_drel's successors."""
  L, fwd, bwd = _calls(lib)
  packing = lib.MMT_FLAG_EXAMPLE_IDS | lib.MMT_FLAG_EXAMPLE_STARTS
  d = _desc(lib)
  d.flags = packing | lib.MMT_FLAG_EXAMPLE_GLOBALS
  d.mask.global_start, d.mask.n_global = 40, 8
  with_globals = L.mmt_workspace_bytes(d)
  assert with_globals > 0, L.mmt_last_error()
  assert bwd(d) == -3 and b'workspace' in L.mmt_last_error()
  d.mask.patches_per_row, d.mask.image_grid = 12, lib.image_grid(1, 2)      # an image grid beside the globals: served
  assert L.mmt_workspace_bytes(d) == with_globals
  assert bwd(d) == -3
  d.mask.patches_per_row, d.mask.image_grid = 0, 0
  d.mask.n_global = 0                                      # the flag with no global token: the origin call
  without = L.mmt_workspace_bytes(d)
  d.flags = packing
  assert L.mmt_workspace_bytes(d) == without > 0
  assert with_globals == without + d.B * d.N * 8 * 32 * 4
  d.mask.n_global = 8                                      # without the flag: refused as before, same words
  assert L.mmt_workspace_bytes(d) == 0
  assert b'example starts with global tokens' in L.mmt_last_error()
  assert fwd(d) == -2 and bwd(d) == -2


def test_flag_without_example_starts_is_invalid(lib):
  L, fwd, bwd = _calls(lib)
  d = _desc(lib)
  d.mask.global_start, d.mask.n_global = 40, 8
  for flags in (lib.MMT_FLAG_EXAMPLE_GLOBALS, lib.MMT_FLAG_EXAMPLE_GLOBALS | lib.MMT_FLAG_EXAMPLE_IDS):
    d.flags = flags
    assert L.mmt_workspace_bytes(d) == 0
    assert fwd(d) == -1 and bwd(d) == -1
    msg = L.mmt_last_error()
    assert b'MMT_FLAG_EXAMPLE_GLOBALS' in msg and b'MMT_FLAG_EXAMPLE_STARTS' in msg and b'MMT_FLAG_EXAMPLE_IDS' in msg


def test_flag_with_a_listed_set_or_image_origin_ids_is_unsupported(lib):
  L, fwd, bwd = _calls(lib)
  d = _desc(lib, R=49)
  d.flags = lib.MMT_FLAG_EXAMPLE_IDS | lib.MMT_FLAG_EXAMPLE_STARTS | lib.MMT_FLAG_EXAMPLE_GLOBALS
  d.mask.global_start, d.mask.n_global = 0, 3
  d.mask.global_index = 1                                  # a listed global set: refused as ever
  assert fwd(d) == -2 and b'listed global-token set' in L.mmt_last_error()
  assert bwd(d) == -2 and b'listed global-token set' in L.mmt_last_error()
  d.mask.global_index = None
  d.mask.global_start, d.mask.n_global = 40, 8
  d.mask.id_mode, d.mask.patches_per_row, d.mask.core_layers = lib.MMT_IDS_2D_IMAGE, 4, 1
  d.mask.image_grid = lib.image_grid(0, 2)
  assert L.mmt_workspace_bytes(d) == 0 and b'MMT_IDS_2D_IMAGE' in L.mmt_last_error()
  assert fwd(d) == -2 and bwd(d) == -2
  d.mask.n_global = 0                                      # ... and served without global tokens, flag or not
  assert L.mmt_workspace_bytes(d) > 0


def _tensors(S=64):
  q = torch.zeros(1, S, 1, 64)
  ids = torch.ones(1, S, dtype=torch.int32)
  return q, ids, torch.zeros(1, S, dtype=torch.int32)


def _flags(lib, pattern, ids, starts):
  from mmt_amd import ops
  q = _tensors()[0]
  return ops._make_desc(q, q, q, q, 0, pattern, None, None, -10000.0, False, 0.0, 0, 0, ids, starts).flags


def test_make_desc_sets_the_flag_for_starts_with_a_global_range_only(lib, monkeypatch):
  import mmt_amd
  from mmt_amd import ops
  monkeypatch.setattr(ops, '_sync_words', lambda device, stream, words: torch.zeros(words, dtype=torch.int32))
  monkeypatch.setattr(ops, '_stream_ptr', lambda device: 0)
  monkeypatch.setattr(ops.step_scalars, 'host_epoch', lambda device: 0)
  _, ids, starts = _tensors()
  G = lib.MMT_FLAG_EXAMPLE_GLOBALS
  with_globals = mmt_amd.AttentionPattern(local_radius=8, global_start=20, n_global=8)
  plain = mmt_amd.AttentionPattern(local_radius=8)
  both = lib.MMT_FLAG_EXAMPLE_IDS | lib.MMT_FLAG_EXAMPLE_STARTS
  assert _flags(lib, with_globals, ids, starts) == both | G
  assert _flags(lib, plain, ids, starts) == both
  assert _flags(lib, with_globals, ids, None) == lib.MMT_FLAG_EXAMPLE_IDS
  assert _flags(lib, with_globals, None, None) == 0
  assert _flags(lib, None, ids, starts) == both


def test_resolve_pattern_keeps_a_global_range_with_starts_structured(lib, monkeypatch):
  import mmt_amd
  from mmt_amd import ops
  q, ids, starts = _tensors()
  sent = []
  monkeypatch.setattr(ops, '_materialized', lambda pattern, *a: sent.append(pattern) or ('mask', 'ids'))
  pat = mmt_amd.AttentionPattern(local_radius=8, global_start=20, n_global=8)
  assert ops._resolve_pattern(pat, None, None, None, q, ids, starts) == (pat, None, None) and not sent
  grid = mmt_amd.AttentionPattern(local_radius=8, global_start=20, n_global=8, patches_per_row=3, grid_radius=1)
  assert ops._resolve_pattern(grid, None, None, None, q, ids, starts) == (grid, None, None) and not sent
  run = mmt_amd.AttentionPattern(local_radius=8, global_index=(22, 20, 21))          # a listed run is the range form
  got = ops._resolve_pattern(run, None, None, None, q, ids, starts)
  assert got[0].global_index is None and (got[0].global_start, got[0].n_global) == (20, 3) and not sent
  # MMT_IDS_2D_IMAGE with global tokens, and a scattered listed set: the dense operator's inputs
  image = mmt_amd.AttentionPattern(local_radius=8, global_start=20, n_global=8, id_mode=lib.MMT_IDS_2D_IMAGE,
                                   patches_per_row=3, core_layers=1)
  assert ops._resolve_pattern(image, None, None, None, q, ids, starts) == (None, 'mask', 'ids') and sent == [image]
  listed = mmt_amd.AttentionPattern(local_radius=8, global_index=(3, 9))
  assert ops._resolve_pattern(listed, None, None, None, q, ids, starts) == (None, 'mask', 'ids') and len(sent) == 2
  # ... and MMT_IDS_2D_IMAGE without global tokens stays structured
  image0 = mmt_amd.AttentionPattern(local_radius=8, id_mode=lib.MMT_IDS_2D_IMAGE, patches_per_row=3, core_layers=1)
  assert ops._resolve_pattern(image0, None, None, None, q, ids, starts) == (image0, None, None) and len(sent) == 2
