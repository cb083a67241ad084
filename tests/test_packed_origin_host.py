"""Packed multimodal examples (`MMT_FLAG_EXAMPLE_STARTS`, the `example_starts=` keyword), host side: the layout helper on
hand-written rows, the library's argument errors through `mmt_workspace_bytes` (no GPU needed), the torch form of the packed
embedding assembly against every example alone, and the composed dense side inputs against the numpy composition."""
import ctypes
import re

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (sets sys.path)
from oracle import side_inputs as si
from tests._cases import grid_mask


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


def test_packed_example_layout_on_hand_written_rows():
  import mmt_amd
  ids, starts, slots, first = mmt_amd.packed_example_layout([[3, 2, 4], [5], []], [[True, False, True], [True], []], 10)
  for t in (ids, starts, slots):
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 10)
  assert ids.tolist() == [[3, 3, 3, 2, 2, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 0, 0, 0, 0, 0], [0] * 10]
  assert starts.tolist() == [[0, 0, 0, 3, 3, 5, 5, 5, 5, 9], [0, 0, 0, 0, 0, 5, 5, 5, 5, 5], [0] * 10]
  assert slots.tolist() == [[0, 0, 0, -1, -1, 1, 1, 1, 1, -1], [2, 2, 2, 2, 2, -1, -1, -1, -1, -1], [-1] * 10]
  assert first.dtype == torch.int64 and first.tolist() == [[0, 0], [0, 3], [0, 5], [1, 0]]
  # every run of equal ids starts where its start says, the tail included
  for b in range(3):
    for s in range(10):
      st = int(starts[b, s])
      assert ids[b, st] == ids[b, s] and (st == 0 or ids[b, st - 1] != ids[b, s])
  with pytest.raises(ValueError):
    mmt_amd.packed_example_layout([[3, 2]], [[True]], 10)
  with pytest.raises(ValueError):
    mmt_amd.packed_example_layout([[8, 8]], [[True, True]], 10)


def test_flag_value_matches_the_header_and_the_abi_is_unchanged(lib):
  header = open(__graft_entry__.ROOT + '/include/mmt_attn.h').read()
  m = re.search(r'#define MMT_FLAG_EXAMPLE_STARTS (\d+)u', header)
  assert m and int(m.group(1)) == lib.MMT_FLAG_EXAMPLE_STARTS == 8
  flags = [lib.MMT_FLAG_SCALE_BEFORE_ADD, lib.MMT_FLAG_ACCUM_REL_GRADS, lib.MMT_FLAG_EXAMPLE_IDS, lib.MMT_FLAG_EXAMPLE_STARTS]
  assert len(set(flags)) == 4 and all(f & (f - 1) == 0 for f in flags)
  assert lib.MMT_ABI_VERSION == 4 and lib.lib().mmt_abi_version() == 4 and '#define MMT_ABI_VERSION 4' in header
  assert ctypes.sizeof(lib.MaskDesc) == 48
  assert lib.MaskDesc.valid_len.offset == 0 and lib.MaskDesc.global_index.offset == 40


def test_example_starts_argument_errors_without_gpu(lib):
  L = lib.lib()
  fwd = lambda d: L.mmt_attn_fwd(d, 1, 1, 1, 1, None, None, None, 1, None, None, 0, None)
  bwd = lambda d: L.mmt_attn_bwd(d, 1, 1, 1, 1, None, None, None, 1, 1, 1, 1, 1, 1, 1, None, 1, 1 << 40, None)
  both = lib.MMT_FLAG_EXAMPLE_IDS | lib.MMT_FLAG_EXAMPLE_STARTS
  d = _desc(lib)
  d.mask.valid_len = 1
  d.flags = lib.MMT_FLAG_EXAMPLE_STARTS                     # starts without the ids flag
  assert L.mmt_workspace_bytes(d) == 0
  assert b'MMT_FLAG_EXAMPLE_IDS' in L.mmt_last_error()
  assert fwd(d) == -1 and bwd(d) == -1
  d.flags = both                                            # both flags, NULL pointer
  d.mask.valid_len = None
  assert L.mmt_workspace_bytes(d) == 0
  assert b'NULL' in L.mmt_last_error() and b'starts' in L.mmt_last_error()
  assert fwd(d) == -1 and bwd(d) == -1
  d.mask.valid_len = 1                                      # both flags and the planes: served
  assert L.mmt_workspace_bytes(d) > 0
  d.mask.patches_per_row = 12                               # ... with an image grid too: the point of the flag
  d.mask.image_grid = lib.image_grid(1, 2)
  assert L.mmt_workspace_bytes(d) > 0
  d.flags = lib.MMT_FLAG_EXAMPLE_IDS                        # ids + grid without starts: refused as before
  assert L.mmt_workspace_bytes(d) == 0
  assert fwd(d) == -2 and b'image grid' in L.mmt_last_error() and b'example ids' in L.mmt_last_error()
  d.flags = both                                            # starts with global tokens: the dense route
  d.mask.image_grid = 0
  d.mask.global_start, d.mask.n_global = 20, 8
  assert L.mmt_workspace_bytes(d) == 0
  assert b'dense operator' in L.mmt_last_error() and b'global tokens' in L.mmt_last_error()
  assert fwd(d) == -2 and bwd(d) == -2
  d.mask.global_start, d.mask.n_global = 0, 3               # a listed global set: refused as ever
  d.mask.global_index = 1
  assert fwd(d) == -2 and b'listed global-token set' in L.mmt_last_error()


def test_python_argument_checks():
  enc = _tiny_encoder()
  with pytest.raises(ValueError, match='needs example_ids'):     # starts say where the example of an id begins
    enc(torch.zeros(1, 8, dtype=torch.int32), example_starts=torch.zeros(1, 8, dtype=torch.int32))
  with pytest.raises(ValueError, match='patch_slots'):
    enc.embed(torch.zeros(1, 8, dtype=torch.int32), None, torch.zeros(1, 4, 12), False,
              example_starts=torch.zeros(1, 8, dtype=torch.int32))


def _tiny_encoder():
  import mmt_amd
  torch.manual_seed(0)
  return mmt_amd.MmtEncoder(vocab_size=50, hidden_size=16, num_hidden_layers=1, num_attention_heads=1, intermediate_size=32,
                            max_absolute_position_embeddings=40, relative_vocab_size=32, patch_embedding_size=12).eval()


def test_packed_embed_rows_equal_each_example_alone_on_the_cpu():
  """The torch form of the assembly: position s of an example takes position row s - start and patch s - start - 2 of
  its own image; an example without an image, and the padding tail, take no patch.  Bit for bit what `embed` gives for
  the example alone."""
  import mmt_amd
  enc = _tiny_encoder()
  P2, S = 4, 40
  lengths, has = [[9, 12, 7], [20, 6]], [[True, False, True], [True, True]]     # row 0 ends in a 12-position tail
  ids, starts, slots, first = mmt_amd.packed_example_layout(lengths, has, S)
  g = torch.Generator().manual_seed(3)
  word_ids = torch.randint(0, 50, (2, S), generator=g, dtype=torch.int32)
  patches = torch.randn(4, P2, 12, generator=g)
  with torch.no_grad():
    got = enc.embed(word_ids, None, patches, False, example_starts=starts, patch_slots=slots)
    e_img = 0
    for b, (row, flags) in enumerate(zip(lengths, has)):
      at = 0
      for L, img in zip(row + [S - sum(row)], flags + [False]):
        if L == 0:
          continue
        alone = enc.embed(word_ids[b:b + 1, at:at + L], None, patches[e_img:e_img + 1] if img else None, False)
        assert torch.equal(got[b, at:at + L], alone[0]), (b, at)
        e_img += int(img)
        at += L
  # the second example of a row is NOT what the row-aligned assembly gives it
  with torch.no_grad():
    aligned = enc.embed(word_ids, None, patches[[0, 2]], False)
  assert not torch.equal(got[0, 9:21], aligned[0, 9:21])


@pytest.mark.parametrize('id_mode,grid', [(1, None), (2, None), (2, (1, 2))], ids=['1d', '2d', '2d-grid'])
def test_compose_origin_equals_the_numpy_composition(id_mode, grid):
  """`ops.compose_origin` (what `_materialized` feeds the dense operator under starts): the single-example [S,S] mask /
  ids gathered at the local positions and ANDed with the id equality, bit for bit the per-run blocks on the diagonal.
  `_materialized` itself builds the single-example pattern with `mmt_side_inputs` on the device, so its first half needs
  a GPU: it is covered by the dense-route case of test_gpu_packed_origin.py, at the attention tolerances."""
  import mmt_amd
  from mmt_amd import ops
  S, P, r, m, radius, g0, ng = 60, 3, 1, 4, 5, 11, 3
  lengths = [[20, 25], [13, 30, 17]]
  ids, starts, _, _ = mmt_amd.packed_example_layout(lengths, [[True] * len(x) for x in lengths], S)
  pat_mask = si.sparse_pattern_mask(S, S, radius, g0, ng).astype(bool)
  if grid:
    pat_mask = pat_mask | grid_mask(S, grid[1], P, grid[0])
  pat_ids = si.relative_ids_from_desc(S, id_mode, m, P, r)
  mask, rel = ops.compose_origin(torch.from_numpy(pat_mask.astype(np.int32)), torch.from_numpy(pat_ids), ids, starts)
  want_mask, want_rel = np.zeros((2, S, S), np.int32), np.zeros((2, S, S), np.int32)
  for b, row in enumerate(lengths):
    at = 0
    for L in row + ([S - sum(row)] if sum(row) < S else []):
      pm = si.sparse_pattern_mask(L, L, radius, g0, ng).astype(bool)
      if grid:
        pm = pm | grid_mask(L, grid[1], P, grid[0])
      want_mask[b, at:at + L, at:at + L] = pm
      want_rel[b, at:at + L, at:at + L] = si.relative_ids_from_desc(max(L, P * P), id_mode, m, P, r)[:L, :L]
      at += L
  assert mask.dtype == torch.int32 and rel.dtype == torch.int32
  assert (mask.numpy() == want_mask).all()
  assert (rel.numpy() == want_rel).all()
