"""PNG inflate on the device, on the GPU: mmt_png_scanlines against the host variant (the same text with the lanes as a
loop), the library's host inflate and zlib.decompress, bit for bit -- every fixture, the hand-built corners and the
stress streams in one call per subseq_bytes, the prefixes of one stream against the host variant's status words,
wrong descriptors between guard bytes, two calls for determinism, and decode_png_images(inflate='device')."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import _png_inflate_cases as C
from tests._png_cases import GUARD, SENTINEL, chunk, data, expected, host_stage, idats, ihdr, names  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  import torch
  if not torch.cuda.is_available():
    pytest.skip('needs a GPU')
  from mmt_amd import _lib
  _lib.build()
  return _lib


@pytest.fixture(scope='module')
def everything(lib):
  """Cases 1 to 3 as one batch: (names, files, expected scanlines or None, expected status), the Batch."""
  rows = [(n, data(n), None, 0) for n in names()]
  rows += [(k, f, want, 0) for k, (f, want) in C.corner_cases().items()]
  rows += [(k, f, want, st) for k, (f, want, st) in C.stress_cases().items()]
  batch = C.Batch(lib, [r[1] for r in rows], guard=GUARD)
  assert batch.B == len(rows)
  return rows, batch


@pytest.fixture(scope='module')
def host_results(lib, everything):
  rows, batch = everything
  return {s: C.run_host(lib, batch, s, SENTINEL) for s in (8, 32, 128)}


@pytest.mark.parametrize('subseq', (8, 32, 128))
def test_fixtures_corners_and_stress_streams_in_one_call(lib, everything, host_results, subseq):
  rows, batch = everything
  raw, status = C.run_device(lib, batch, subseq, SENTINEL)
  assert [int(s) for s in status] == [r[3] for r in rows], {r[0]: int(s) for r, s in zip(rows, status) if s != r[3]}
  C.check_equivalence(batch, raw, status, subseq, SENTINEL)
  host_raw, host_status = host_results[subseq]
  assert np.array_equal(status, host_status)
  for k, (name, _, want, st) in enumerate(rows):
    if st == 0:
      got = bytes(batch.slice(raw, k))
      assert got == bytes(batch.slice(host_raw, k)), name
      assert got == zlib.decompress(batch.stream(k)), name
      assert want is None or got == want, name
  assert np.array_equal(raw, host_raw)                          # also what a refused stream left behind: the same bytes


def test_two_calls_give_the_same_bytes_and_status(lib, everything):
  rows, batch = everything
  a = C.run_device(lib, batch, 32, SENTINEL)
  b = C.run_device(lib, batch, 32, SENTINEL)
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_statuses_of_prefixes_corruptions_and_hand_built_streams(lib):
  files = C.mutations(data('64x3_g8_f1_i1_dynamic')) + [f for f, _ in C.status_cases().values()]
  batch = C.Batch(lib, files, guard=GUARD)
  assert batch.B > 0.9 * len(files) and any(batch.host_ok) and not all(batch.host_ok)
  for subseq in C.SUBSEQ:
    raw, status = C.run_device(lib, batch, subseq, SENTINEL)
    C.check_equivalence(batch, raw, status, subseq, SENTINEL)
    host_raw, host_status = C.run_host(lib, batch, subseq, SENTINEL)
    assert np.array_equal(status, host_status) and np.array_equal(raw, host_raw)
  want = [st for _, st in C.status_cases().values()]
  assert [int(s) for s in status[-len(want):]] == want


def test_wrong_descriptors_stay_inside_the_buffers(lib):
  import torch
  L = lib.lib()
  blobs = [data(n) for n in ('33x70_rgb8_f3_i0_fixed', '130x7_g2_fcycle_i0_dynamic', '16x200_p8_f3_i0_stored')]
  good = C.Batch(lib, blobs, guard=GUARD)
  n_raw, n_comp = good.n_raw - 2 * GUARD, good.n_comp
  offsets = (-1, -(1 << 40), 1, 7, n_raw - 1, n_raw, n_raw + 12345, n_comp - 2, n_comp, 1 << 50, 2 ** 63 - 1, -2 ** 63)
  sizes = (0, -5, 1, 2, 3, 8, 1000, 65535, 1 << 30, 2 ** 31 - 1, -2 ** 31)
  # every wrong descriptor is one image of one big batch over the same three streams and the same raw block
  rows_im, rows_st = [], []
  for a, off in enumerate(offsets):
    for s, size in enumerate(sizes):
      for variant in range(6):
        k = (a + s) % 3
        m = lib.PngImage.from_buffer_copy(good.images[k])
        t = lib.PngStream.from_buffer_copy(good.streams[(a + variant) % 3])
        m.raw_offset -= GUARD
        if variant == 0: t.comp_offset = off
        if variant == 1: t.comp_bytes = off; t.comp_offset = offsets[(a + s) % len(offsets)]
        if variant == 2: m.raw_offset = off; m.width = size
        if variant == 3: m.raw_bytes = off; m.height = size; m.interlace = a % 3
        if variant == 4: m.width = size; m.height = sizes[(s + a) % len(sizes)]; m.bit_depth = (1, 2, 4, 8, 16, 0, -1, 3)[(a + s) % 8]; m.color_type = (0, 2, 3, 4, 6, -1, 99)[s % 7]
        if variant == 5: m.raw_offset = off; m.raw_bytes = offsets[(a + 5) % len(offsets)]; t.comp_bytes = size; m.interlace = 1
        rows_im.append(m); rows_st.append(t)
  B = len(rows_im)
  images, streams = (lib.PngImage * B)(*rows_im), (lib.PngStream * B)(*rows_st)
  dev = lambda a: torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).cuda()
  images_d, streams_d = dev(images), dev(streams)
  comp = torch.full((n_comp + 2 * GUARD,), SENTINEL, dtype=torch.uint8)
  comp[GUARD:GUARD + n_comp] = torch.from_numpy(good.comp)
  comp = comp.cuda()
  need = L.mmt_png_scanlines_workspace_bytes(B)
  work = torch.empty(need, dtype=torch.uint8, device='cuda')
  for subseq in C.SUBSEQ:
    buf = torch.full((good.n_raw,), SENTINEL, dtype=torch.uint8, device='cuda')
    status = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    lib.check(L.mmt_png_scanlines(B, images_d.data_ptr(), streams_d.data_ptr(), comp.data_ptr() + GUARD, n_comp, buf.data_ptr() + GUARD, n_raw,
                                  status.data_ptr(), subseq, work.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n_raw:] == SENTINEL).all())
    assert bool(((status >= 0) & (status <= 11)).all())
  assert L.mmt_png_scanlines(B, images_d.data_ptr(), streams_d.data_ptr(), comp.data_ptr(), n_comp, buf.data_ptr(), n_raw, status.data_ptr(), 24,
                             work.data_ptr(), need, None) == -1 and b'power of two' in L.mmt_last_error()


def test_decode_png_images_on_the_gpu_equals_the_committed_pixels_and_the_default_call(lib):
  import torch
  from mmt_amd import feature_pipeline as fp
  blobs = [data(n) for n in names()]
  got = fp.decode_png_images(blobs, 'cuda', inflate='device')
  default = fp.decode_png_images(blobs, 'cuda')
  assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, default))
  pixels, offsets = got[0].cpu().numpy(), got[1].cpu().numpy()
  for i, n in enumerate(names()):
    e = expected(n)
    assert np.array_equal(pixels[offsets[i]:offsets[i] + e.size].reshape(e.shape), e), n
  # a file the kernel refuses and the host refuses too: the host path's message
  bad = list(blobs[:5])
  bad[2] = C.status_cases()['distance'][0]
  with pytest.raises(ValueError) as host:
    fp.decode_png_images(bad, 'cuda')
  with pytest.raises(ValueError) as dev:
    fp.decode_png_images(bad, 'cuda', inflate='device')
  assert str(dev.value) == str(host.value) and str(dev.value).startswith('data[2] ')
  mixed = fp.decode_images(blobs[:4], 'cuda', png_inflate='device')
  assert all(torch.equal(a, b) for a, b in zip(mixed, fp.decode_images(blobs[:4], 'cuda')))
