"""PNG inflate on the device, without a GPU: mmt_png_gather and mmt_png_scanlines_host -- the host variant runs the
text the kernel runs, with the 256 lanes as a loop -- against the library's host inflate and zlib.decompress, bit for
bit: every fixture, the hand-built corners, streams that stress the rounds and the resolution of the copies, the
equivalence (status 0 exactly when mmt_png_inflate accepts, then equal bytes) on every prefix and single-byte corruption
of three files and on one stream per status word, wrong descriptors between guard bytes, and the Python entry points."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import _jpeg_cases as J
from tests import _png_inflate_cases as C
from tests._png_cases import GUARD, SENTINEL, chunk, data, expected, host_stage, idats, ihdr, names  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ('9x17_g8_f0_i0_stored', '64x3_g8_f1_i1_dynamic', '9x17_p2_f0_i0_fixed')


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


@pytest.fixture(scope='module')
def fixtures(lib):
  return C.Batch(lib, [data(n) for n in names()], guard=GUARD)


@pytest.mark.parametrize('subseq', (8, 32, 128))
def test_every_fixture_equals_the_host_inflate_and_zlib(lib, fixtures, subseq):
  assert fixtures.B == len(names()) and all(fixtures.host_ok)
  raw, status = C.run_host(lib, fixtures, subseq, SENTINEL)
  assert not status.any(), status
  C.check_equivalence(fixtures, raw, status, subseq, SENTINEL)
  images, host_raw, _, _, _ = host_stage(lib, [data(n) for n in names()], guard=GUARD)
  assert np.array_equal(raw, host_raw)                          # the same layout, the same bytes, the guards included
  for k in range(fixtures.B):
    assert bytes(fixtures.slice(raw, k)) == zlib.decompress(fixtures.stream(k)), names()[k]


@pytest.mark.parametrize('subseq', (8, 32, 128))
def test_decode_png_images_on_cpu_equals_the_committed_pixels(lib, subseq):
  from mmt_amd import feature_pipeline as fp
  blobs = [data(n) for n in names()]
  pixels, offsets, heights, widths = fp.decode_png_images(blobs, 'cpu', inflate='device', subseq_bytes=subseq)
  for i, n in enumerate(names()):
    e = expected(n)
    assert (int(heights[i]), int(widths[i])) == e.shape[:2]
    assert np.array_equal(pixels[int(offsets[i]):int(offsets[i]) + e.size].numpy().reshape(e.shape), e), n
  default = fp.decode_png_images(blobs, 'cpu')
  assert all(bool((a == b).all()) for a, b in zip(default, (pixels, offsets, heights, widths)))


@pytest.mark.parametrize('subseq', (8, 32, 128))
def test_the_hand_built_corners(lib, subseq):
  cases = C.corner_cases()
  assert len(cases) == 3
  batch = C.Batch(lib, [f for f, _ in cases.values()], guard=GUARD)
  raw, status = C.run_host(lib, batch, subseq, SENTINEL)
  assert batch.B == 3 and not status.any(), status
  C.check_equivalence(batch, raw, status, subseq, SENTINEL)
  for k, (_, want) in enumerate(cases.values()):
    assert bytes(batch.slice(raw, k)) == want


@pytest.fixture(scope='module')
def stress(lib):
  cases = C.stress_cases()
  return cases, C.Batch(lib, [c[0] for c in cases.values()], guard=GUARD)


@pytest.mark.parametrize('subseq', C.SUBSEQ)
def test_streams_that_stress_rounds_and_resolution(lib, stress, subseq):
  cases, batch = stress
  assert batch.B == len(cases)
  raw, status = C.run_host(lib, batch, subseq, SENTINEL)
  C.check_equivalence(batch, raw, status, subseq, SENTINEL)
  for k, (name, (_, want, st)) in enumerate(cases.items()):
    assert status[k] == st, (name, int(status[k]))
    if want is not None:
      assert zlib.decompress(batch.stream(k)) == want and bytes(batch.slice(raw, k)) == want, name


def test_raw_size_one_through_the_descriptors(lib):
  """One byte of output is no image (a row is a filter byte and a sample), so the descriptor is written by hand."""
  L = lib.lib()
  for subseq in C.SUBSEQ:
    for payload in (b'\x00', b'\x04', b'\x05'):
      comp = np.frombuffer(zlib.compress(payload, 9), dtype=np.uint8).copy()
      im = lib.PngImage(1, 1, 8, 0, 0, 0, 3, 1, 0)
      st = lib.PngStream(0, comp.size)
      raw = np.full(7, SENTINEL, dtype=np.uint8)
      status = np.zeros(1, dtype=np.int32)
      need = L.mmt_png_scanlines_workspace_bytes(1)
      work = np.empty(need, dtype=np.uint8)
      lib.check(L.mmt_png_scanlines_host(1, ctypes.byref(im), ctypes.byref(st), comp.ctypes.data, comp.size, raw.ctypes.data, raw.size,
                                         status.ctypes.data, subseq, work.ctypes.data, need))
      assert status[0] == 0 and bytes(raw) == bytes([SENTINEL] * 3) + payload + bytes([SENTINEL] * 3)


@pytest.mark.parametrize('subseq', C.SUBSEQ)
def test_one_stream_per_status_word(lib, subseq):
  cases = C.status_cases()
  batch = C.Batch(lib, [f for f, _ in cases.values()], guard=GUARD)
  assert batch.B == len(cases)
  raw, status = C.run_host(lib, batch, subseq, SENTINEL)
  C.check_equivalence(batch, raw, status, subseq, SENTINEL)
  assert [int(s) for s in status] == [st for _, st in cases.values()], dict(zip(cases, status))
  assert {st for _, st in cases.values()} == set(range(11))     # every word but MMT_PNG_ST_NO_PROGRESS, see status_cases


@pytest.mark.parametrize('name', SMALL)
def test_equivalence_on_every_prefix_and_single_byte_corruption(lib, name):
  files = C.mutations(data(name))
  batch = C.Batch(lib, files, guard=GUARD)
  assert batch.B > 0.9 * len(files) and not all(batch.host_ok) and any(batch.host_ok)       # a broken zlib header stops at the gather
  for subseq in C.SUBSEQ:
    raw, status = C.run_host(lib, batch, subseq, SENTINEL)
    C.check_equivalence(batch, raw, status, (name, subseq), SENTINEL)


def test_wrong_descriptors_stay_inside_the_buffers(lib):
  L = lib.lib()
  blobs = [data(n) for n in ('33x70_rgb8_f3_i0_fixed', '130x7_g2_fcycle_i0_dynamic', '16x200_p8_f3_i0_stored')]
  good = C.Batch(lib, blobs, guard=GUARD)
  n_raw, n_comp = good.n_raw - 2 * GUARD, good.n_comp
  buf = np.full(good.n_raw, SENTINEL, dtype=np.uint8)
  inner = buf[GUARD:GUARD + n_raw]                               # the call sees only this; the guards lie outside it
  comp = np.full(n_comp + 2 * GUARD, SENTINEL, dtype=np.uint8)
  comp[GUARD:GUARD + n_comp] = good.comp
  offsets = (-1, -(1 << 40), 1, 7, n_raw - 1, n_raw, n_raw + 12345, n_comp - 2, n_comp, 1 << 50, 2 ** 63 - 1, -2 ** 63)
  sizes = (0, -5, 1, 2, 3, 8, 1000, 65535, 1 << 30, 2 ** 31 - 1, -2 ** 31)
  need = L.mmt_png_scanlines_workspace_bytes(3)
  work = np.empty(need, dtype=np.uint8)
  status = np.zeros(3, dtype=np.int32)
  calls = 0
  for a, off in enumerate(offsets):
    for s, size in enumerate(sizes):
      for variant in range(6):
        images = (lib.PngImage * 3)(*[lib.PngImage.from_buffer_copy(good.images[k]) for k in range(3)])
        streams = (lib.PngStream * 3)(*[lib.PngStream.from_buffer_copy(good.streams[k]) for k in range(3)])
        for k in range(3):
          images[k].raw_offset -= GUARD
        m, t = images[(a + s) % 3], streams[(a + variant) % 3]
        if variant == 0: t.comp_offset = off
        if variant == 1: t.comp_bytes = off; t.comp_offset = offsets[(a + s) % len(offsets)]
        if variant == 2: m.raw_offset = off; m.width = size
        if variant == 3: m.raw_bytes = off; m.height = size; m.interlace = a % 3
        if variant == 4: m.width = size; m.height = sizes[(s + a) % len(sizes)]; m.bit_depth = (1, 2, 4, 8, 16, 0, -1, 3)[(a + s) % 8]; m.color_type = (0, 2, 3, 4, 6, -1, 99)[s % 7]
        if variant == 5: m.raw_offset = off; m.raw_bytes = offsets[(a + 5) % len(offsets)]; t.comp_bytes = size; m.interlace = 1
        for subseq in C.SUBSEQ:
          lib.check(L.mmt_png_scanlines_host(3, images, streams, comp.ctypes.data + GUARD, n_comp, inner.ctypes.data, n_raw, status.ctypes.data,
                                             subseq, work.ctypes.data, need))
          calls += 1
          assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + n_raw:] == SENTINEL), (off, size, variant)
          assert np.all((status >= 0) & (status <= 11))
  assert calls == len(offsets) * len(sizes) * 6 * 2
  # argument errors are return codes; a bad stream is not
  im, st = good.images, good.streams
  args = lambda **kw: [kw.get('B', 3), im, st, comp.ctypes.data + GUARD, kw.get('n_comp', n_comp), inner.ctypes.data, kw.get('n_raw', n_raw),
                       status.ctypes.data, kw.get('subseq', 32), work.ctypes.data, kw.get('need', need)]
  assert L.mmt_png_scanlines_host(*args(B=0)) == -1
  assert L.mmt_png_scanlines_host(*args(n_comp=0)) == -1
  assert L.mmt_png_scanlines_host(*args(n_raw=0)) == -1
  for bad in (0, 4, 24, 256, -8):
    assert L.mmt_png_scanlines_host(*args(subseq=bad)) == -1 and b'power of two' in L.mmt_last_error()
  assert L.mmt_png_scanlines_host(*args(need=need - 1)) != 0 and b'bytes needed' in L.mmt_last_error()
  assert L.mmt_png_scanlines_workspace_bytes(0) == 0


def test_gather_applies_the_rules_and_words_of_the_host_walk(lib):
  L = lib.lib()
  g8 = np.arange(12, dtype=np.uint8).reshape(3, 4)
  from tests import _png_cases as P
  raw = P.scanlines('g8', g8, 1)
  good = P.deflate(raw)
  h = P.ihdr(4, 3, 8, 0)

  def both(blob):
    im = lib.PngImage()
    lib.check(L.mmt_png_info(blob, len(blob), ctypes.byref(im)))
    out, pal = np.zeros(64, dtype=np.uint8), np.zeros(768, dtype=np.uint8)
    rc_h = L.mmt_png_inflate(blob, len(blob), ctypes.byref(im), out.ctypes.data, 64, pal.ctypes.data)
    msg_h = L.mmt_last_error().decode() if rc_h else ''
    comp = np.full(len(blob) + 2 * GUARD, SENTINEL, dtype=np.uint8)
    st = lib.PngStream(GUARD, 0)
    rc_g = L.mmt_png_gather(blob, len(blob), ctypes.byref(im), comp.ctypes.data, GUARD + len(blob), ctypes.byref(st), pal.ctypes.data)
    msg_g = L.mmt_last_error().decode() if rc_g else ''
    assert np.all(comp[:GUARD] == SENTINEL) and np.all(comp[GUARD + len(blob):] == SENTINEL)
    return (rc_h, msg_h), (rc_g, msg_g), bytes(comp[GUARD:GUARD + st.comp_bytes])

  file_of = lambda *idat, tail=chunk(b'IEND'), extra=b'': P.SIGNATURE + h + extra + b''.join(idat) + tail
  # accepted: one chunk, split chunks, an empty chunk, a gap that ends the stream, bytes behind IEND
  for blob, stream in ((file_of(chunk(b'IDAT', good)), good),
                       (file_of(idats(good, 1)), good), (file_of(idats(good, 7)), good),
                       (file_of(chunk(b'IDAT', good[:3]), chunk(b'IDAT', b''), chunk(b'IDAT', good[3:])), good),
                       (file_of(chunk(b'IDAT', good), chunk(b'tEXt', b'k\x00v', crc=1), chunk(b'IDAT', b'junk')), good),
                       (file_of(chunk(b'IDAT', good)) + b'trailing', good)):
    host, gather, comp = both(blob)
    assert host == (0, '') and gather == (0, '') and comp == stream
  # refused with the host's code and words
  for blob in (file_of(chunk(b'IDAT', good, crc=7)),
               file_of(chunk(b'IDAT', good[:5]), chunk(b'IDAT', good[5:], crc=7)),
               file_of(chunk(b'IDAT', good), chunk(b'IDAT', b'junk', crc=7)),
               file_of(chunk(b'IDAT', good), tail=chunk(b'IEND', b'', crc=7)),
               file_of(chunk(b'IDAT', good), tail=b''),
               file_of(chunk(b'IDAT', good))[:-1],
               file_of(chunk(b'IDAT', good), chunk(b'tRNS', b'\x00\x05')),
               file_of(chunk(b'IDAT', good), chunk(b'ABcd', b'x')),
               file_of(chunk(b'IDAT', b'\x78')),
               file_of(chunk(b'IDAT', b'\x78\xbb' + good[2:])),
               file_of(chunk(b'IDAT', b'\x88\x1c' + good[2:])),
               file_of(chunk(b'IDAT', b'\x78\x9d' + good[2:])),
               file_of(chunk(b'IDAT', b'\x79\x9c' + good[2:]))):
    host, gather, _ = both(blob)
    assert host[0] != 0 and gather == host, (host, gather)
  # arguments
  blob = file_of(chunk(b'IDAT', good))
  im = lib.PngImage()
  lib.check(L.mmt_png_info(blob, len(blob), ctypes.byref(im)))
  comp, pal = np.zeros(len(blob), dtype=np.uint8), np.zeros(768, dtype=np.uint8)
  st = lib.PngStream(0, 0)
  assert L.mmt_png_gather(blob, len(blob), ctypes.byref(im), comp.ctypes.data, len(good) - 1, ctypes.byref(st), pal.ctypes.data) == -1
  assert b'leave comp_out' in L.mmt_last_error()
  st.comp_offset = -1
  assert L.mmt_png_gather(blob, len(blob), ctypes.byref(im), comp.ctypes.data, comp.size, ctypes.byref(st), pal.ctypes.data) == -1
  st.comp_offset = 0
  assert L.mmt_png_gather(blob, len(blob), ctypes.byref(im), None, comp.size, ctypes.byref(st), pal.ctypes.data) == -1
  im.width += 1
  assert L.mmt_png_gather(blob, len(blob), ctypes.byref(im), comp.ctypes.data, comp.size, ctypes.byref(st), pal.ctypes.data) == -1
  assert b'does not describe this stream' in L.mmt_last_error()


# ---------------------------------------------------------------------------------------------------
# the Python entry points
# ---------------------------------------------------------------------------------------------------
def test_a_corrupt_file_in_a_batch_raises_the_host_paths_message(lib):
  from mmt_amd import feature_pipeline as fp
  blobs = [data(n) for n in names()[:6]]
  for make in (lambda b: b[:len(b) // 2],                                                     # the chunk walk refuses it
               lambda b: b[:-20] + bytes([b[-20] ^ 0x10]) + b[-19:],                          # Adler-32 or CRC, at the end of the data
               lambda b: C.status_cases()['distance'][0], lambda b: C.status_cases()['filter byte'][0]):
    bad = list(blobs)
    bad[4] = make(blobs[4])
    with pytest.raises(ValueError) as host:
      fp.decode_png_images(bad, 'cpu')
    for workers in (1, 4):
      with pytest.raises(ValueError) as dev:
        fp.decode_png_images(bad, 'cpu', inflate='device', workers=workers)
      assert str(dev.value) == str(host.value) and str(dev.value).startswith('data[4] cannot be decoded: ')


def test_decode_images_passes_png_inflate_to_the_png_items_only(lib):
  from mmt_amd import feature_pipeline as fp
  jpegs = [J.data(n) for n in ('33x31_420_q75', '9x2_422_q50', '17x9_grey_q80')]
  pngs = [data(n) for n in names()[:5]]
  mixed = [pngs[0], jpegs[0], pngs[1], pngs[2], jpegs[1], jpegs[2], pngs[3], pngs[4]]
  for items in (mixed, pngs, jpegs):
    default = fp.decode_images(items, 'cpu')
    device = fp.decode_images(items, 'cpu', png_inflate='device')
    assert all(bool((a == b).all()) for a, b in zip(default, device))
  feats = fp.images_to_patch_features(pngs, 32, 8, device='cpu')
  feats_dev = fp.images_to_patch_features(pngs, 32, 8, device='cpu', png_inflate='device')
  import torch
  assert feats.keys() == feats_dev.keys()
  for k in feats:
    assert torch.equal(feats[k], feats_dev[k]) if isinstance(feats[k], torch.Tensor) else feats[k] == feats_dev[k], k


def test_unknown_values_raise(lib):
  from mmt_amd import feature_pipeline as fp
  blobs = [data(names()[0])]
  with pytest.raises(ValueError, match="inflate must be 'host' or 'device'"):
    fp.decode_png_images(blobs, 'cpu', inflate='gpu')
  with pytest.raises(ValueError, match="png_inflate must be 'host' or 'device'"):
    fp.decode_images(blobs, 'cpu', png_inflate='auto')
  for bad in (0, 4, 48, 256):
    with pytest.raises(ValueError, match='power of two'):
      fp.decode_png_images(blobs, 'cpu', inflate='device', subseq_bytes=bad)


def test_sanitizer_program_of_the_host_variant():
  """`make asan-png-inflate`: a stand-alone program over host code only, under AddressSanitizer and UBSan."""
  import shutil
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  csrc = os.path.join(ROOT, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-png-inflate'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'png inflate asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
