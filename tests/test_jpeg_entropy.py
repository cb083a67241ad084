"""JPEG entropy decode on the device, without a GPU: mmt_jpeg_scan_plan and mmt_jpeg_entropy_host -- the functions the
kernels run, as plain loops, round for round -- against the merged host path (mmt_jpeg_coefficients), bit for bit over
whole buffers; the refusals, the fallbacks of decode_jpeg_images(entropy='device', device='cpu'), and the sanitizer
program (`make asan-jpeg-entropy`)."""
import ctypes
import os

import numpy as np
import pytest

from tests import _jpeg_cases as J
from tests import _jpeg_entropy_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (8, 128)


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


def check_parity(lib, items, subseq_bytes):
  """Plans at the worst-case max_rounds: no file may fall back, coef equals the host decode over the whole buffer and
  the guard, qtables are equal."""
  images, coef, qtables, _, _, ok = E.host_stage(lib, items)
  assert all(ok)
  plans = E.Plans(lib, items, images, subseq_bytes)
  assert plans.rc == [0] * len(items), plans.messages
  got, status = E.entropy_host(lib, plans, images, coef.size, plans.worst_rounds)
  assert status.tolist() == [0] * len(items), status.tolist()
  bad = np.nonzero(got[:coef.size] != coef)[0]
  assert bad.size == 0, f'{bad.size} coefficients differ, first at {bad[0]}: got {got[bad[0]]}, want {coef[bad[0]]}'
  assert np.all(got[coef.size:] == E.COEF_FILL)
  assert np.array_equal(plans.qtables, qtables)
  return plans


@pytest.mark.parametrize('subseq_bytes', SIZES)
def test_every_fixture_alone_equals_the_host_decode(lib, subseq_bytes):
  for name in J.names():
    check_parity(lib, [name], subseq_bytes)


@pytest.mark.parametrize('subseq_bytes', SIZES)
def test_all_fixtures_in_one_call_equal_the_host_decode(lib, subseq_bytes):
  names = list(J.names())
  order = np.random.default_rng(20215).permutation(len(names))
  check_parity(lib, [names[i] for i in order], subseq_bytes)


@pytest.mark.parametrize('subseq_bytes', SIZES)
def test_restart_segments_one_pixel_files_and_long_codes(lib, subseq_bytes):
  """Named: segments of one and two MCUs (rst1, rst2), the 1 x 1 files, and the optimised tables of q100_opt, whose
  codes are long."""
  rst = [n for n in J.names() if n.endswith(('_rst1', '_rst2'))]
  ones = [n for n in J.names() if n.startswith('1x1_')]
  opt = [n for n in J.names() if n.endswith('_q100_opt')]
  assert len(rst) == 26 and len(ones) == 7 and len(opt) == 13
  plans = check_parity(lib, rst, subseq_bytes)
  for b, name in enumerate(rst):
    s = plans.scans[b]
    assert s.restart_interval == (1 if name.endswith('_rst1') else 2)
    assert s.n_segments == -(-s.mcus // s.restart_interval) and s.n_subseq >= s.n_segments, name
  check_parity(lib, ones, subseq_bytes)
  plans = check_parity(lib, opt, subseq_bytes)
  # a q100_opt table holds codes beyond the 9-bit lookup: the longer-code branch of the decoder is on the tested path
  tables = plans.huff.reshape(len(opt) * 6, lib.MMT_JPEG_HUFF_WORDS)
  used = tables[:, :256].any(axis=1)                            # a grey file leaves four of its six tables zero
  longest = tables[:, 256:263].view(np.int32)                   # the largest code of lengths 10..16, -1: none
  assert (longest[used] >= 0).any()


@pytest.mark.parametrize('subseq_bytes', SIZES)
def test_dense_stuffing(lib, subseq_bytes):
  """Noise at quality 100: the file holds 0xff 0x00 pairs, and at size 8 at least one subsequence begins on the 0x00 of
  a pair (the reader must skip it)."""
  raw = E.dense_stuffing()
  sos = raw.index(b'\xff\xda')
  assert raw.count(b'\xff\x00', sos) >= 20
  plans = check_parity(lib, [raw, '48x80_444_q90'], subseq_bytes)
  if subseq_bytes == 8:
    s = plans.scans[0]
    first = s.byte_offset - plans.file_offsets[0]
    on_zero = [at for at in range(first + 8, first + s.byte_count, 8) if raw[at - 1] == 0xFF and raw[at] == 0x00]
    assert s.n_segments == 1 and on_zero, 'no subsequence of 8 bytes begins on a stuffed zero'


def test_one_round_does_not_converge_and_the_python_call_falls_back(lib):
  from mmt_amd import feature_pipeline as fp
  name = '48x80_444_q90'
  images, coef, _, _, _, _ = E.host_stage(lib, [name, '9x3_444_q90'])
  plans = E.Plans(lib, [name, '9x3_444_q90'], images, 8)
  _, status = E.entropy_host(lib, plans, images, coef.size, 1)
  assert status[0] == lib.MMT_JPEG_ST_NOT_CONVERGED, status.tolist()
  blobs = [J.data(name), J.data('9x3_444_q90')]
  pixels, offsets, heights, widths = fp.decode_jpeg_images(blobs, 'cpu', entropy='device', subseq_bytes=8, max_rounds=1)
  for i, n in enumerate((name, '9x3_444_q90')):
    e = J.expected(n)
    assert (int(heights[i]), int(widths[i])) == e.shape[:2]
    assert np.array_equal(pixels[int(offsets[i]):int(offsets[i]) + e.size].numpy(), e.reshape(-1)), n


def test_three_scans_are_refused_by_the_plan_and_served_by_the_fallback(lib):
  import torch
  from mmt_amd import feature_pipeline as fp
  raw = E.three_scans()
  images, _, _, _, _, ok = E.host_stage(lib, [raw])
  assert ok == [True]
  plans = E.Plans(lib, [raw], images, 128)
  assert plans.rc == [E.E_UNSUPPORTED] and 'the host decode takes it' in plans.messages[0], plans.messages
  blobs = [J.data('8x8_420_q75'), raw, J.data('17x9_grey_q80')]
  host = fp.decode_jpeg_images(blobs, 'cpu', entropy='host')
  dev = fp.decode_jpeg_images(blobs, 'cpu', entropy='device')
  for a, b in zip(host, dev):
    assert a.dtype == b.dtype and torch.equal(a, b)
  e = J.expected('17x9_444_q90')                                # the same coefficients as the fixture: the same pixels
  assert np.array_equal(dev[0][int(dev[1][1]):int(dev[1][1]) + e.size].numpy(), e.reshape(-1))
  # malformed headers stay MMT_E_INVALID
  im, scan = lib.JpegImage(), lib.JpegScan()
  good = J.data('17x9_420_q75')
  lib.check(lib.lib().mmt_jpeg_info(good, len(good), ctypes.byref(im)))
  assert lib.lib().mmt_jpeg_scan_plan(good, 40, ctypes.byref(im), 128, ctypes.byref(scan), None, None, None, 0, None, 0) == E.E_INVALID
  assert lib.lib().mmt_jpeg_scan_plan(good, len(good), ctypes.byref(im), 96, ctypes.byref(scan), None, None, None, 0, None, 0) == E.E_INVALID
  assert b'power of two' in lib.lib().mmt_last_error()


@pytest.mark.parametrize('subseq_bytes', SIZES)
def test_corrupt_streams_get_a_status_and_disturb_nothing(lib, subseq_bytes):
  """A truncated scan and an inverted byte between two good files: the bad images get an error status, the good ones
  are exact, nothing is written outside the planes, and the Python call raises what entropy='host' raises."""
  from mmt_amd import feature_pipeline as fp
  items = ['33x31_422_q50', E.truncated_scan(), E.flipped_byte(lib), '48x80_420_q30_rst1']
  images, coef, _, _, _, ok = E.host_stage(lib, items)
  assert ok == [True, False, False, True]
  plans = E.Plans(lib, items, images, subseq_bytes)
  assert plans.rc == [0, 0, 0, 0], plans.messages
  got, status = E.entropy_host(lib, plans, images, coef.size, plans.worst_rounds)
  errors = (lib.MMT_JPEG_ST_BAD_CODE, lib.MMT_JPEG_ST_RUN, lib.MMT_JPEG_ST_OVERRUN, lib.MMT_JPEG_ST_BLOCKS)
  assert status[0] == 0 and status[3] == 0 and status[1] in errors and status[2] in errors, status.tolist()
  good = E.planes_mask(images, coef.size, (0, 3))
  assert np.array_equal(got[:coef.size][good], coef[good])
  assert np.all(got[coef.size:] == E.COEF_FILL)                 # the planes tile the buffer: the guard is what lies outside
  for bad in (1, 2):
    blobs = [E.blob(it) for it in items if it is not items[3 - bad]]       # one bad file at a time, at index 1
    with pytest.raises(ValueError) as host:
      fp.decode_jpeg_images(blobs, 'cpu', entropy='host')
    with pytest.raises(ValueError) as dev:
      fp.decode_jpeg_images(blobs, 'cpu', entropy='device', subseq_bytes=subseq_bytes)
    assert str(dev.value) == str(host.value) and 'data[1]' in str(host.value)


def test_arguments_are_checked(lib):
  from mmt_amd import feature_pipeline as fp
  blobs = [J.data('8x8_444_q90')]
  for kw in (dict(entropy='gpu'), dict(entropy='device', subseq_bytes=96), dict(entropy='device', max_rounds=0)):
    with pytest.raises(ValueError):
      fp.decode_jpeg_images(blobs, 'cpu', **kw)
  auto = fp.decode_jpeg_images(blobs, 'cpu', entropy='auto')    # no GPU asked for: the host path
  assert np.array_equal(auto[0].numpy(), J.expected('8x8_444_q90').reshape(-1))
  L = lib.lib()
  assert L.mmt_jpeg_entropy_workspace_bytes(1, 10, 10, 96, 4) == 0 and L.mmt_jpeg_entropy_workspace_bytes(1, 10, 11, 128, 4) == 0
  assert L.mmt_jpeg_entropy_workspace_bytes(0, 10, 10, 128, 4) == 0 and L.mmt_jpeg_entropy_workspace_bytes(1, 10, 10, 128, 0) == 0
  images, coef, _, _, _, _ = E.host_stage(lib, ['8x8_444_q90'])
  plans = E.Plans(lib, ['8x8_444_q90'], images, 128)
  need = plans.workspace_bytes(lib, 2)
  ws, status = J.aligned(need, np.uint8), np.zeros(1, dtype=np.int32)
  a = lambda **kw: plans.args(**{**dict(images_ptr=ctypes.addressof(images), bytes_ptr=plans.bytes.ctypes.data,
                                        scans_ptr=ctypes.addressof(plans.scans), huff_ptr=plans.huff.ctypes.data,
                                        seg_ptr=plans.segments.ctypes.data, sub_ptr=plans.subseqs.ctypes.data, max_rounds=2,
                                        coef_ptr=coef.ctypes.data, coef_elems=coef.size, status_ptr=status.ctypes.data,
                                        ws_ptr=ws.ctypes.data, ws_bytes=need), **kw})
  assert L.mmt_jpeg_entropy_host(*a()) == 0
  assert L.mmt_jpeg_entropy_host(*a(ws_bytes=need - 1)) == -3 and b'bytes needed' in L.mmt_last_error()
  assert L.mmt_jpeg_entropy_host(*a(max_rounds=0)) == -1
  assert L.mmt_jpeg_entropy_host(*a(coef_ptr=None)) == -1
  assert L.mmt_jpeg_entropy_host(*a(bytes_ptr=plans.bytes.ctypes.data + 1)) == -1 and b'aligned' in L.mmt_last_error()


def test_decode_image_features_passes_entropy_through(lib):
  import types
  import torch
  from mmt_amd import feature_pipeline as fp
  cfg = types.SimpleNamespace(is_training=False, image_size=32, patch_size=16, output_channel_bits=3)
  blobs = [J.data(n) for n in ('33x31_420_q75', '9x2_422_q50', '48x80_444_q90', '17x9_grey_q80', '1x1_420_q75')] + [E.three_scans()]
  host = fp.decode_image_features(cfg, blobs, keep_unnormalized=True, device='cpu', entropy='host')
  dev = fp.decode_image_features(cfg, blobs, keep_unnormalized=True, device='cpu', entropy='device')
  assert set(host) == set(dev)
  for k in host:
    assert torch.equal(host[k], dev[k]) if isinstance(host[k], torch.Tensor) else host[k] == dev[k], k
  pf = fp.images_to_patch_features(blobs, 32, 16, device='cpu', entropy='device')
  assert torch.equal(pf['patch_embeddings'], host['patch_embeddings'])


def test_sanitizer_program_of_the_entropy_host_stage():
  """`make asan-jpeg-entropy` (csrc/Makefile): mmt_jpeg_scan_plan and mmt_jpeg_entropy_host under AddressSanitizer +
  UBSan, driven by a C program with its own main over the fixtures, their truncations and corruptions, and wrong plans.
  CPU only; nothing is loaded into Python."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  csrc = os.path.join(ROOT, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-jpeg-entropy'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'jpeg entropy asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
