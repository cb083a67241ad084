"""JPEG decode without a GPU: the numpy oracle against the committed Pillow decodes, the host stage (mmt_jpeg_info,
mmt_jpeg_coefficients) against the oracle coefficient for coefficient, mmt_jpeg_pixels_host and the Python entry
points against the committed pixels -- all bit for bit -- the refusals, and the sanitizer program (`make asan-jpeg`)."""
import ctypes
import io
import os
import types

import numpy as np
import pytest

from tests import _jpeg_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


def test_fixture_set_is_the_stated_one_and_small():
  sizes = ('1x1', '8x8', '7x5', '9x2', '9x3', '9x4', '40x1', '1x40', '17x9', '16x16', '33x31', '24x17', '48x80')
  modes = ('444_q90', '422_q50', '420_q75', '420_q100_opt', '420_q30_rst1', '422_q95_rst2', 'grey_q80')
  assert list(J.names()) == [f'{s}_{m}' for s in sizes for m in modes] + [J.LARGE]
  files = os.listdir(J.GOLDEN)
  assert all(os.path.getsize(os.path.join(J.GOLDEN, f)) <= 64 * 1024 for f in files)
  assert sum(os.path.getsize(os.path.join(J.GOLDEN, f)) for f in files) <= 256 * 1024


def test_oracle_equals_the_committed_pillow_decode_on_every_fixture():
  for name in J.names():
    d = J.decode(name)
    assert d.rgb.shape == J.expected(name).shape, name
    assert np.array_equal(d.rgb, J.expected(name)), name


def test_oracle_and_committed_pixels_equal_a_live_pillow_decode():
  Image = pytest.importorskip('PIL.Image')
  for name in J.names():
    live = np.asarray(Image.open(io.BytesIO(J.data(name))).convert('RGB'))
    assert np.array_equal(live, J.expected(name)), name
    assert np.array_equal(live, J.decode(name).rgb), name


def test_info_and_coefficients_equal_the_oracle(lib):
  L = lib.lib()
  for name in J.names():
    d, raw = J.decode(name), J.data(name)
    im = lib.JpegImage()
    lib.check(L.mmt_jpeg_info(raw, len(raw), ctypes.byref(im)))
    assert (im.width, im.height, im.components) == (d.width, d.height, d.components), name
    n = d.components
    assert list(im.h_samp)[:n] == d.h_samp and list(im.v_samp)[:n] == d.v_samp, name
    assert list(im.blocks_w)[:n] == d.blocks_w and list(im.blocks_h)[:n] == d.blocks_h, name
    sizes = [bw * bh * 64 for bw, bh in zip(d.blocks_w, d.blocks_h)]
    assert list(im.coef_offset)[:n] == [sum(sizes[:c]) for c in range(n)] and im.coef_elems == sum(sizes), name
    assert im.pixel_offset == 0
    coef = J.aligned(im.coef_elems + 64, np.int16, fill=0x5555)           # 64 guard elements behind the planes
    q = J.aligned(192, np.uint16, fill=0xFFFF)
    lib.check(L.mmt_jpeg_coefficients(raw, len(raw), ctypes.byref(im), coef.ctypes.data, im.coef_elems, q.ctypes.data))
    assert np.all(coef[im.coef_elems:] == 0x5555), name
    for c in range(n):
      got = coef[im.coef_offset[c]:im.coef_offset[c] + sizes[c]].reshape(d.coef[c].shape)
      assert np.array_equal(got, d.coef[c]), (name, c)
    assert np.array_equal(q.reshape(3, 64), d.qtables), name


def test_pixels_host_equals_the_expected_pixels(lib):
  L = lib.lib()
  for name in J.names():
    images, coef, q, offs, n = J.host_stage(lib, [name])
    out = np.full(n + J.GUARD, J.SENTINEL, dtype=np.uint8)
    work = J.aligned(coef.size, np.uint8, fill=0xFF)
    lib.check(L.mmt_jpeg_pixels_host(1, images, coef.ctypes.data, coef.size, q.ctypes.data, out.ctypes.data, n,
                                     work.ctypes.data, work.size))
    J.check_packed(out, [J.expected(name)], offs)


def test_refusals_name_their_reason(lib):
  L = lib.lib()
  want = {'refuse_progressive.jpg': 'progressive', 'refuse_cmyk.jpg': '4 components', 'refuse_arithmetic.jpg': 'arithmetic',
          'refuse_signature.png': 'decode it on the host'}
  for name in J.REFUSALS:
    raw = J.data(name)
    im = lib.JpegImage()
    assert L.mmt_jpeg_info(raw, len(raw), ctypes.byref(im)) == -2, name          # MMT_E_UNSUPPORTED
    msg = L.mmt_last_error().decode()
    assert msg and want[name] in msg, (name, msg)
  raw = J.data('17x9_420_q75')
  im = lib.JpegImage()
  assert L.mmt_jpeg_info(raw[:40], 40, ctypes.byref(im)) == -1 and L.mmt_last_error()     # truncated: MMT_E_INVALID
  lib.check(L.mmt_jpeg_info(raw, len(raw), ctypes.byref(im)))
  coef, q = J.aligned(im.coef_elems, np.int16), J.aligned(192, np.uint16)
  assert L.mmt_jpeg_coefficients(raw, len(raw) - 9, ctypes.byref(im), coef.ctypes.data, im.coef_elems, q.ctypes.data) == -1
  assert L.mmt_last_error()
  assert L.mmt_jpeg_coefficients(raw, len(raw), ctypes.byref(im), coef.ctypes.data, im.coef_elems - 1, q.ctypes.data) == -1
  assert b'leaves coef' in L.mmt_last_error()


def test_decode_jpeg_images_cpu_batch_equals_per_file_results_for_any_worker_count(lib):
  from mmt_amd import feature_pipeline as fp
  names = list(J.names())
  kinds = (bytes, bytearray, memoryview, lambda b: np.frombuffer(b, dtype=np.uint8))
  blobs = [kinds[i % 4](J.data(n)) for i, n in enumerate(names)]
  pixels, offsets, heights, widths = fp.decode_jpeg_images(blobs, 'cpu', workers=1)
  assert pixels.dtype.is_floating_point is False and pixels.numel() == sum(J.expected(n).size for n in names)
  for i, n in enumerate(names):
    e = J.expected(n)
    assert (int(heights[i]), int(widths[i])) == e.shape[:2]
    got = pixels[int(offsets[i]):int(offsets[i]) + e.size].numpy().reshape(e.shape)
    assert np.array_equal(got, e), n
    one = fp.decode_jpeg_images([J.data(n)], 'cpu')[0].numpy().reshape(e.shape)          # alone, the file gives the same bytes
    assert np.array_equal(one, got), n
  many = fp.decode_jpeg_images(blobs, 'cpu', workers=16)
  huge = fp.decode_jpeg_images(blobs, 'cpu', workers=10 ** 6)   # clamped to 16
  for a, b, c in zip((pixels, offsets, heights, widths), many, huge):
    assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy()) and np.array_equal(a.numpy(), c.numpy())


def test_decode_jpeg_images_refusal_names_the_example(lib):
  from mmt_amd import feature_pipeline as fp
  blobs = [J.data('8x8_444_q90'), J.data('refuse_progressive.jpg'), J.data('9x3_420_q75')]
  with pytest.raises(ValueError, match=r'data\[1\].*progressive'):
    fp.decode_jpeg_images(blobs, 'cpu')
  cut = J.data('33x31_420_q75')[:-20]
  with pytest.raises(ValueError, match=r'data\[2\]'):
    fp.decode_jpeg_images([blobs[0], blobs[2], cut], 'cpu', workers=2)
  with pytest.raises(ValueError, match='empty'):
    fp.decode_jpeg_images([], 'cpu')


def test_decode_image_features_takes_encoded_bytes_on_cpu(lib):
  import torch
  from mmt_amd import feature_pipeline as fp
  cfg = types.SimpleNamespace(is_training=False, image_size=32, patch_size=16, output_channel_bits=3)
  names = ['33x31_420_q75', '9x2_422_q50', '48x80_444_q90', '17x9_grey_q80', '1x1_420_q75']
  got = fp.decode_image_features(cfg, [J.data(n) for n in names], keep_unnormalized=True, device='cpu')
  ref = fp.decode_image_features(cfg, [torch.from_numpy(J.expected(n).copy()) for n in names], keep_unnormalized=True)
  assert set(got) == set(ref)
  for k in ref:
    if isinstance(ref[k], torch.Tensor):
      assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), k
    else:
      assert got[k] == ref[k], k
  pf = fp.images_to_patch_features([J.data(n) for n in names], 32, 16, device='cpu')
  assert torch.equal(pf['patch_embeddings'], ref['patch_embeddings'])


def test_sanitizer_program_of_the_host_stage():
  """`make asan-jpeg` (csrc/Makefile): the host side of jpeg_decode.hip under AddressSanitizer + UBSan, driven by a C
  program over the fixtures, their truncations and corruptions, and wrong metadata.  CPU only."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  csrc = os.path.join(ROOT, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-jpeg'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'jpeg asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
