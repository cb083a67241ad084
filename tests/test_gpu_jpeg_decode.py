"""mmt_jpeg_pixels on the GPU, through the ctypes boundary on caller-owned buffers, against the committed Pillow decodes
of tests/golden/jpeg (tests/_jpeg_cases.py).  Parity is bit for bit: no tolerance.  The images sit at mostly odd pixel
offsets with gaps between them and a guard behind the buffer, pixels_out is pre-filled with a sentinel, and every
comparison covers the whole buffer, so a byte written outside an image fails the test that wrote it.  The metadata is
always the library's own: the clamping is exercised on the host under the sanitizer (`make asan-jpeg`)."""
import types

import numpy as np
import pytest
import torch

from tests import _jpeg_cases as J

pytestmark = pytest.mark.gpu


class Call:
  """Device buffers of one batch of fixtures; run() is one mmt_jpeg_pixels on them."""

  def __init__(self, names, workspace_fill=None):
    from mmt_amd import _lib
    self.lib, self.names = _lib, list(names)
    images, coef, qtables, self.offsets, self.n = J.host_stage(_lib, self.names)
    self.B, self.coef_elems = len(self.names), coef.size
    self.images = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8).cuda()
    self.coef = torch.from_numpy(coef.copy()).cuda()
    self.qtables = torch.from_numpy(qtables.view(np.int16).copy()).cuda()
    self.out = torch.full((self.n + J.GUARD,), J.SENTINEL, dtype=torch.uint8, device='cuda')
    self.need = _lib.lib().mmt_jpeg_workspace_bytes(self.coef_elems)
    self.ws = torch.empty(self.need, dtype=torch.uint8, device='cuda')
    if workspace_fill is not None:
      self.ws.fill_(workspace_fill)

  def run(self):
    self.lib.check(self.lib.lib().mmt_jpeg_pixels(
        self.B, self.images.data_ptr(), self.coef.data_ptr(), self.coef_elems, self.qtables.data_ptr(), self.out.data_ptr(),
        self.n, self.ws.data_ptr(), self.need, torch.cuda.current_stream().cuda_stream))

  def result(self):
    torch.cuda.synchronize()
    return self.out.cpu().numpy()

  def check(self):
    J.check_packed(self.result(), [J.expected(n) for n in self.names], self.offsets)


MODES = sorted({n.split('_', 1)[1] for n in J.names()})


@pytest.mark.parametrize('mode', MODES)
def test_every_fixture_alone(mode):
  """One call per file, the file at an odd pixel offset.  The 96 x 100 file (mode 420_q75) takes several steps of the
  IDCT pass and more than one workgroup of each pass."""
  for name in J.names():
    if name.split('_', 1)[1] == mode:
      c = Call([name])
      c.run()
      c.check()


def shuffled():
  names = [n for n in J.names() if n != J.LARGE]
  order = np.random.default_rng(20214).permutation(len(names))
  names = [names[i] for i in order]
  return names[:len(names) // 2] + [J.LARGE] + names[len(names) // 2:]


def test_all_fixtures_in_one_call_in_a_shuffled_order():
  names = shuffled()
  assert len(names) == len(J.names()) and names.index(J.LARGE) == (len(names) - 1) // 2
  c = Call(names)
  c.run()
  c.check()


def test_repeatable_and_independent_of_the_workspace_contents():
  """Two calls on the same buffers are bit-identical, and a workspace pre-filled with 0x00 or 0xFF gives the same bytes:
  every plane byte the colour pass reads was written by the IDCT pass of the same call."""
  names = shuffled()[30:62]
  first = Call(names)
  first.run()
  a = first.result().copy()
  first.run()
  assert np.array_equal(first.result(), a)
  for fill in (0x00, 0xFF):
    other = Call(names, workspace_fill=fill)
    other.run()
    assert np.array_equal(other.result(), a), fill
  J.check_packed(a, [J.expected(n) for n in names], first.offsets)


def test_recorded_graph_follows_new_coefficients():
  """The call recorded once with torch.cuda.graph; the coefficients and tables of a second set of files of the same
  shapes and sampling (another quality and other content) are copied in place and the replay gives their pixels."""
  first = ['48x80_420_q75', '17x9_420_q75', '33x31_420_q75', '9x2_420_q75']
  second = [n.replace('420_q75', '420_q100_opt') for n in first]
  c, other = Call(first), Call(second)
  assert bytes(c.images.cpu().numpy()) == bytes(other.images.cpu().numpy())          # the same metadata
  c.run()                                                             # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    c.run()
  graph.replay()
  c.check()
  c.coef.copy_(other.coef)
  c.qtables.copy_(other.qtables)
  c.out.fill_(J.SENTINEL)
  graph.replay()
  J.check_packed(c.result(), [J.expected(n) for n in second], c.offsets)
  assert any(not np.array_equal(J.expected(a), J.expected(b)) for a, b in zip(first, second))


def test_decode_jpeg_images_on_the_device_equals_the_expected_pixels():
  from mmt_amd import feature_pipeline as fp
  names = shuffled()
  pixels, offsets, heights, widths = fp.decode_jpeg_images([J.data(n) for n in names], 'cuda', workers=4)
  assert pixels.is_cuda and offsets.is_cuda and heights.dtype == torch.int32 and offsets.dtype == torch.int64
  host = pixels.cpu().numpy()
  for i, n in enumerate(names):
    e = J.expected(n)
    assert (int(heights[i]), int(widths[i])) == e.shape[:2]
    assert np.array_equal(host[int(offsets[i]):int(offsets[i]) + e.size], e.reshape(-1)), n
  assert host.size == sum(J.expected(n).size for n in names)


def test_decode_image_features_takes_encoded_bytes_on_the_device():
  """decode_image_features on encoded bytes equals the same call on the oracle-decoded tensors: with is_training false,
  and once with use_rand_aug and a fixed generator -- the packed tuple feeds RandAugment unchanged."""
  from mmt_amd import feature_pipeline as fp
  names = ['48x80_420_q75', '33x31_444_q90', '24x17_422_q50', '17x9_grey_q80', '9x2_420_q30_rst1', J.LARGE, '1x1_422_q95_rst2']
  blobs = [J.data(n) for n in names]
  tensors = [torch.from_numpy(J.decode(n).rgb.copy()).cuda() for n in names]
  for training in (False, True):
    cfg = types.SimpleNamespace(is_training=training, use_rand_aug=training, image_size=32, patch_size=16, output_channel_bits=3)
    got = fp.decode_image_features(cfg, blobs, generator=torch.Generator('cuda').manual_seed(5), keep_unnormalized=True, device='cuda')
    ref = fp.decode_image_features(cfg, tensors, generator=torch.Generator('cuda').manual_seed(5), keep_unnormalized=True)
    assert set(got) == set(ref)
    for k in ref:
      if isinstance(ref[k], torch.Tensor):
        assert got[k].is_cuda and torch.equal(got[k], ref[k]), (training, k)
      else:
        assert got[k] == ref[k], (training, k)
