"""mmt_png_pixels on the GPU, through the ctypes boundary on caller-owned buffers, against the committed Pillow decodes
of tests/golden/png (tests/_png_cases.py).  Parity is bit for bit: no tolerance.  pixels_out, the workspace and the
scanlines sit inside larger buffers pre-filled with a sentinel, and every comparison covers the whole buffer, so a byte
written outside an image fails the test that wrote it."""
import types

import numpy as np
import pytest
import torch

from tests import _jpeg_cases as J
from tests import _png_cases as P

pytestmark = pytest.mark.gpu


class Call:
  """Device buffers of one batch of fixtures; run() is one mmt_png_pixels on them.  pixels_out and the workspace are the
  middle of buffers with GUARD sentinel bytes on both sides."""

  def __init__(self, names, gap=0):
    from mmt_amd import _lib
    self.lib, self.names = _lib, list(names)
    images, raw, pal, self.offsets, self.n = P.host_stage(_lib, [P.data(n) for n in self.names])
    if gap:                                                     # images apart from each other, at odd offsets
      self.offsets = [o + (i + 1) * gap for i, o in enumerate(self.offsets)]
      for i, o in enumerate(self.offsets):
        images[i].pixel_offset = o
      self.n += (len(self.names) + 1) * gap
    self.host_images = images
    self.B, self.raw_bytes = len(self.names), raw.size
    self.images = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8).cuda()
    self.raw = torch.from_numpy(raw.copy()).cuda()
    self.pal = torch.from_numpy(pal.copy()).cuda()
    self.out_all = torch.full((self.n + 2 * P.GUARD,), P.SENTINEL, dtype=torch.uint8, device='cuda')
    self.out = self.out_all[P.GUARD:P.GUARD + self.n]
    self.need = _lib.lib().mmt_png_workspace_bytes(self.raw_bytes)
    assert self.need == self.raw_bytes
    self.ws_all = torch.full((self.need + 2 * P.GUARD,), P.SENTINEL, dtype=torch.uint8, device='cuda')
    self.ws = self.ws_all[P.GUARD:P.GUARD + self.need]

  def set_images(self, images):
    self.images = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8).cuda()

  def run(self):
    self.lib.check(self.lib.lib().mmt_png_pixels(
        self.B, self.images.data_ptr(), self.raw.data_ptr(), self.raw_bytes, self.pal.data_ptr(), self.out.data_ptr(), self.n,
        self.ws.data_ptr(), self.need, torch.cuda.current_stream().cuda_stream))

  def result(self):
    """The pixels and the GUARD bytes behind them; the bytes in front and around the workspace are checked here."""
    torch.cuda.synchronize()
    host, ws = self.out_all.cpu().numpy(), self.ws_all.cpu().numpy()
    assert np.all(host[:P.GUARD] == P.SENTINEL) and np.all(host[P.GUARD + self.n:] == P.SENTINEL)
    assert np.all(ws[:P.GUARD] == P.SENTINEL) and np.all(ws[P.GUARD + self.need:] == P.SENTINEL)
    return host[P.GUARD:]

  def check(self):
    """Every image equals its expected pixels and every byte between and behind the images is the sentinel."""
    got = self.result()
    want = np.full(got.size, P.SENTINEL, dtype=np.uint8)
    for n, o in zip(self.names, self.offsets):
      e = P.expected(n)
      want[o:o + e.size] = e.reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (self.names if len(self.names) < 4 else len(self.names), int(bad[0]), bad.size)


def group_of(name):
  return name.split('_')[1] if name not in P.EXTRA else 'extra'


@pytest.mark.parametrize('group', P.KINDS + ('extra',))
def test_every_fixture_alone(group):
  """One call per file, the file at an odd pixel offset."""
  for name in P.names():
    if group_of(name) == group:
      c = Call([name], gap=7)
      c.run()
      c.check()


def shuffled():
  names = list(P.names())
  return [names[i] for i in np.random.default_rng(20215).permutation(len(names))]


def test_all_fixtures_in_one_call_in_a_shuffled_order_with_gaps():
  """No image borrows a neighbour's geometry, and the bytes between the images stay the sentinel."""
  c = Call(shuffled(), gap=5)
  c.run()
  c.check()


def test_recorded_graph_replays_from_the_same_raw_and_leaves_it_unchanged():
  """The call recorded once with torch.cuda.graph and replayed twice with no new upload: the same pixels each time, so raw
  is not modified -- and raw is compared before and after too.  A workspace full of other bytes changes nothing."""
  c = Call(shuffled()[:40], gap=3)
  before = c.raw.cpu().numpy().copy()
  c.run()                                                             # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    c.run()
  for fill in (0x00, 0xFF):
    c.out.fill_(P.SENTINEL)
    c.ws.fill_(fill)
    graph.replay()
    c.check()
  assert np.array_equal(c.raw.cpu().numpy(), before)


def test_wrong_metadata_is_clamped_into_the_buffers():
  """The wrong-metadata cases of the sanitizer driver that the clamping rule defines: sizes and offsets that leave the
  buffers, another depth or colour type, filter bytes above 4.  The call returns, writes nothing outside pixels_out or the
  workspace, and the image whose metadata is right keeps its pixels where the wrong one cannot reach them."""
  names = ['33x70_rgb8_f3_i0_fixed', '65x5_p1_f3_i1_stored']
  assert all(n in P.names() for n in names)
  c = Call(names)
  good = c.host_images
  big = 1 << 40
  cases = [dict(raw_offset=-1), dict(raw_offset=big), dict(raw_bytes=big), dict(raw_bytes=-5), dict(raw_bytes=3),
           dict(pixel_offset=-7), dict(pixel_offset=big), dict(pixel_offset=c.n - 4), dict(width=0), dict(width=-3, height=2 ** 31 - 1),
           dict(width=2 ** 31 - 1, height=2 ** 31 - 1), dict(width=1000, height=1), dict(bit_depth=1), dict(bit_depth=16, color_type=0),
           dict(color_type=2), dict(color_type=6, bit_depth=7), dict(interlace=0), dict(interlace=9, height=200), dict(palette_entries=-1),
           dict(palette_entries=10 ** 6)]
  for case in cases:
    images = (c.lib.PngImage * 2)()
    images[0], images[1] = good[0], good[1]
    for k, v in case.items():
      setattr(images[1], k, v)
    c.set_images(images)
    c.out.fill_(P.SENTINEL)
    c.run()
    c.result()                                                  # the guards around pixels_out and the workspace
  # filter bytes above 4 count as None
  c.set_images(good)
  raw = c.raw.cpu().numpy().copy()
  d = P.decode(names[0])
  assert d.interlace == 0
  step = 1 + 3 * d.width
  for r, v in enumerate((5, 6, 77, 255)):
    raw[good[0].raw_offset + r * step] = v
  c.raw = torch.from_numpy(raw).cuda()
  c.out.fill_(P.SENTINEL)
  c.run()
  got = c.result()
  e = P.expected(names[1])
  assert np.array_equal(got[c.offsets[1]:c.offsets[1] + e.size], e.reshape(-1))        # the other image is untouched by it
  as_none = raw.copy()
  for r in range(4):
    as_none[good[0].raw_offset + r * step] = 0
  c.raw = torch.from_numpy(as_none).cuda()
  c.out.fill_(P.SENTINEL)
  c.run()
  assert np.array_equal(c.result(), got)


def test_decode_images_mixed_on_the_device_equals_the_cpu_result():
  from mmt_amd import feature_pipeline as fp
  pn, jn = shuffled()[:12], ['48x80_420_q75', '17x9_grey_q80', '9x3_444_q90', '33x31_422_q50']
  blobs = [P.data(n) for n in pn[:5]] + [J.data(jn[0])] + [P.data(n) for n in pn[5:9]] + [J.data(n) for n in jn[1:]] + [P.data(n) for n in pn[9:]]
  ref = fp.decode_images(blobs, 'cpu')
  for entropy in ('host', 'device'):
    got = fp.decode_images(blobs, 'cuda', entropy=entropy, workers=4)
    assert got[0].is_cuda and got[1].dtype == torch.int64 and got[2].dtype == torch.int32
    for a, b in zip(got[1:], ref[1:]):
      assert torch.equal(a.cpu(), b), entropy
    host = got[0].cpu()
    for i in range(len(blobs)):
      o, n = int(ref[1][i]), int(ref[2][i]) * int(ref[3][i]) * 3
      assert torch.equal(host[o:o + n], ref[0][o:o + n]), (entropy, i)
  alone = fp.decode_images([P.data(n) for n in pn], 'cuda')
  for i, n in enumerate(pn):
    e = P.expected(n)
    assert np.array_equal(alone[0][int(alone[1][i]):int(alone[1][i]) + e.size].cpu().numpy(), e.reshape(-1)), n


def test_decode_image_features_takes_png_bytes_on_the_device():
  """decode_image_features on PNG bytes equals the same call on the decoded tensors: with is_training false, and once with
  use_rand_aug and a fixed generator."""
  from mmt_amd import feature_pipeline as fp
  names = ['33x70_rgb8_f3_i0_fixed', '16x200_g2_f1_i1_fixed', '130x7_p1_f4_i0_dynamic', '33x70_p8_f2_i1_fixed', '1x1_g8_f1_i0_fixed', 'pillow_palette',
           'short_palette']
  assert all(n in P.names() for n in names)
  blobs = [P.data(n) for n in names]
  tensors = [torch.from_numpy(P.expected(n).copy()).cuda() for n in names]
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
