"""mmt_jpeg_entropy on the GPU, through the ctypes boundary on caller-owned device buffers, against the merged host path
(mmt_jpeg_coefficients; tests/_jpeg_entropy_cases.py) and, behind mmt_jpeg_pixels, against the committed Pillow decodes.
Parity is bit for bit: coef is pre-filled with 0x5555 with a guard behind it and compared whole, so a coefficient
written outside a plane fails the test that wrote it.  Parity cases run at the plan's worst-case max_rounds, at which
no file may fall back.  Corrupt inputs are status tests: the same bounded code has walked them on the host under the
sanitizer (`make asan-jpeg-entropy`), and the device must give the same words as mmt_jpeg_entropy_host."""
import types

import numpy as np
import pytest
import torch

from tests import _jpeg_cases as J
from tests import _jpeg_entropy_cases as E

pytestmark = pytest.mark.gpu


def default_size():
  from mmt_amd import feature_pipeline as fp
  return fp.JPEG_ENTROPY_SUBSEQ_BYTES


class Call:
  """Device buffers of one batch; run() is one mmt_jpeg_entropy on them."""

  def __init__(self, items, subseq_bytes, max_rounds=None, workspace_fill=None):
    from mmt_amd import _lib
    self.lib, self.items = _lib, list(items)
    self.images_h, self.want, self.want_q, self.offsets, self.n, self.ok = E.host_stage(_lib, self.items)
    self.plans = E.Plans(_lib, self.items, self.images_h, subseq_bytes)
    self.coef_elems = self.want.size
    self.max_rounds = self.plans.worst_rounds if max_rounds is None else max_rounds
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()
    self.images = torch.frombuffer(bytearray(bytes(self.images_h)), dtype=torch.uint8).cuda()
    self.scans = torch.frombuffer(bytearray(bytes(self.plans.scans)), dtype=torch.uint8).cuda()
    self.bytes, self.huff, self.qtables = up(self.plans.bytes), up(self.plans.huff), up(self.plans.qtables)
    self.segments, self.subseqs = up(self.plans.segments), up(self.plans.subseqs)
    self.coef = torch.full((self.coef_elems + 64,), E.COEF_FILL, dtype=torch.int16, device='cuda')
    self.status = torch.full((self.plans.B,), -99, dtype=torch.int32, device='cuda')
    self.need = self.plans.workspace_bytes(_lib, self.max_rounds)
    self.ws = torch.empty(self.need, dtype=torch.uint8, device='cuda')
    if workspace_fill is not None:
      self.ws.fill_(workspace_fill)

  def load(self, other):
    """The bytes and plans of another batch of the same shapes, in place."""
    for mine, theirs in ((self.bytes, other.bytes), (self.scans, other.scans), (self.huff, other.huff), (self.qtables, other.qtables),
                         (self.segments, other.segments), (self.subseqs, other.subseqs)):
      mine[:theirs.numel()].copy_(theirs)

  def run(self):
    self.lib.check(self.lib.lib().mmt_jpeg_entropy(*self.plans.args(
        self.images.data_ptr(), self.bytes.data_ptr(), self.scans.data_ptr(), self.huff.data_ptr(), self.segments.data_ptr(),
        self.subseqs.data_ptr(), self.max_rounds, self.coef.data_ptr(), self.coef_elems, self.status.data_ptr(), self.ws.data_ptr(),
        self.need), torch.cuda.current_stream().cuda_stream))

  def result(self):
    torch.cuda.synchronize()
    return self.coef.cpu().numpy(), self.status.cpu().numpy()

  def check(self):
    """Every file decoded on the device (no fallback), coef and guard equal to the host decode, qtables equal; then
    mmt_jpeg_pixels on the device's coefficients gives the committed pixels of the fixtures."""
    assert self.plans.rc == [0] * len(self.items), self.plans.messages
    coef, status = self.result()
    assert status.tolist() == [0] * len(self.items), status.tolist()
    bad = np.nonzero(coef[:self.coef_elems] != self.want)[0]
    assert bad.size == 0, f'{bad.size} coefficients differ, first at {bad[0]}: got {coef[bad[0]]}, want {self.want[bad[0]]}'
    assert np.all(coef[self.coef_elems:] == E.COEF_FILL)
    assert np.array_equal(self.plans.qtables, self.want_q)
    if all(isinstance(it, str) for it in self.items):
      L = self.lib.lib()
      out = torch.full((self.n + J.GUARD,), J.SENTINEL, dtype=torch.uint8, device='cuda')
      need = L.mmt_jpeg_workspace_bytes(self.coef_elems)
      ws = torch.empty(need, dtype=torch.uint8, device='cuda')
      self.lib.check(L.mmt_jpeg_pixels(len(self.items), self.images.data_ptr(), self.coef.data_ptr(), self.coef_elems, self.qtables.data_ptr(),
                                       out.data_ptr(), self.n, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
      torch.cuda.synchronize()
      J.check_packed(out.cpu().numpy(), [J.expected(n) for n in self.items], self.offsets)


def shuffled():
  names = [n for n in J.names() if n != J.LARGE]
  order = np.random.default_rng(20216).permutation(len(names))
  names = [names[i] for i in order]
  return names[:len(names) // 2] + [J.LARGE] + names[len(names) // 2:]


MODES = sorted({n.split('_', 1)[1] for n in J.names()})


@pytest.mark.parametrize('size', ['8', 'default'])
@pytest.mark.parametrize('mode', MODES)
def test_every_fixture_alone(mode, size):
  sb = 8 if size == '8' else default_size()
  for name in J.names():
    if name.split('_', 1)[1] == mode:
      c = Call([name], sb)
      c.run()
      c.check()


@pytest.mark.parametrize('size', ['8', 'default'])
def test_all_fixtures_in_one_call_in_a_shuffled_order(size):
  sb = 8 if size == '8' else default_size()
  names = shuffled()
  assert len(names) == len(J.names())
  c = Call(names, sb)
  if sb == 8:
    # 48x80_444_q90 spans at least three workgroups: states cross workgroup boundaries between launches and the offsets
    # come from the cross-workgroup prefix sums
    scan = c.plans.scans[names.index('48x80_444_q90')]
    assert len(J.data('48x80_444_q90')) == 7799 and scan.n_segments == 1
    assert -(-scan.n_subseq // 256) >= 3, scan.n_subseq           # 256 subsequences per workgroup (kEntThreads, jpeg_entropy.h)
  c.run()
  c.check()


def test_dense_stuffing_on_the_device():
  for sb in (8, default_size()):
    c = Call([E.dense_stuffing(), '48x80_444_q90'], sb)
    c.run()
    c.check()


@pytest.mark.parametrize('case', ['one_round', 'corrupt'])
def test_device_equals_the_host_variant_status_words_included(case):
  """The same plans through mmt_jpeg_entropy and mmt_jpeg_entropy_host: the same coefficients over the whole buffer and
  the same status words, for max_rounds = 1 (not converged) and for the truncated and the inverted-byte file between
  two good ones."""
  from mmt_amd import _lib
  if case == 'one_round':
    items, sb, rounds = ['48x80_444_q90', '9x3_444_q90', '33x31_420_q75'], 8, 1
  else:
    items, sb, rounds = ['33x31_422_q50', E.truncated_scan(), E.flipped_byte(_lib), '48x80_420_q30_rst1'], 8, None
  c = Call(items, sb, max_rounds=rounds)
  c.run()
  coef, status = c.result()
  want, want_status = E.entropy_host(_lib, c.plans, c.images_h, c.coef_elems, c.max_rounds)
  assert status.tolist() == want_status.tolist(), (status.tolist(), want_status.tolist())
  if case == 'one_round':
    assert status[0] == _lib.MMT_JPEG_ST_NOT_CONVERGED
  else:
    assert status[0] == 0 and status[3] == 0 and 0 < status[1] < 16 and 0 < status[2] < 16
    good = E.planes_mask(c.images_h, c.coef_elems, (0, 3))
    assert np.array_equal(coef[:c.coef_elems][good], c.want[good])
  assert np.array_equal(coef, want)


def test_repeatable_and_independent_of_the_workspace_contents():
  names = shuffled()[20:52]
  first = Call(names, default_size())
  first.run()
  a, sa = (x.copy() for x in first.result())
  first.run()
  b, sb = first.result()
  assert np.array_equal(a, b) and np.array_equal(sa, sb)
  for fill in (0x00, 0xFF):
    other = Call(names, default_size(), workspace_fill=fill)
    other.run()
    c, sc = other.result()
    assert np.array_equal(a, c) and np.array_equal(sa, sc), fill
  first.check()


def test_recorded_graph_follows_new_bytes_and_plans():
  """The call recorded once with torch.cuda.graph on buffers sized for the larger of two sets of equal shapes; the second
  set's bytes and plans are copied in place and the replay gives its coefficients."""
  small = ['48x80_420_q75', '17x9_420_q75', '33x31_420_q75', '9x2_420_q75']
  large = [n.replace('420_q75', '420_q100_opt') for n in small]
  sb = default_size()
  c, other = Call(large, sb), Call(small, sb)
  assert bytes(c.images.cpu().numpy()) == bytes(other.images.cpu().numpy())          # the same metadata
  assert c.bytes.numel() >= other.bytes.numel() and c.plans.n_subseq >= other.plans.n_subseq and c.plans.n_segments >= other.plans.n_segments
  assert c.plans.max_subseq >= other.plans.max_subseq and c.max_rounds >= other.plans.worst_rounds
  c.run()                                                             # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    c.run()
  c.coef.fill_(E.COEF_FILL)
  graph.replay()
  c.check()
  c.load(other)
  c.coef.fill_(E.COEF_FILL)
  c.status.fill_(-99)
  graph.replay()
  coef, status = c.result()
  assert status.tolist() == [0] * 4
  assert np.array_equal(coef[:c.coef_elems], other.want) and np.all(coef[c.coef_elems:] == E.COEF_FILL)
  assert not np.array_equal(c.want, other.want)


def test_decode_jpeg_images_with_device_entropy_equals_the_expected_pixels():
  from mmt_amd import feature_pipeline as fp
  names = shuffled()
  blobs = [J.data(n) for n in names]
  blobs.insert(40, E.three_scans())                              # refused by the plan: the host decode takes it
  names.insert(40, '17x9_444_q90')
  pixels, offsets, heights, widths = fp.decode_jpeg_images(blobs, 'cuda', workers=4, entropy='device')
  assert pixels.is_cuda and offsets.is_cuda and heights.dtype == torch.int32 and offsets.dtype == torch.int64
  host = pixels.cpu().numpy()
  for i, n in enumerate(names):
    e = J.expected(n)
    assert (int(heights[i]), int(widths[i])) == e.shape[:2]
    assert np.array_equal(host[int(offsets[i]):int(offsets[i]) + e.size], e.reshape(-1)), n
  assert host.size == sum(J.expected(n).size for n in names)
  one = fp.decode_jpeg_images(blobs, 'cuda', entropy='device', subseq_bytes=8, max_rounds=1)[0]      # most files fall back
  auto = fp.decode_jpeg_images(blobs, 'cuda', entropy='auto')[0]
  assert torch.equal(one, pixels) and torch.equal(auto, pixels)


def test_decode_image_features_with_device_entropy_equals_host_entropy():
  from mmt_amd import feature_pipeline as fp
  names = ['48x80_420_q75', '33x31_444_q90', '24x17_422_q50', '17x9_grey_q80', '9x2_420_q30_rst1', J.LARGE, '1x1_422_q95_rst2']
  blobs = [J.data(n) for n in names]
  for training in (False, True):
    cfg = types.SimpleNamespace(is_training=training, use_rand_aug=training, image_size=32, patch_size=16, output_channel_bits=3)
    got = fp.decode_image_features(cfg, blobs, generator=torch.Generator('cuda').manual_seed(5), keep_unnormalized=True, device='cuda',
                                   entropy='device')
    ref = fp.decode_image_features(cfg, blobs, generator=torch.Generator('cuda').manual_seed(5), keep_unnormalized=True, device='cuda',
                                   entropy='host')
    assert set(got) == set(ref)
    for k in ref:
      if isinstance(ref[k], torch.Tensor):
        assert got[k].is_cuda and torch.equal(got[k], ref[k]), (training, k)
      else:
        assert got[k] == ref[k], (training, k)
