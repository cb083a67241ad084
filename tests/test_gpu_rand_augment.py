"""mmt_rand_augment on the GPU, through the ctypes boundary on caller-owned buffers, against the numpy oracle of
tests/_augment_cases.py.  Parity is bit-exact: no tolerance.  The images sit at odd offsets with gaps between them and
a guard behind the buffer, out_pixels is pre-filled with a sentinel, and every comparison covers the whole buffer, so
a byte written outside an image fails the test that wrote it."""
import numpy as np
import pytest
import torch

from tests import _augment_cases as ac

pytestmark = pytest.mark.gpu


class Call:
  """Device buffers of one packed batch; run() is one mmt_rand_augment on them."""

  def __init__(self, images, ids, arg, out_shift=0, workspace_fill=None):
    from mmt_amd import _lib
    self.lib = _lib
    pixels, offsets, heights, widths, n = ac.pack(images)
    self.n, self.B, self.host_offsets = n, len(images), offsets
    self.pixels = torch.from_numpy(pixels).cuda()
    self.offsets, self.heights, self.widths = (torch.from_numpy(x).cuda() for x in (offsets, heights, widths))
    self.op = torch.tensor(ids, dtype=torch.int32).cuda()
    self.arg = torch.from_numpy(np.ascontiguousarray(arg, dtype=np.float32)).cuda()
    self.out_store = torch.full((n + ac.GUARD + out_shift,), ac.SENTINEL, dtype=torch.uint8, device='cuda')
    self.out = self.out_store[out_shift:]          # out_shift = 1: source and destination differ in alignment
    self.need = _lib.lib().mmt_rand_augment_workspace_bytes(self.B)
    self.ws = torch.empty(self.need, dtype=torch.uint8, device='cuda')
    if workspace_fill is not None:
      self.ws.fill_(workspace_fill)

  def run(self):
    self.lib.check(self.lib.lib().mmt_rand_augment(
        self.B, self.pixels.data_ptr(), self.n, self.offsets.data_ptr(), self.heights.data_ptr(), self.widths.data_ptr(),
        self.op.data_ptr(), self.arg.data_ptr(), self.out.data_ptr(), self.ws.data_ptr(), self.need,
        torch.cuda.current_stream().cuda_stream))

  def result(self):
    torch.cuda.synchronize()
    return self.out.cpu().numpy()


def case(op, variant):
  images = ac.image_set()
  arg = np.stack([ac.case_args(op, im.shape[0], im.shape[1], variant) for im in images])
  want = [ac.expected(b, op, variant) for b in range(len(images))]
  return images, [op] * len(images), arg, want


@pytest.mark.parametrize('op', ac.ALL_IDS)
def test_each_operation_over_the_image_set(op):
  """Every image of the set under one operation, for each argument variant of tests/_augment_cases.py; gaps and guard
  keep their sentinel.  The 96 x 100 image spans three chunks of the statistics pass (STATS_CHUNK pixels each)."""
  for variant in range(3 if op in ac.TEST_ARGS or op in ac.AFFINE else 1):
    images, ids, arg, want = case(op, variant)
    c = Call(images, ids, arg)
    c.run()
    ac.check_packed(c.result(), want, c.host_offsets, c.n)


def mixed_batch():
  images = list(ac.image_set())
  picks = [9, 8, 5, 4, 9, 7, 3, 2, 1, 0, 6, 6, 5, 8, 4]              # 15 images; the large one under Equalize and Contrast,
  ids = [1, 0, 2, 3, 6, 5, 4, 8, 7, -1, 9, 10, 11, 12, 13]           # the narrow-range one under AutoContrast
  assert sorted(ids) == ac.ALL_IDS
  chosen = [images[k] for k in picks]
  arg = np.stack([ac.case_args(i, im.shape[0], im.shape[1], 1) for i, im in zip(ids, chosen)])
  want = [ac.expected(k, i, 1) for k, i in zip(picks, ids)]
  return chosen, ids, arg, want


def test_fifteen_images_fifteen_ids_in_one_call():
  images, ids, arg, want = mixed_batch()
  c = Call(images, ids, arg)
  c.run()
  ac.check_packed(c.result(), want, c.host_offsets, c.n)


def test_ids_outside_the_list_copy_the_image():
  images = list(ac.image_set())[3:8]
  ids = [14, -2, 1 << 30, -(1 << 31), 255]
  c = Call(images, ids, np.full((5, 8), 3.0, dtype=np.float32))
  c.run()
  ac.check_packed(c.result(), images, c.host_offsets, c.n)


def test_repeatable_and_independent_of_the_workspace_contents():
  """Two calls on the same buffers are bit-identical, and a workspace pre-filled with 0xFF (or 0x00) gives the same
  bytes: the call clears what it uses."""
  images, ids, arg, want = mixed_batch()
  first = Call(images, ids, arg)
  first.run()
  a = first.result().copy()
  first.run()                                                         # the histograms of the first call are still in the workspace
  assert np.array_equal(first.result(), a)
  for fill in (0xFF, 0x00):
    other = Call(images, ids, arg, workspace_fill=fill)
    other.run()
    assert np.array_equal(other.result(), a), fill
  ac.check_packed(a, want, first.host_offsets, first.n)


def test_destination_with_another_alignment():
  """out_pixels one byte off the source's alignment: the byte stream of the table operations takes its scalar form."""
  images, ids, arg, want = mixed_batch()
  c = Call(images, ids, arg, out_shift=1)
  c.run()
  ac.check_packed(c.result(), want, c.host_offsets, c.n)
  assert int(c.out_store[0]) == ac.SENTINEL


def test_overlap_is_refused_on_device_pointers():
  images, ids, arg, _ = mixed_batch()
  c = Call(images, ids, arg)
  c.out = c.pixels
  with pytest.raises(c.lib.MmtError, match='overlaps'):
    c.run()


def test_recorded_graph_follows_new_values():
  """One call recorded with torch.cuda.graph on a single stream; op, arg and the pixels are overwritten in place and the
  replay is compared with the oracle for the new values (the metadata keeps its place: same sizes, another order of ids)."""
  images, ids, arg, want = mixed_batch()
  c = Call(images, ids, arg)
  c.run()                                                             # warm-up outside the capture
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    c.run()
  graph.replay()
  ac.check_packed(c.result(), want, c.host_offsets, c.n)
  new_ids = ids[1:] + ids[:1]
  new_images = [np.ascontiguousarray(255 - im) for im in images]
  new_arg = np.stack([ac.case_args(i, im.shape[0], im.shape[1], 0) for i, im in zip(new_ids, new_images)])
  c.op.copy_(torch.tensor(new_ids, dtype=torch.int32))
  c.arg.copy_(torch.from_numpy(new_arg))
  c.pixels.copy_(torch.from_numpy(ac.pack(new_images)[0]))
  c.out_store.fill_(ac.SENTINEL)
  graph.replay()
  new_want = [ac.augment(im, i, a) for im, i, a in zip(new_images, new_ids, new_arg)]
  ac.check_packed(c.result(), new_want, c.host_offsets, c.n)
  assert any(not np.array_equal(a, b) for a, b in zip(want, new_want))


def test_python_entries_equal_their_cpu_paths():
  """rand_augment and decode_image_features on device tensors against the same functions on CPU tensors: the
  augmentation bit-equal, the front end's outputs inside the bounds of check_outputs (tests/_cases.py) around the
  float64 restatement of the augmented images."""
  from mmt_amd import configs
  from mmt_amd import feature_pipeline as fp
  from tests._cases import check_outputs
  images, ids, arg, want = mixed_batch()
  op_t, arg_t = torch.tensor(ids, dtype=torch.int32), torch.from_numpy(arg)
  cpu = fp.rand_augment([torch.from_numpy(im.copy()) for im in images], op_t, arg_t)
  dev = fp.rand_augment([torch.from_numpy(im.copy()).cuda() for im in images], op_t.cuda(), arg_t.cuda())
  for a, b in zip(cpu, dev):
    assert b.is_cuda and torch.equal(a, b.cpu())
  for b, im in enumerate(want):
    o = int(cpu[1][b])
    assert np.array_equal(cpu[0][o:o + im.size].numpy(), im.reshape(-1))
  # decode_image_features: the draws of the device generator, replayed through the public functions.  Images of 400
  # pixels and more, so that a translation by 100 pixels leaves no patch constant (a constant 128 sits on a bin edge
  # of the label ids in every channel, and check_outputs leaves out at most 2 % of the patches).
  rng = np.random.default_rng(ac.SEED + 1)
  big = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((400, 420), (431, 407), (405, 450), (440, 400), (412, 433), (420, 415))]
  cfg = configs.MmtPretrainDataConfig(is_training=True, use_rand_aug=True, image_size=32, patch_size=16)
  dev_images = [torch.from_numpy(im).cuda() for im in big]
  out = fp.decode_image_features(cfg, dev_images, generator=torch.Generator('cuda').manual_seed(11), keep_unnormalized=True)
  g = torch.Generator('cuda').manual_seed(11)
  packed = fp._pack_images(dev_images)
  op_d, arg_d = fp.rand_augment_plan(packed[2], packed[3], generator=g)
  flip = (torch.rand(len(big), generator=g, device='cuda') > 0.5).cpu()
  print('drawn ops', op_d.tolist(), 'flip', flip.tolist())
  for b, (im, i) in enumerate(zip(big, op_d.tolist())):               # the device plan holds the float64 formulas' values
    sign = -1 if i in ac.AFFINE and float(arg_d[b, {2: 3, 9: 1, 10: 3, 11: 2, 12: 5}[i]]) < 0 else 1
    assert np.array_equal(arg_d[b].cpu().numpy(), ac.default_args(i, im.shape[0], im.shape[1], sign)), (b, i)
  on_dev = fp.rand_augment(packed, op_d, arg_d)
  on_host = fp.rand_augment(tuple(t.cpu() for t in packed), op_d.cpu(), arg_d.cpu())
  assert torch.equal(on_dev[0].cpu(), on_host[0])                     # the augmentation: bit-equal to the CPU path ...
  augmented = [ac.augment(im, i, a) for im, i, a in zip(big, op_d.tolist(), arg_d.cpu().numpy())]
  for b, im in enumerate(augmented):                                  # ... and to the oracle
    o = int(packed[1][b])
    assert np.array_equal(on_host[0][o:o + im.size].numpy(), im.reshape(-1)), (b, int(op_d[b]))
  check_outputs(out, augmented, 32, 16, flip.tolist(), 3)
  host = fp.images_to_patch_features(on_host, 32, 16, flip=flip, keep_unnormalized=True, output_channel_bits=3)
  check_outputs(host, augmented, 32, 16, flip.tolist(), 3)
  cfg_eval = configs.MmtPretrainDataConfig(is_training=False, use_rand_aug=True, image_size=32, patch_size=16)
  ev = fp.decode_image_features(cfg_eval, dev_images)
  plain = fp.images_to_patch_features(dev_images, 32, 16, output_channel_bits=3)
  assert all(torch.equal(ev[k], plain[k]) for k in ('patch_embeddings', 'mpp_label_ids'))
