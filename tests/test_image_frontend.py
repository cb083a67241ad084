"""Image front end (mmt_amd/feature_pipeline.images_to_patch_features, C entry point mmt_image_patches) without a GPU.

The yardstick is `restatement` (tests/_cases.py): float64 numpy, written from the reference's text (`decode_fn`,
src/data/data_utils.py:195-222; MPP label ids :448-481) and independent of the torch and HIP code.  It keeps the
reference's own order -- normalise, THEN resize (:204-205) -- while the product resizes once and normalises afterwards.
The float half is unpinned: tensorflow is not installed where these tests were written, so tf.image.resize itself
was never run against them."""
import ctypes

import numpy as np
import pytest
import torch

from tests._cases import CONFIGS, EDGE_EPS, batch, check_outputs, patches, restatement


def test_the_fixed_seed_keeps_the_restatement_within_the_edge_cap():
  for image_size, patch_size in CONFIGS:
    for flip in (None, [1, 0, 1, 0, 1]):
      dist = restatement(batch(image_size), image_size, patch_size, flip, 3)[3]
      assert (dist <= EDGE_EPS).mean() <= 0.02
  assert (restatement(batch(24), 24, 8, None, 1)[3] <= EDGE_EPS).mean() <= 0.02
  assert (restatement(batch(24)[1:], 24, 8, None, 8)[3] <= EDGE_EPS).mean() <= 0.02      # tests/test_gpu_image_frontend.py


def test_hand_checked_resize():
  """1x2 image [a, b] to width 4: src = -0.25, 0.25, 0.75, 1.25 -> [a, 0.75a + 0.25b, 0.25a + 0.75b, b]."""
  from mmt_amd import feature_pipeline as fp
  a, b = np.array([10, 200, 30]), np.array([250, 0, 90])
  im = np.stack([a, b])[None].astype(np.uint8)
  out = fp.images_to_patch_features([torch.from_numpy(im)], 4, 4, keep_unnormalized=True)
  got = out['unnormalized_patch_embeddings'].numpy().reshape(4, 4, 3)
  want = np.stack([a, 0.75 * a + 0.25 * b, 0.25 * a + 0.75 * b, b]) / 255.0
  assert np.abs(got - want[None]).max() <= 1e-6
  assert np.abs(restatement([im], 4, 4)[1].reshape(4, 4, 3) - want[None]).max() <= 1e-12      # and the yardstick


def test_identity():
  from mmt_amd import feature_pipeline as fp
  u8 = np.random.default_rng(1).integers(0, 256, size=(24, 24, 3), dtype=np.uint8)
  out = fp.images_to_patch_features([torch.from_numpy(u8)], 24, 8, keep_unnormalized=True)
  want = patches(u8.astype(np.float32) / np.float32(255), 8)
  assert np.array_equal(out['unnormalized_patch_embeddings'].numpy()[0], want)


@pytest.mark.parametrize('size', [(1, 1), (3, 50), (40, 40), (64, 17)])
def test_constant_colour(size):
  from mmt_amd import feature_pipeline as fp
  im = torch.tensor([10, 100, 200], dtype=torch.uint8).expand(*size, 3).contiguous()
  out = fp.images_to_patch_features([im], 24, 8, output_channel_bits=3)
  assert out['mpp_label_ids'].dtype == torch.int32 and out['mpp_label_ids'].shape == (1, 9)
  assert (out['mpp_label_ids'] == 0 + 3 * 8 + 6 * 64).all()


@pytest.mark.parametrize('image_size,patch_size', CONFIGS)
@pytest.mark.parametrize('flip', [None, [1, 0, 1, 0, 1]], ids=['noflip', 'flip'])
def test_torch_path_matches_the_restatement(image_size, patch_size, flip):
  from mmt_amd import feature_pipeline as fp
  images = batch(image_size)
  tf = None if flip is None else torch.tensor(flip, dtype=torch.bool)
  out = fp.images_to_patch_features([torch.from_numpy(x) for x in images], image_size, patch_size, flip=tf,
                                    keep_unnormalized=True, output_channel_bits=3)
  check_outputs(out, images, image_size, patch_size, flip, 3)
  out16 = fp.images_to_patch_features([torch.from_numpy(x) for x in images], image_size, patch_size, flip=tf,
                                      out_dtype=torch.bfloat16)
  assert set(out16) == {'patch_embeddings', 'num_image_wordpieces'} and out16['patch_embeddings'].dtype == torch.bfloat16
  check_outputs(out16, images, image_size, patch_size, flip, 0, bf16=True)


def test_packed_input_equals_the_list_and_feeds_the_existing_functions():
  from mmt_amd import feature_pipeline as fp
  images = [torch.from_numpy(x) for x in batch(24)]
  pixels = torch.cat([x.reshape(-1) for x in images])
  sizes = torch.tensor([x.shape[:2] for x in images], dtype=torch.int32)
  offsets = torch.cumsum(torch.tensor([0] + [x.numel() for x in images[:-1]]), 0)
  a = fp.images_to_patch_features(images, 24, 8, keep_unnormalized=True, output_channel_bits=3)
  b = fp.images_to_patch_features((pixels, offsets, sizes[:, 0].contiguous(), sizes[:, 1].contiguous()), 24, 8,
                                  keep_unnormalized=True, output_channel_bits=3)
  for k in ('patch_embeddings', 'unnormalized_patch_embeddings', 'mpp_label_ids'):
    assert torch.equal(a[k], b[k]), k
  # the new outputs are what make_mpp_label_ids expects
  assert torch.equal(fp.make_mpp_label_ids(a['unnormalized_patch_embeddings'], 8), a['mpp_label_ids'])


def test_python_argument_errors():
  from mmt_amd import feature_pipeline as fp
  im = torch.zeros(4, 4, 3, dtype=torch.uint8)
  bad = [
      (dict(images=[im.float()]), 'uint8'),
      (dict(images=[im[..., :2]]), r'\[height, width, 3\]'),
      (dict(images=[im[:0]]), 'empty'),
      (dict(images=[]), 'empty'),
      (dict(image_size=0), 'positive'),
      (dict(patch_size=0), 'positive'),
      (dict(patch_size=9), 'exceeds'),
      (dict(out_dtype=torch.float16), 'out_dtype'),
      (dict(output_channel_bits=9), 'output_channel_bits'),
      (dict(flip=torch.zeros(2, dtype=torch.bool)), 'flip'),
      (dict(flip=torch.zeros(1)), 'flip'),
      (dict(images=(im.reshape(-1), torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32),
                    torch.ones(1, dtype=torch.int32))), 'offsets'),
      (dict(images=(im.reshape(-1), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32),
                    torch.ones(1, dtype=torch.int32))), 'positive'),
      (dict(images=(im.reshape(-1), torch.zeros(1, dtype=torch.int64), torch.full((1,), 5, dtype=torch.int32),
                    torch.full((1,), 4, dtype=torch.int32))), 'leaves the pixel buffer'),
  ]
  for kw, match in bad:
    args = dict(images=[im], image_size=8, patch_size=4)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
      fp.images_to_patch_features(**args)


def test_c_entry_point_argument_errors_without_gpu():
  """The host-side refusals of mmt_image_patches: they return before anything is launched, so the fake non-NULL
  pointers are never used (as in test_c_abi.test_argument_errors_without_gpu)."""
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  L = _lib.lib()

  def desc(**kw):
    d = _lib.ImageDesc()
    d.B, d.image_size, d.patch_size, d.out_dtype, d.channel_bits = 2, 32, 16, _lib.MMT_F32, 3
    d.mean[:] = [0.485, 0.456, 0.406]
    for k, v in kw.items():
      if k == 'mean':
        d.mean[:] = v
      else:
        setattr(d, k, v)
    return d

  def call(d, pixels=1, nbytes=64, offsets=1, heights=1, widths=1, out=1):
    return L.mmt_image_patches(d, pixels, nbytes, offsets, heights, widths, None, out, None, None, None)

  assert ctypes.sizeof(_lib.ImageDesc) == 32
  assert call(None) == -1 and b'desc is NULL' in L.mmt_last_error()
  for kw in (dict(pixels=None), dict(offsets=None), dict(heights=None), dict(widths=None), dict(out=None)):
    assert call(desc(), **kw) == -1 and b'NULL argument' in L.mmt_last_error(), kw
  assert call(desc(), nbytes=0) == -1 and b'pixels_bytes' in L.mmt_last_error()
  for kw in (dict(B=0), dict(B=-3), dict(image_size=0), dict(patch_size=0), dict(patch_size=-1)):
    assert call(desc(**kw)) == -1 and b'must be positive' in L.mmt_last_error(), kw
  assert call(desc(patch_size=33)) == -1 and b'exceeds image_size' in L.mmt_last_error()
  assert call(desc(out_dtype=2)) == -1 and b'out_dtype' in L.mmt_last_error()
  for bits in (-1, 9):
    assert call(desc(channel_bits=bits)) == -1 and b'channel_bits' in L.mmt_last_error()
  assert call(desc(mean=[0.485, 0.0, 0.406])) == -1 and b'mean[1]' in L.mmt_last_error()
  # P * P * B beyond the grid arithmetic: 2^15 * 2^15 patches per image, 2 images
  assert call(desc(image_size=1 << 15, patch_size=1)) == -1 and b'grid arithmetic' in L.mmt_last_error()
  assert call(desc(B=1 << 20, image_size=64, patch_size=1)) == -1 and b'grid arithmetic' in L.mmt_last_error()
  assert call(desc(B=1, image_size=1 << 30, patch_size=1 << 15)) == -1 and b'values per patch' in L.mmt_last_error()
