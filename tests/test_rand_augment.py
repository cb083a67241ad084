"""RandAugment without a GPU: the oracle of tests/_augment_cases.py against hand-written vectors and Pillow, the torch
path of mmt_amd.feature_pipeline.rand_augment against the oracle (bit-exact, every id on every image of the set), the
plan, decode_image_features in the three states of the config, and the refusals of mmt_rand_augment through the C ABI."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import _augment_cases as ac
from tests._cases import batch


def arg8(*values):
  arg = np.zeros(8, dtype=np.float32)
  arg[:len(values)] = values
  return arg


def rgb(values):
  """A [1, n, 3] image with the same value on the three channels."""
  return np.repeat(np.array(values, dtype=np.uint8)[None, :, None], 3, axis=2)


# ---- hand-written vectors ----------------------------------------------------------------------------------------------
def test_posterize_solarize_solarize_add_by_hand():
  assert ac.augment(rgb([0, 15, 16, 255]), 3, arg8(4))[0, :, 0].tolist() == [0, 0, 16, 240]
  assert ac.augment(rgb([0, 15, 16, 255]), 3, arg8(0))[0, :, 1].tolist() == [0, 0, 0, 0]
  assert ac.augment(rgb([0, 15, 16, 255]), 3, arg8(8))[0, :, 2].tolist() == [0, 15, 16, 255]
  assert ac.augment(rgb([100, 127, 128, 200]), 13, arg8(110))[0, :, 0].tolist() == [210, 237, 128, 200]
  assert ac.augment(rgb([100, 127, 128, 200]), 13, arg8(200))[0, :, 0].tolist() == [255, 255, 128, 200]
  every = rgb(list(range(256)))
  assert np.array_equal(ac.augment(every, 4, arg8(256)), every)                     # magnitude 10: the identity, literally
  assert ac.augment(rgb([0, 127, 128, 255]), 4, arg8(128))[0, :, 0].tolist() == [0, 127, 127, 0]
  assert np.array_equal(ac.augment(every, -1, arg8()), every) and np.array_equal(ac.augment(every, 99, arg8()), every)


def test_blend_truncates_and_clips_on_both_sides():
  # Brightness = blend(0, v, f): 1.9 * 100 = 190.000..., 1.9 * 7 = 13.29... -> 13 (truncation), 1.9 * 200 clips at 255
  assert ac.augment(rgb([7, 100, 200, 255]), 7, arg8(1.9))[0, :, 0].tolist() == [13, 190, 255, 255]
  assert ac.augment(rgb([7, 100]), 7, arg8(0.5))[0, :, 0].tolist() == [3, 50]       # 3.5 -> 3
  # Contrast around the mean: one pixel of each of 0 and 200 -> grey mean 100; 100 + 1.9 * (0 - 100) = -90 -> 0, the
  # other 100 + 1.9 * 100 = 290 -> 255; with f = 0.37: 100 - 37 = 63, 100 + 37 = 137
  assert ac.augment(rgb([0, 200]), 6, arg8(1.9))[0, :, 0].tolist() == [0, 255]
  assert ac.augment(rgb([0, 200]), 6, arg8(0.37))[0, :, 0].tolist() == [63, 137]
  # Color: grey of (255, 0, 0) is (19595 * 255 + 32768) >> 16 = 76; factor 0 gives the grey, factor 1 the pixel
  red = np.array([[[255, 0, 0]]], dtype=np.uint8)
  assert ac.augment(red, 5, arg8(0.0))[0, 0].tolist() == [76, 76, 76]
  assert ac.augment(red, 5, arg8(1.0))[0, 0].tolist() == [255, 0, 0]
  assert ac.augment(red, 5, arg8(1.9))[0, 0].tolist() == [255, 0, 0]               # 76 + 1.9 * 179 clips, 76 - 1.9 * 76 clips


def test_autocontrast_and_equalize_by_hand():
  im = rgb([50, 100, 150])
  assert ac.augment(im, 0, arg8())[0, :, 0].tolist() == [0, 127, 255]               # scale 2.55: 50 * 2.55 - 127.5 = 0, 127.5 -> 127
  flat = np.full((4, 4, 3), 9, dtype=np.uint8)
  assert np.array_equal(ac.augment(flat, 0, arg8()), flat) and np.array_equal(ac.augment(flat, 1, arg8()), flat)
  # Equalize: 510 pixels of 10 and 510 of 20 and one of 30: last = 1, step = 1020 // 255 = 4;
  # lut[10] = (0 + 2) // 4 = 0, lut[20] = (510 + 2) // 4 = 128, lut[30] = (1020 + 2) // 4 = 255
  values = np.array([10] * 510 + [20] * 510 + [30], dtype=np.uint8)
  out = ac.augment(np.repeat(values[None, :, None], 3, axis=2), 1, arg8())
  assert sorted(set(out[0, :, 1].tolist())) == [0, 128, 255]
  assert out[0, 0, 0] == 0 and out[0, 510, 0] == 128 and out[0, 1020, 0] == 255


def test_sharpness_of_a_3x3_by_hand():
  im = np.zeros((3, 3, 3), dtype=np.uint8)
  im[..., 0] = [[10, 20, 30], [40, 100, 60], [70, 80, 90]]                          # neighbours 400 + 5 * 100 = 900 -> 69
  im[..., 1] = 200                                                                  # flat: 13 * 200 / 13 = 200
  im[..., 2] = [[0, 0, 0], [0, 13, 0], [0, 0, 0]]                                   # 65 // 13 = 5
  out = ac.augment(im, 8, arg8(1.9))
  want = im.copy()
  want[1, 1] = [int(np.float32(69) + np.float32(1.9) * np.float32(31)), 200, int(np.float32(5) + np.float32(1.9) * np.float32(8))]
  assert want[1, 1].tolist() == [127, 200, 20]
  assert np.array_equal(out, want)                                                  # the border is unchanged
  small = ac.image_set()[1]
  assert np.array_equal(ac.augment(small, 8, arg8(1.9)), small)                     # 2x3: no interior


def test_translate_and_quarter_turn_by_hand():
  im = np.arange(27, dtype=np.uint8).reshape(3, 3, 3)
  out = ac.augment(im, 11, arg8(1, 0, 1, 0, 1, 0))                                  # sx = x + 1: column x takes column x + 1
  assert np.array_equal(out[:, :2], im[:, 1:]) and (out[:, 2] == 128).all()
  out = ac.augment(im, 12, arg8(1, 0, 0, 0, 1, -1))                                 # sy = y - 1: row 0 is outside
  assert np.array_equal(out[1:], im[:2]) and (out[0] == 128).all()
  out = ac.augment(im, 2, arg8(0, -1, 2, 1, 0, 0))                                  # sx = 2 - y, sy = x: an exact quarter turn
  for y in range(3):
    for x in range(3):
      assert np.array_equal(out[y, x], im[x, 2 - y])
  huge = ac.augment(im, 11, arg8(1, 0, 3e38, 0, 1, 0))                              # beyond 2^30 and infinite sums: all outside
  assert (huge == 128).all()
  assert (ac.augment(im, 11, arg8(1, 0, float('nan'), 0, 1, 0)) == 128).all()


# ---- Pillow pins ---------------------------------------------------------------------------------------------------------
def test_integer_operations_equal_pillow():
  Image = pytest.importorskip('PIL.Image')
  ImageOps = pytest.importorskip('PIL.ImageOps')
  for im in ac.image_set():
    pil = Image.fromarray(np.ascontiguousarray(im))                                 # uint8 [h, w, 3]: mode RGB
    assert np.array_equal(ac.augment(im, 1, arg8()), np.asarray(ImageOps.equalize(pil))), im.shape
    for bits in (1, 4, 8):
      assert np.array_equal(ac.augment(im, 3, arg8(bits)), np.asarray(ImageOps.posterize(pil, bits))), (im.shape, bits)
    for thr in (0, 128, 256):
      assert np.array_equal(ac.augment(im, 4, arg8(thr)), np.asarray(ImageOps.solarize(pil, thr))), (im.shape, thr)
    assert np.array_equal(ac.augment(im, 5, arg8(0.0))[..., 0], np.asarray(pil.convert('L'))), im.shape
    diff = np.abs(ac.augment(im, 0, arg8()).astype(int) - np.asarray(ImageOps.autocontrast(pil)).astype(int))
    assert diff.max() <= 1, (im.shape, diff.max())                                  # Pillow computes in double, we in fp32


# ---- the torch path of the package ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('op', ac.ALL_IDS)
def test_cpu_path_equals_the_oracle(op):
  from mmt_amd import feature_pipeline as fp
  images = ac.image_set()
  for variant in range(3 if op in ac.TEST_ARGS or op in ac.AFFINE else 1):
    arg = np.stack([ac.case_args(op, im.shape[0], im.shape[1], variant) for im in images])
    out, offsets, heights, widths = fp.rand_augment([torch.from_numpy(im.copy()) for im in images],
                                                    torch.full((len(images),), op, dtype=torch.int32), torch.from_numpy(arg))
    for b, im in enumerate(images):
      got = out[int(offsets[b]):int(offsets[b]) + im.size].reshape(im.shape).numpy()
      assert np.array_equal(got, ac.expected(b, op, variant)), (op, variant, im.shape)
    assert heights.tolist() == [im.shape[0] for im in images] and widths.tolist() == [im.shape[1] for im in images]


def test_cpu_path_mixed_ids_packed_input_and_out():
  from mmt_amd import feature_pipeline as fp
  images = ac.image_set()
  ids = [ac.ALL_IDS[(3 * b) % 15] for b in range(len(images))] + [14, -7]
  images = list(images) + [images[5], images[6]]
  arg = np.stack([ac.case_args(i, im.shape[0], im.shape[1], 0) for i, im in zip(ids, images)])
  pixels, offsets, heights, widths, n = ac.pack(images)
  packed = tuple(torch.from_numpy(x) for x in (pixels[:n].copy(), offsets, heights, widths))
  out = torch.full((n,), ac.SENTINEL, dtype=torch.uint8)
  res = fp.rand_augment(packed, torch.tensor(ids, dtype=torch.int32), torch.from_numpy(arg), out=out)
  assert res[0] is out
  want = [ac.augment(im, i, a) for im, i, a in zip(images, ids, arg)]
  ac.check_packed(np.concatenate([out.numpy(), np.full(ac.GUARD, ac.SENTINEL, np.uint8)]), want, offsets, n)
  assert np.array_equal(want[-1], images[-1]) and np.array_equal(want[-2], images[-2])     # ids outside [-1, 13] copy
  with pytest.raises(ValueError, match='overlap'):
    fp.rand_augment(packed, torch.tensor(ids, dtype=torch.int32), torch.from_numpy(arg), out=packed[0])
  with pytest.raises(ValueError, match='int32'):
    fp.rand_augment(packed, torch.tensor(ids), torch.from_numpy(arg))


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_draws_ids_in_range_both_signs_and_repeats_with_the_seed():
  from mmt_amd import feature_pipeline as fp
  assert fp.RAND_AUGMENT_OPS == ac.OPS
  B = 512
  heights = torch.randint(1, 600, (B,), dtype=torch.int32)
  widths = torch.randint(1, 600, (B,), dtype=torch.int32)
  op, arg = fp.rand_augment_plan(heights, widths, generator=torch.Generator().manual_seed(7))
  assert op.dtype == torch.int32 and op.shape == (B,) and arg.dtype == torch.float32 and arg.shape == (B, 8)
  assert int(op.min()) == 0 and int(op.max()) == 13 and len(set(op.tolist())) == 14
  shear = arg[op == 9, 1]
  assert bool((shear > 0).any()) and bool((shear < 0).any())
  again = fp.rand_augment_plan(heights, widths, generator=torch.Generator().manual_seed(7))
  assert torch.equal(op, again[0]) and torch.equal(arg, again[1])
  other = fp.rand_augment_plan(heights, widths, generator=torch.Generator().manual_seed(8))
  assert not torch.equal(op, other[0])


@pytest.mark.parametrize('magnitude,translate_const', [(10.0, 100.0), (4.0, 30.0)])
def test_plan_coefficients_match_the_float64_formulas(magnitude, translate_const):
  from mmt_amd import feature_pipeline as fp
  ids = [i for i in range(-1, 14) for _ in (0, 1)]
  signs = [1.0, -1.0] * 15
  rng = np.random.default_rng(3)
  hs, ws = rng.integers(1, 700, len(ids)), rng.integers(1, 700, len(ids))
  op, arg = fp.rand_augment_plan(torch.tensor(hs, dtype=torch.int32), torch.tensor(ws, dtype=torch.int32), magnitude=magnitude,
                                 translate_const=translate_const, ops=torch.tensor(ids), signs=torch.tensor(signs))
  assert op.tolist() == ids
  for b, (i, sg) in enumerate(zip(ids, signs)):
    want = ac.default_args(i, int(hs[b]), int(ws[b]), sg, magnitude, translate_const)
    assert np.array_equal(arg[b].numpy(), want), (i, sg, arg[b], want)
  if magnitude == 10.0:
    assert float(arg[ids.index(4), 0]) == 256.0 and float(arg[ids.index(3), 0]) == 4.0 and float(arg[ids.index(13), 0]) == 110.0
    assert float(arg[ids.index(7), 0]) == np.float32(1.9)
    k = ids.index(2)
    assert abs(float(arg[k, 0]) - math.cos(math.radians(30))) < 1e-7 and abs(float(arg[k, 3]) - 0.5) < 1e-7


# ---- decode_image_features ---------------------------------------------------------------------------------------------------
def test_decode_image_features_in_the_three_config_states():
  from mmt_amd import configs
  from mmt_amd import feature_pipeline as fp
  images = [torch.from_numpy(x) for x in batch(32)]
  B = len(images)
  same = lambda a, b: set(a) == set(b) and all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a)
  # evaluation: images_to_patch_features bit for bit, with the pretraining config's ids
  cfg = configs.MmtPretrainDataConfig(is_training=False, use_rand_aug=True, image_size=32, patch_size=16)
  got = fp.decode_image_features(cfg, images, keep_unnormalized=True)
  want = fp.images_to_patch_features(images, 32, 16, keep_unnormalized=True, output_channel_bits=cfg.output_channel_bits)
  assert same(got, want) and 'mpp_label_ids' in got
  plain = configs.MmtDataConfig(is_training=False, image_size=32, patch_size=16)
  assert same(fp.decode_image_features(plain, images), fp.images_to_patch_features(images, 32, 16))
  # training without RandAugment: the flip coin alone, u > 0.5, first draw of the generator
  cfg = configs.MmtDataConfig(is_training=True, use_rand_aug=False, image_size=32, patch_size=16)
  got = fp.decode_image_features(cfg, images, generator=torch.Generator().manual_seed(5))
  flip = torch.rand(B, generator=torch.Generator().manual_seed(5)) > 0.5
  assert bool(flip.any()) and not bool(flip.all())
  assert same(got, fp.images_to_patch_features(images, 32, 16, flip=flip))
  # training with RandAugment: plan, augmentation, then the coin, from one generator
  cfg = configs.MmtPretrainDataConfig(is_training=True, use_rand_aug=True, image_size=32, patch_size=16)
  got = fp.decode_image_features(cfg, images, generator=torch.Generator().manual_seed(5), out_dtype=torch.bfloat16)
  g = torch.Generator().manual_seed(5)
  packed = fp._pack_images(images)
  op, arg = fp.rand_augment_plan(packed[2], packed[3], generator=g)
  augmented = fp.rand_augment(packed, op, arg)
  flip = torch.rand(B, generator=g) > 0.5
  want = fp.images_to_patch_features(augmented, 32, 16, flip=flip, out_dtype=torch.bfloat16, output_channel_bits=3)
  assert same(got, want) and got['patch_embeddings'].dtype == torch.bfloat16
  for b, im in enumerate(images):                                       # and the augmentation is the oracle's
    o = int(packed[1][b])
    assert np.array_equal(augmented[0][o:o + im.numel()].reshape(im.shape).numpy(), ac.augment(im.numpy(), int(op[b]), arg[b].numpy()))
  assert not torch.equal(augmented[0], packed[0])


# ---- refusals through the C ABI ------------------------------------------------------------------------------------------------
def test_refusals_without_gpu():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  L = _lib.lib()
  assert L.mmt_rand_augment_workspace_bytes(0) == 0 and L.mmt_rand_augment_workspace_bytes(-3) == 0
  need = L.mmt_rand_augment_workspace_bytes(3)
  assert need == 3 * 4 * 256 * 4
  buf = (ctypes.c_uint8 * 4096)()
  ws = (ctypes.c_uint8 * need)()
  a = ctypes.addressof(buf)
  w = ctypes.addressof(ws)
  ok = dict(B=3, pixels=a, n=1024, offsets=a, heights=a, widths=a, op=a, arg=a, out=a + 2048, ws=w, ws_bytes=need)

  def call(**kw):
    k = dict(ok, **kw)
    return L.mmt_rand_augment(k['B'], k['pixels'], k['n'], k['offsets'], k['heights'], k['widths'], k['op'], k['arg'], k['out'],
                              k['ws'], k['ws_bytes'], None)

  for name in ('pixels', 'offsets', 'heights', 'widths', 'op', 'arg', 'out'):
    assert call(**{name: None}) == -1, name
    assert b'NULL argument' in L.mmt_last_error(), name
  for B in (0, -1):
    assert call(B=B) == -1 and b'must be positive' in L.mmt_last_error()
  for n in (0, -5, 1 << 60):
    assert call(n=n) == -1 and b'pixels_bytes' in L.mmt_last_error()
  for out in (a, a + 1023, a - 1023, a + 1):
    assert call(out=out) == -1 and b'overlaps' in L.mmt_last_error(), out - a
  assert call(ws=None) == -3 and b'workspace' in L.mmt_last_error()
  assert call(ws_bytes=need - 1) == -3 and b'%d bytes needed' % need in L.mmt_last_error()
  assert call(ws_bytes=0) == -3
