"""RandAugment: the numpy oracle, the image set and the packing helper of tests/test_rand_augment.py (CPU) and
tests/test_gpu_rand_augment.py (GPU).  The definitions are DESIGN.md section 4 restated in numpy: integer arithmetic in
int64, float arithmetic in np.float32 with every product and sum its own numpy operation (numpy never fuses them), so
parity with the kernels and with the torch path of mmt_amd.feature_pipeline is bit-exact -- no tolerance anywhere.
Pillow pins the integer operations independently (test_rand_augment.py)."""
import functools
import math

import numpy as np

OPS = ('AutoContrast', 'Equalize', 'Rotate', 'Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness', 'Sharpness',
       'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'SolarizeAdd')
ALL_IDS = list(range(-1, 14))          # -1: identity
AFFINE = (2, 9, 10, 11, 12)
SEED = 20212
STATS_CHUNK = 4096                     # pixels per workgroup step of the statistics pass (csrc/rand_augment.h: kRandAugChunk)
F32 = np.float32


@functools.lru_cache(maxsize=None)
def image_set():
  """The issue's images, in its order.  The last one has 96 * 100 = 9600 pixels, more than two chunks of STATS_CHUNK:
  three workgroups of the statistics pass each hold a part of its histograms and the merge across them happens."""
  rng = np.random.default_rng(SEED)
  rand = lambda h, w, lo=0, hi=256: rng.integers(lo, hi, size=(h, w, 3), dtype=np.uint8)
  images = [rand(1, 1), rand(2, 3), rand(3, 3), rand(5, 7), rand(17, 16), rand(37, 23), rand(64, 48),
            np.full((8, 8, 3), 77, dtype=np.uint8), rand(40, 40, 90, 154), rand(96, 100)]
  assert images[-1].shape[0] * images[-1].shape[1] > 2 * STATS_CHUNK
  for im in images:
    im.setflags(write=False)
  return tuple(images)


def grey(im):
  im = im.astype(np.int64)
  return (19595 * im[..., 0] + 38470 * im[..., 1] + 7471 * im[..., 2] + 32768) >> 16


def blend(a, b, f):
  """trunc(clip(a + f * (b - a), 0, 255)): a, b integer arrays, f one float32."""
  d = (b.astype(np.int64) - a.astype(np.int64)).astype(F32)
  prod = F32(f) * d
  t = a.astype(F32) + prod
  return np.minimum(np.maximum(t, F32(0)), F32(255)).astype(np.int64)


def equalize_lut(channel):
  hist = [int((channel == v).sum()) for v in range(256)]
  last = [c for c in hist if c][-1]
  step = (sum(hist) - last) // 255
  if step == 0:
    return None
  lut, below = [0] * 256, 0
  for v in range(256):
    lut[v] = min(255, (below + step // 2) // step)
    below += hist[v]
  lut[0] = 0
  return np.array(lut, dtype=np.int64)


def affine(im, a, b):
  h, w = im.shape[:2]
  a, b = [F32(v) for v in a], [F32(v) for v in b]
  x = np.arange(w, dtype=F32)[None, :].repeat(h, 0)
  y = np.arange(h, dtype=F32)[:, None].repeat(w, 1)
  with np.errstate(all='ignore'):
    sx = (a[0] * x + a[1] * y) + a[2]
    sy = (b[0] * x + b[1] * y) + b[2]
    rx, ry = np.floor(sx + F32(0.5)), np.floor(sy + F32(0.5))
  ok = (np.abs(rx) < F32(2.0 ** 30)) & (np.abs(ry) < F32(2.0 ** 30))          # false for NaN and infinity as well
  ix, iy = np.where(ok, rx, -1).astype(np.int64), np.where(ok, ry, -1).astype(np.int64)
  ok &= (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
  out = np.full_like(im, 128)
  out[ok] = im[iy[ok], ix[ok]]
  return out


def augment(im, op, arg):
  """One operation on a uint8 [h, w, 3] array; arg: 8 float32 values."""
  arg = np.asarray(arg, dtype=F32)
  h, w = im.shape[:2]
  v = im.astype(np.int64)
  if op == 0:
    out = v.copy()
    for c in range(3):
      lo, hi = int(v[..., c].min()), int(v[..., c].max())
      if hi > lo:
        scale = F32(255.0) / F32(hi - lo)
        off = F32(-lo) * scale
        prod = v[..., c].astype(F32) * scale
        out[..., c] = np.minimum(np.maximum(prod + off, F32(0)), F32(255)).astype(np.int64)
  elif op == 1:
    out = v.copy()
    for c in range(3):
      lut = equalize_lut(v[..., c])
      if lut is not None:
        out[..., c] = lut[v[..., c]]
  elif op == 3:
    bits = int(arg[0])
    out = (v >> (8 - bits)) << (8 - bits)
  elif op == 4:
    out = np.where(v < int(arg[0]), v, 255 - v)
  elif op == 13:
    out = np.where(v < 128, np.minimum(255, v + int(arg[0])), v)
  elif op == 5:
    out = blend(grey(im)[..., None].repeat(3, -1), v, arg[0])
  elif op == 6:
    g = grey(im)
    m = (int(g.sum()) + g.size // 2) // g.size
    out = blend(np.full_like(v, m), v, arg[0])
  elif op == 7:
    out = blend(np.zeros_like(v), v, arg[0])
  elif op == 8:
    out = v.copy()
    if h >= 3 and w >= 3:
      centre = v[1:-1, 1:-1]
      around = sum(v[dy:dy + h - 2, dx:dx + w - 2] for dy in range(3) for dx in range(3)) - centre      # the 8 neighbours
      out[1:-1, 1:-1] = blend((around + 5 * centre) // 13, centre, arg[0])
  elif op in AFFINE:
    out = affine(im, arg[0:3], arg[3:6])
  else:
    out = v
  return out.astype(np.uint8)


def default_args(op, h, w, sign=1, magnitude=10.0, translate_const=100.0):
  """arg[8] of an operation from the magnitude: float64 formulas, rounded once to float32."""
  L = magnitude / 10.0
  arg = np.zeros(8, dtype=np.float64)
  if op in (5, 6, 7, 8):
    arg[0] = 1.8 * L + 0.1
  elif op == 3:
    arg[0] = int(4 * L)
  elif op == 4:
    arg[0] = int(256 * L)
  elif op == 13:
    arg[0] = int(110 * L)
  elif op == 2:
    t = sign * math.radians(30.0 * L)
    c, s = math.cos(t), math.sin(t)
    arg[:6] = [c, -s, ((w - 1) - (c * (w - 1) - s * (h - 1))) / 2, s, c, ((h - 1) - (s * (w - 1) + c * (h - 1))) / 2]
  elif op == 9:
    arg[:6] = [1, sign * 0.3 * L, 0, 0, 1, 0]
  elif op == 10:
    arg[:6] = [1, 0, 0, sign * 0.3 * L, 1, 0]
  elif op == 11:
    arg[:6] = [1, 0, sign * translate_const * L, 0, 1, 0]
  elif op == 12:
    arg[:6] = [1, 0, 0, 0, 1, sign * translate_const * L]
  return arg.astype(F32)


# Arguments the parity tests use besides the magnitude-10 defaults: blends that clip on both sides and truncate, a
# Solarize that does something (at magnitude 10 it is the identity), translations that stay inside the small images.
TEST_ARGS = {3: (4, 0, 8, 1), 4: (256, 128, 0), 13: (110, 0, 255), 5: (1.9, 0.0, 0.37), 6: (1.9, 0.37), 7: (1.9, 0.37),
             8: (1.9, 0.37, -0.6)}


def case_args(op, h, w, variant):
  """arg[8] of parity case `variant` (0, 1, ...) of an operation on an h x w image."""
  if op in TEST_ARGS:
    arg = np.zeros(8, dtype=F32)
    arg[0] = TEST_ARGS[op][variant % len(TEST_ARGS[op])]
    return arg
  if op in AFFINE:
    return default_args(op, h, w, sign=1 if variant % 2 == 0 else -1, magnitude=10.0 if variant < 2 else 0.3)
  return np.zeros(8, dtype=F32)


@functools.lru_cache(maxsize=None)
def expected(index, op, variant):
  """The oracle's result for image `index` of the set, computed once and shared by the tests (read-only)."""
  im = image_set()[index]
  out = augment(im, op, case_args(op, im.shape[0], im.shape[1], variant))
  out.setflags(write=False)
  return out


SENTINEL = 0xA5
GUARD = 256


def pack(images, gaps=(5, 16, 0, 7, 3, 1, 32, 2, 11, 13, 6, 9, 4, 8, 10, 17)):
  """Packed layout with gaps: (pixels uint8 [n + GUARD] filled with SENTINEL outside the images, offsets int64,
  heights, widths int32, n = the pixels_bytes to pass).  The gaps make most offsets odd, so the byte stream of the
  apply pass has a scalar head and tail around its 16-byte body."""
  offs, at = [], gaps[0]
  for i, im in enumerate(images):
    offs.append(at)
    at += im.size + gaps[(i + 1) % len(gaps)]
  pixels = np.full(at + GUARD, SENTINEL, dtype=np.uint8)
  for o, im in zip(offs, images):
    pixels[o:o + im.size] = im.reshape(-1)
  return (pixels, np.array(offs, dtype=np.int64), np.array([im.shape[0] for im in images], dtype=np.int32),
          np.array([im.shape[1] for im in images], dtype=np.int32), at)


def check_packed(got, images_expected, offsets, n):
  """`got` (uint8 [n + GUARD], pre-filled with SENTINEL) holds exactly the expected images; gaps and guard untouched."""
  want = np.full(got.shape, SENTINEL, dtype=np.uint8)
  for o, im in zip(offsets, images_expected):
    want[o:o + im.size] = im.reshape(-1)
  bad = np.nonzero(got != want)[0]
  assert bad.size == 0, f'{bad.size} bytes differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]} (offsets {list(offsets)})'
