"""Writes tests/golden/jpeg: the JPEG fixtures of tests/test_jpeg_decode.py and tests/test_gpu_jpeg_decode.py.

  <name>.jpg       encoded by Pillow (libjpeg-turbo)
  expected_<mode>.npz   'pixels': Pillow's own decode (`convert('RGB')`: grey gives R = G = B) of the files of that
                   mode, uint8 [h, w, 3] each, flattened and concatenated in the order of fixtures.txt
  fixtures.txt     the decodable files, one name per line (csrc/asan/jpeg_driver.c walks it)
  refuse_*.{jpg,png}  files the decoder must refuse

The committed arrays pin the oracle to libjpeg's default decode (JDCT_ISLOW, fancy upsampling) on machines without
Pillow.  Run from the repository root:  python tests/golden/make_jpeg_golden.py"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'jpeg')
SEED = 20213
SIZES = ((1, 1), (8, 8), (7, 5), (9, 2), (9, 3), (9, 4), (40, 1), (1, 40), (17, 9), (16, 16), (33, 31), (24, 17), (48, 80))   # h x w
MODES = (('444_q90', dict(subsampling=0, quality=90)),
         ('422_q50', dict(subsampling=1, quality=50)),
         ('420_q75', dict(subsampling=2, quality=75)),
         ('420_q100_opt', dict(subsampling=2, quality=100, optimize=True)),
         ('420_q30_rst1', dict(subsampling=2, quality=30, restart_marker_blocks=1)),
         ('422_q95_rst2', dict(subsampling=1, quality=95, restart_marker_blocks=2)),
         ('grey_q80', dict(quality=80)))


def content(rng, number, h, w):
  """Even-numbered sizes: uniform noise.  Odd-numbered ones: a smooth pattern plus noise."""
  if number % 2 == 0:
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
  y, x = np.mgrid[0:h, 0:w].astype(np.float64)
  base = np.stack([128 + 100 * np.sin(x / 5.0 + y / 9.0), 255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1)], axis=-1)
  return np.clip(base + rng.normal(0.0, 12.0, size=(h, w, 3)), 0, 255).astype(np.uint8)


def encode(arr, mode, kw):
  buf = io.BytesIO()
  im = Image.fromarray(arr[..., 1], 'L') if mode.startswith('grey') else Image.fromarray(arr, 'RGB')
  im.save(buf, 'JPEG', **kw)
  return buf.getvalue()


def main():
  os.makedirs(HERE, exist_ok=True)
  rng = np.random.default_rng(SEED)
  names, expected = [], {}

  def keep(name, data):
    with open(os.path.join(HERE, name + '.jpg'), 'wb') as f:
      f.write(data)
    names.append(name)
    expected[name] = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))

  for number, (h, w) in enumerate(SIZES):
    arr = content(rng, number, h, w)
    for mode, kw in MODES:
      keep(f'{h}x{w}_{mode}', encode(arr, mode, kw))
  keep('96x100_420_q75', encode(content(rng, 1, 96, 100), '420_q75', dict(subsampling=2, quality=75)))     # more than one workgroup

  small = content(rng, 1, 16, 16)
  refusals = {'refuse_progressive.jpg': encode(small, '420', dict(subsampling=2, quality=75, progressive=True))}
  buf = io.BytesIO()
  Image.fromarray(np.concatenate([small, small[..., :1]], axis=-1), 'CMYK').save(buf, 'JPEG', quality=75)
  refusals['refuse_cmyk.jpg'] = buf.getvalue()
  base = bytearray(encode(small, '444', dict(subsampling=0, quality=75)))
  at = base.index(b'\xff\xc0')
  base[at + 1] = 0xC9                                           # the SOF marker of arithmetic coding
  refusals['refuse_arithmetic.jpg'] = bytes(base)
  refusals['refuse_signature.png'] = b'\x89PNG\r\n\x1a\n' + bytes(24)
  for name, data in refusals.items():
    with open(os.path.join(HERE, name), 'wb') as f:
      f.write(data)

  for mode in sorted({n.split('_', 1)[1] for n in names}):     # one small file per mode: few zip entries, none large
    flat = np.concatenate([expected[n].reshape(-1) for n in names if n.split('_', 1)[1] == mode])
    np.savez_compressed(os.path.join(HERE, f'expected_{mode}.npz'), pixels=flat)
  with open(os.path.join(HERE, 'fixtures.txt'), 'w') as f:
    f.write('\n'.join(names) + '\n')
  total = sum(os.path.getsize(os.path.join(HERE, n)) for n in os.listdir(HERE))
  print(f'{len(names)} fixtures, {len(refusals)} refusals, {total} bytes')


if __name__ == '__main__':
  main()
