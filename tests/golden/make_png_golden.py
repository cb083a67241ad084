"""Writes tests/golden/png: the crossed fixtures of tests/_png_cases.plan() from its own PNG writer, three files written
by Pillow itself, one file with ancillary chunks and one palette file with fewer entries than indices used; then
fixtures.txt and expected_pixels.rgb, Pillow's decode (`Image.open(f).convert('RGB')`) of every file, back to back in the
order of fixtures.txt.  Needs Pillow; the tests do not.  Run from the repository root:

  python tests/golden/make_png_golden.py
"""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _png_cases as P  # noqa: E402


def pillow_files():
  rgb, _ = P.content('rgb8', 24, 19, seed=501)
  out = {}
  buf = io.BytesIO()
  Image.fromarray(rgb, 'RGB').save(buf, 'PNG', optimize=True)
  out['pillow_optimize'] = buf.getvalue()
  buf = io.BytesIO()
  Image.fromarray(rgb, 'RGB').quantize(colors=23).save(buf, 'PNG')
  out['pillow_palette'] = buf.getvalue()
  buf = io.BytesIO()
  Image.fromarray(rgb, 'RGB').convert('1').save(buf, 'PNG')     # Pillow writes no interlaced files: a 1-bit grey one instead
  out['pillow_bilevel'] = buf.getvalue()
  return out


def ancillary_file():
  h, w = 9, 17
  rgb, _ = P.content('rgb8', h, w, seed=502)
  before = (P.chunk(b'gAMA', struct.pack('>I', 45455)) + P.chunk(b'tEXt', b'Comment\x00skipped') +
            P.chunk(b'acTL', struct.pack('>II', 1, 0)) + P.chunk(b'fcTL', struct.pack('>IIIIIHHBB', 0, w, h, 0, 0, 1, 10, 0, 0)))
  after = P.chunk(b'tEXt', b'Comment\x00behind the data', crc=12345)         # an ancillary CRC error: ignored, as libpng does
  return P.encode('rgb8', rgb, filters='cycle', lace=1, before_idat=before, after_idat=after, split=50)


def short_palette_file():
  smp, pal = P.content('p4', 9, 17, seed=503, palette_entries=5)              # indices 0..15, five entries
  return P.encode('p4', smp, palette=pal, filters=4, lace=0, block='fixed')


def main():
  os.makedirs(P.GOLDEN, exist_ok=True)
  files = {name: P.build(name) for name, *_ in P.plan()}
  files.update(pillow_files())
  files['ancillary_chunks'] = ancillary_file()
  files['short_palette'] = short_palette_file()
  assert list(files)[-5:] == list(P.EXTRA)
  pixels = []
  for name, raw in files.items():
    assert len(raw) <= 16 * 1024, name
    with open(os.path.join(P.GOLDEN, name + '.png'), 'wb') as f:
      f.write(raw)
    pixels.append(np.asarray(Image.open(io.BytesIO(raw)).convert('RGB')).reshape(-1))
  with open(os.path.join(P.GOLDEN, 'fixtures.txt'), 'w') as f:
    f.write('\n'.join(files) + '\n')
  np.concatenate(pixels).astype(np.uint8).tofile(os.path.join(P.GOLDEN, 'expected_pixels.rgb'))
  print(len(files), 'files,', sum(len(v) for v in files.values()), 'bytes of PNG,', sum(p.size for p in pixels), 'bytes of pixels')


if __name__ == '__main__':
  main()
