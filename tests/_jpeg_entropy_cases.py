"""JPEG entropy decode on the device: the buffers of the C ABI for a batch of files, the yardstick, and the files no
committed fixture provides, for tests/test_jpeg_entropy.py (CPU) and tests/test_gpu_jpeg_entropy.py (GPU).

The yardstick is the merged host path -- mmt_jpeg_info and mmt_jpeg_coefficients per file, as tests/_jpeg_cases.py's
host_stage lays a batch out (planes back to back, coef pre-filled with 0x5555) -- which tests/test_jpeg_decode.py ties
to the numpy oracle and to the committed Pillow decodes.  It is never the code under test.  Parity is bit for bit."""
import ctypes
import functools
import os
import sys

import numpy as np

from tests import _jpeg_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEF_FILL = 0x5555
E_INVALID, E_UNSUPPORTED = -1, -2


def blob(item):
  """A fixture name or the bytes themselves."""
  return J.data(item) if isinstance(item, str) else bytes(item)


def host_stage(lib, items):
  """J.host_stage for fixture names or bytes: (images, coef int16 with every file the host decodes, qtables uint16
  [B * 192], pixel offsets, pixels_bytes, ok: per file whether mmt_jpeg_coefficients took it)."""
  L = lib.lib()
  gaps = (5, 16, 0, 7, 3, 1, 32, 2, 11, 13, 6, 9, 4, 8, 10, 17)
  B = len(items)
  images = (lib.JpegImage * B)()
  base, at, offs = 0, gaps[0], []
  for b, item in enumerate(items):
    raw = blob(item)
    lib.check(L.mmt_jpeg_info(raw, len(raw), ctypes.byref(images[b])))
    for c in range(3):
      images[b].coef_offset[c] += base
    base += images[b].coef_elems
    images[b].pixel_offset = at
    offs.append(at)
    at += images[b].width * images[b].height * 3 + gaps[(b + 1) % len(gaps)]
  coef = J.aligned(base, np.int16, fill=COEF_FILL)
  qtables = J.aligned(B * 192, np.uint16)
  ok = []
  for b, item in enumerate(items):
    raw = blob(item)
    ok.append(L.mmt_jpeg_coefficients(raw, len(raw), ctypes.byref(images[b]), coef.ctypes.data, base, qtables[b * 192:].ctypes.data) == 0)
  return images, coef, qtables, offs, at, ok


class Plans:
  """mmt_jpeg_scan_plan over a batch, concatenated as mmt_jpeg_entropy takes it.  The files sit back to back behind an odd
  number of bytes, so scans start at every alignment.  rc[b] is the plan call's return code; a refused file keeps a
  zeroed scan.  worst_rounds: the subsequences of the longest segment, the max_rounds at which the decode is exact by
  construction."""

  def __init__(self, lib, items, images, subseq_bytes):
    L = lib.lib()
    self.B, self.subseq_bytes = len(items), subseq_bytes
    raws = [blob(it) for it in items]
    self.scans = (lib.JpegScan * self.B)()
    self.rc, self.messages = [], []
    huffs, qts, segs, subs = [], [], [], []
    at_bytes, n_seg, n_sub = 3, 0, 0
    self.file_offsets = []
    for b, raw in enumerate(raws):
      self.file_offsets.append(at_bytes)
      scan = lib.JpegScan()
      rc = L.mmt_jpeg_scan_plan(raw, len(raw), ctypes.byref(images[b]), subseq_bytes, ctypes.byref(scan), None, None, None, 0, None, 0)
      huff = np.zeros(6 * lib.MMT_JPEG_HUFF_WORDS, dtype=np.uint32)
      qt = np.zeros(192, dtype=np.uint16)
      if rc == 0:
        seg = np.full(scan.n_segments * 4, -7, dtype=np.int32)
        sub = np.full(scan.n_subseq, -7, dtype=np.int32)
        # one entry too few is refused, the exact capacity is taken
        assert L.mmt_jpeg_scan_plan(raw, len(raw), ctypes.byref(images[b]), subseq_bytes, ctypes.byref(scan), huff.ctypes.data,
                                    qt.ctypes.data, seg.ctypes.data, scan.n_segments, sub.ctypes.data, scan.n_subseq - 1) == E_INVALID
        lib.check(L.mmt_jpeg_scan_plan(raw, len(raw), ctypes.byref(images[b]), subseq_bytes, ctypes.byref(scan), huff.ctypes.data,
                                       qt.ctypes.data, seg.ctypes.data, scan.n_segments, sub.ctypes.data, scan.n_subseq))
        scan.byte_offset += at_bytes
        scan.segment_offset, scan.subseq_offset = n_seg, n_sub
        self.scans[b] = scan
        segs.append(seg); subs.append(sub)
        n_seg += scan.n_segments; n_sub += scan.n_subseq
      else:
        self.messages.append(L.mmt_last_error().decode())
      self.rc.append(rc)
      huffs.append(huff); qts.append(qt)
      at_bytes += len(raw)
    self.bytes = J.aligned(at_bytes + 5, np.uint8, fill=0xFF)
    for o, raw in zip(self.file_offsets, raws):
      self.bytes[o:o + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    self.huff = J.aligned(self.B * 6 * lib.MMT_JPEG_HUFF_WORDS, np.uint32)
    self.huff[:] = np.concatenate(huffs)
    self.qtables = J.aligned(self.B * 192, np.uint16)
    self.qtables[:] = np.concatenate(qts)
    self.n_segments, self.n_subseq = max(n_seg, 1), max(n_sub, 1)
    self.segments = J.aligned(self.n_segments * 4, np.int32)
    self.subseqs = J.aligned(self.n_subseq, np.int32)
    if segs:
      self.segments[:n_seg * 4] = np.concatenate(segs)
      self.subseqs[:n_sub] = np.concatenate(subs)
    self.max_subseq = max([s.n_subseq for s in self.scans] + [1])
    self.worst_rounds = max([s.max_segment_subseq for s in self.scans] + [1])

  def workspace_bytes(self, lib, max_rounds):
    need = lib.lib().mmt_jpeg_entropy_workspace_bytes(self.B, self.n_subseq, self.max_subseq, self.subseq_bytes, max_rounds)
    assert need > 0
    return need

  def args(self, images_ptr, bytes_ptr, scans_ptr, huff_ptr, seg_ptr, sub_ptr, max_rounds, coef_ptr, coef_elems, status_ptr, ws_ptr, ws_bytes):
    return (self.B, bytes_ptr, self.bytes.size, images_ptr, scans_ptr, huff_ptr, seg_ptr, self.n_segments, sub_ptr, self.n_subseq,
            self.max_subseq, self.subseq_bytes, max_rounds, coef_ptr, coef_elems, status_ptr, ws_ptr, ws_bytes)


def entropy_host(lib, plans, images, coef_elems, max_rounds, workspace_fill=0xA5):
  """mmt_jpeg_entropy_host on fresh buffers: (coef int16 pre-filled with 0x5555, 64 guard elements behind, status int32)."""
  coef = J.aligned(coef_elems + 64, np.int16, fill=COEF_FILL)
  status = np.full(plans.B, -99, dtype=np.int32)
  need = plans.workspace_bytes(lib, max_rounds)
  ws = J.aligned(need, np.uint8, fill=workspace_fill)
  lib.check(lib.lib().mmt_jpeg_entropy_host(*plans.args(
      ctypes.addressof(images), plans.bytes.ctypes.data, ctypes.addressof(plans.scans), plans.huff.ctypes.data, plans.segments.ctypes.data,
      plans.subseqs.ctypes.data, max_rounds, coef.ctypes.data, coef_elems, status.ctypes.data, ws.ctypes.data, need)))
  return coef, status


def planes_mask(images, coef_elems, which):
  """True over the coefficient planes of the images `which` lists."""
  m = np.zeros(coef_elems, dtype=bool)
  for b in which:
    im = images[b]
    for c in range(im.components):
      m[im.coef_offset[c]:im.coef_offset[c] + im.blocks_w[c] * im.blocks_h[c] * 64] = True
  return m


# ---------------------------------------------------------------------------------------------------
# synthesised files
# ---------------------------------------------------------------------------------------------------
def _timing_tool():
  tools = os.path.join(ROOT, 'tools')
  if tools not in sys.path:
    sys.path.insert(0, tools)
  import jpeg_decode_timing
  return jpeg_decode_timing


@functools.lru_cache(maxsize=None)
def dense_stuffing():
  """Noise at quality 100 through the small baseline encoder of tools/jpeg_decode_timing.py (4:2:0, Annex K tables): long
  codes and many 0xff bytes, each followed by its stuffed 0x00."""
  rgb = np.random.default_rng(77).integers(0, 256, size=(40, 56, 3), dtype=np.uint8)
  return _timing_tool().encode_jpeg(rgb, quality=100)


class _BitWriter:
  def __init__(self):
    self.out, self.acc, self.n = bytearray(), 0, 0

  def put(self, value, length):
    self.acc = (self.acc << length) | (value & ((1 << length) - 1))
    self.n += length
    while self.n >= 8:
      byte = (self.acc >> (self.n - 8)) & 0xFF
      self.out.append(byte)
      if byte == 0xFF:
        self.out.append(0)
      self.n -= 8
    self.acc &= (1 << self.n) - 1

  def finish(self):
    if self.n:
      self.put((1 << (8 - self.n)) - 1, 8 - self.n)
    return bytes(self.out)


@functools.lru_cache(maxsize=None)
def three_scans(name='17x9_444_q90'):
  """The coefficients of a 4:4:4 fixture (from the numpy oracle) written as a sequential file of three scans, one
  component each, with the Annex K luminance tables: the same pixels as the fixture, a layout the device path refuses."""
  t = _timing_tool()
  d = J.decode(name)
  assert d.components == 3 and d.h_samp == [1, 1, 1] and d.v_samp == [1, 1, 1]
  dc_code, dc_len = t._codes(t.DC_BITS, t.DC_VALS)
  ac_code, ac_len = t._codes(t.AC_BITS, t.AC_VALS)

  def seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)

  def size_and_bits(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)

  out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
  for c in range(3):
    out += seg(0xDB, bytes([c]) + bytes(int(d.qtables[c][z]) for z in J.ZIGZAG))
  out += seg(0xC0, bytes([8]) + d.height.to_bytes(2, 'big') + d.width.to_bytes(2, 'big') + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 2]))
  out += seg(0xC4, bytes([0x00] + t.DC_BITS + t.DC_VALS)) + seg(0xC4, bytes([0x10] + t.AC_BITS + t.AC_VALS))
  for c in range(3):
    w = _BitWriter()
    pred = 0
    for by in range(d.blocks_h[c]):
      for bx in range(d.blocks_w[c]):
        zz = [int(d.coef[c][by, bx, z]) for z in J.ZIGZAG]
        s, bits = size_and_bits(zz[0] - pred)
        pred = zz[0]
        w.put(int(dc_code[s]), int(dc_len[s]))
        if s:
          w.put(bits, s)
        run = 0
        for k in range(1, 64):
          if zz[k] == 0:
            run += 1
            continue
          while run > 15:
            w.put(int(ac_code[0xF0]), int(ac_len[0xF0]))
            run -= 16
          s, bits = size_and_bits(zz[k])
          w.put(int(ac_code[(run << 4) | s]), int(ac_len[(run << 4) | s]))
          w.put(bits, s)
          run = 0
        if run:
          w.put(int(ac_code[0]), int(ac_len[0]))
    out += seg(0xDA, bytes([1, c + 1, 0x00, 0, 63, 0])) + w.finish()
  return out + b'\xff\xd9'


CORRUPT_SOURCE = '48x80_420_q75'


@functools.lru_cache(maxsize=None)
def truncated_scan():
  """The scan cut in the middle, the EOI marker kept: the header is intact, the segment ends early."""
  raw = J.data(CORRUPT_SOURCE)
  sos = raw.index(b'\xff\xda')
  return raw[:sos + (len(raw) - sos) // 2] + b'\xff\xd9'


_FLIPPED = []


def flipped_byte(lib):
  """One byte in the middle of the scan inverted (never to or from 0xff, so that the markers stay): the first position
  from the middle on at which the host decode calls the stream corrupt."""
  if _FLIPPED:
    return _FLIPPED[0]
  L = lib.lib()
  good = J.data(CORRUPT_SOURCE)
  sos = good.index(b'\xff\xda')
  im = lib.JpegImage()
  lib.check(L.mmt_jpeg_info(good, len(good), ctypes.byref(im)))
  coef, q = J.aligned(im.coef_elems, np.int16), J.aligned(192, np.uint16)
  for at in range(sos + (len(good) - sos) // 2, len(good) - 2):
    if good[at] in (0x00, 0xFF) or good[at - 1] == 0xFF:
      continue
    raw = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
    if L.mmt_jpeg_coefficients(raw, len(raw), ctypes.byref(im), coef.ctypes.data, im.coef_elems, q.ctypes.data) == E_INVALID:
      _FLIPPED.append(raw)
      return raw
  raise AssertionError('no single inverted byte makes the host decode refuse the file')
