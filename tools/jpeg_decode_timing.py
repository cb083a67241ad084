"""Times of the JPEG decode (csrc/jpeg_decode.hip, mmt_amd.feature_pipeline.decode_jpeg_images) on a batch a data
loader would hand over: 64 images of 1008 x 1008 (BASELINE config 3), 4:2:0, quality 90, random content.  The files are
synthesised here by a small baseline encoder in numpy (Annex K tables, float DCT) -- no file is read and no library is
needed; `--distinct` contents (default 8) are encoded and repeated to fill the batch, since random content of one size
costs the decoder the same whichever seed made it.

Reported:
  host     mmt_jpeg_coefficients over the batch at workers 1, 8 and 16 (wall clock, best of --host-rounds), per image
  upload   bytes of coefficients, tables and metadata the device stage takes, against the decoded pixels' bytes
  device   mmt_jpeg_pixels by HIP events: warm-up, then rounds of calls; median and range over the rounds
  pillow   where Pillow is installed: its decode of the same files in one thread plus the upload of the pixels
  entropy  the device entropy decode (csrc/jpeg_entropy.hip) on the same files, for subseq_bytes 64, 128, 256 and 512:
           mmt_jpeg_scan_plan over the batch at workers 1, 8 and 16; the upload of the file bytes and plans; the rounds
           each file needed (a call with a generous max_rounds, then the per-round changed words), as a histogram;
           mmt_jpeg_entropy by HIP events at max_rounds = the most any file needed + 2; and that sum against the host
           decode at 16 workers plus its coefficient upload, from this same run.  The coefficients are checked against
           mmt_jpeg_coefficients' before anything is timed.

A record, not a gate: nothing is asserted on the times.  Writes one JSON record (--out)."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
          100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_VALS = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
           0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
           0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
           0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
           0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
           0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
           0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
           0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def _codes(bits, vals):
  """symbol -> (code, length) as two arrays of 256 entries."""
  code_of, len_of = np.zeros(256, dtype=np.uint64), np.zeros(256, dtype=np.int64)
  code, k = 0, 0
  for length in range(1, 17):
    for _ in range(bits[length - 1]):
      code_of[vals[k]], len_of[vals[k]] = code, length
      code += 1
      k += 1
    code <<= 1
  return code_of, len_of


def _quant(base, quality):
  scale = 5000 // quality if quality < 50 else 200 - 2 * quality
  return np.clip((np.array(base) * scale + 50) // 100, 1, 255).astype(np.int64)


def _blocks(plane, q):
  """[H, W] float (multiples of 8) -> quantised DCT coefficients int64 [H/8, W/8, 64] in zigzag order."""
  k = np.arange(8)
  C = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))
  h, w = plane.shape
  x = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
  d = C @ x @ C.T
  return np.rint(d.reshape(h // 8, w // 8, 64) / q).astype(np.int64)[..., ZIGZAG]


def _size(v):
  a = np.abs(v)
  return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def encode_jpeg(rgb, quality=90):
  """Baseline 4:2:0 JPEG of a uint8 [h, w, 3] array: JFIF colour, 2 x 2 box-averaged chroma, one interleaved scan."""
  h, w = rgb.shape[:2]
  H, W = -(-h // 16) * 16, -(-w // 16) * 16
  x = np.pad(rgb.astype(np.float64), ((0, H - h), (0, W - w), (0, 0)), mode='edge')
  r, g, b = x[..., 0], x[..., 1], x[..., 2]
  y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
  cb = (-0.168736 * r - 0.331264 * g + 0.5 * b).reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
  cr = (0.5 * r - 0.418688 * g - 0.081312 * b).reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
  ql, qc = _quant(Q_LUMA, quality), _quant(Q_CHROMA, quality)
  by, bcb, bcr = _blocks(y, ql[ZIGZAG]), _blocks(cb, qc[ZIGZAG]), _blocks(cr, qc[ZIGZAG])
  my, mx = H // 16, W // 16
  ymcu = by.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, 4, 64)       # Y00 Y01 Y10 Y11 per MCU
  z = np.concatenate([ymcu, bcb.reshape(-1, 1, 64), bcr.reshape(-1, 1, 64)], axis=1)        # [MCUs, 6, 64]
  n = z.shape[0]
  for lo, hi in ((0, 4), (4, 5), (5, 6)):                       # DC prediction per component, in scan order
    dc = z[:, lo:hi, 0].reshape(-1)
    z[:, lo:hi, 0] = np.diff(dc, prepend=0).reshape(n, hi - lo)
  z = z.reshape(n * 6, 64)
  dc_code, dc_len = _codes(DC_BITS, DC_VALS)
  ac_code, ac_len = _codes(AC_BITS, AC_VALS)

  size = _size(z)
  bits = np.where(z < 0, z + (1 << size) - 1, z).astype(np.uint64)
  val = np.zeros((n * 6, 65), dtype=np.uint64)                  # one entry per coefficient, [64] is the end of block
  length = np.zeros((n * 6, 65), dtype=np.int64)
  val[:, 0] = (dc_code[size[:, 0]] << size[:, 0].astype(np.uint64)) | bits[:, 0]
  length[:, 0] = dc_len[size[:, 0]] + size[:, 0]
  nz = z != 0
  nz[:, 0] = True                                               # runs count from the DC position
  pos = np.where(nz, np.arange(64)[None, :], 0)
  prev = np.maximum.accumulate(pos, axis=1)
  prev = np.concatenate([np.zeros((n * 6, 1), dtype=np.int64), prev[:, :-1]], axis=1)       # last non-zero position before k
  run = np.arange(64)[None, :] - prev - 1
  ac = (z != 0) & (np.arange(64)[None, :] > 0)
  sym = ((run & 15) << 4) | size
  v = (ac_code[sym] << size.astype(np.uint64)) | bits
  ln = ac_len[sym] + size
  zrl_code, zrl_len = ac_code[0xF0], int(ac_len[0xF0])
  for count in (1, 2, 3):                                       # runs of 16 and more: ZRL symbols in front
    many = ac & ((run >> 4) == count)
    prefix = np.uint64(0)
    for _ in range(count):
      prefix = (prefix << np.uint64(zrl_len)) | zrl_code
    v = np.where(many, (prefix << ln.astype(np.uint64)) | v, v)
    ln = np.where(many, ln + count * zrl_len, ln)
  val[:, :64] = np.where(ac, v, val[:, :64])
  length[:, :64] = np.where(ac, ln, length[:, :64])
  last = np.where(ac, np.arange(64)[None, :], 0).max(axis=1)
  val[:, 64] = np.where(last < 63, ac_code[0x00], 0)
  length[:, 64] = np.where(last < 63, ac_len[0x00], 0)

  keep = length.reshape(-1) > 0
  val, length = val.reshape(-1)[keep], length.reshape(-1)[keep]
  start = np.cumsum(length) - length
  total = int(start[-1] + length[-1])
  idx = np.repeat(np.arange(val.size, dtype=np.int32), length)
  shift = (length[idx] - 1 - (np.arange(total, dtype=np.int64) - start[idx])).astype(np.uint64)
  stream = ((val[idx] >> shift) & np.uint64(1)).astype(np.uint8)
  stream = np.concatenate([stream, np.ones((-total) % 8, dtype=np.uint8)])
  data = np.packbits(stream)
  data = np.insert(data, np.nonzero(data == 0xFF)[0] + 1, 0)    # byte stuffing

  def seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)

  out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
  out += seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist())) + seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
  out += seg(0xC0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
  out += seg(0xC4, bytes([0x00] + DC_BITS + DC_VALS)) + seg(0xC4, bytes([0x10] + AC_BITS + AC_VALS))
  out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x00, 3, 0x00, 0, 63, 0]))
  return out + data.tobytes() + b'\xff\xd9'


def entropy_leg(torch, _lib, L, bufs, images, n_coef, coef_d, dev, args):
  """The device entropy decode of the batch; coef_d: the host decode's coefficients on the device, the yardstick."""
  B = len(bufs)
  img_d = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8).to(dev)
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  stream = torch.cuda.current_stream(dev).cuda_stream
  generous = 64
  out = {}
  for sb in (64, 128, 256, 512):
    def plan(i):
      a, scan = bufs[i], _lib.JpegScan()
      _lib.check(L.mmt_jpeg_scan_plan(a.ctypes.data, a.size, ctypes.byref(images[i]), sb, ctypes.byref(scan), None, None, None, 0, None, 0))
      huff, qt = np.empty(6 * _lib.MMT_JPEG_HUFF_WORDS, dtype=np.uint32), np.empty(192, dtype=np.uint16)
      seg, sub = np.empty(scan.n_segments * 4, dtype=np.int32), np.empty(scan.n_subseq, dtype=np.int32)
      _lib.check(L.mmt_jpeg_scan_plan(a.ctypes.data, a.size, ctypes.byref(images[i]), sb, ctypes.byref(scan), huff.ctypes.data, qt.ctypes.data,
                                      seg.ctypes.data, scan.n_segments, sub.ctypes.data, scan.n_subseq))
      return scan, huff, qt, seg, sub

    plan_ms = {}
    for workers in (1, 8, 16):
      best = None
      for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        if workers == 1:
          plans = [plan(i) for i in range(B)]
        else:
          with ThreadPoolExecutor(max_workers=workers) as pool:
            plans = list(pool.map(plan, range(B)))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
      plan_ms[str(workers)] = round(best * 1e3, 2)
    scans = (_lib.JpegScan * B)()
    at_b = at_seg = at_sub = 0
    for i, (scan, _, _, _, _) in enumerate(plans):
      scan.byte_offset += at_b
      scan.segment_offset, scan.subseq_offset = at_seg, at_sub
      scans[i] = scan
      at_b += bufs[i].size; at_seg += scan.n_segments; at_sub += scan.n_subseq
    max_sub = max(sc.n_subseq for sc in scans)
    pin = lambda a: torch.from_numpy(np.array(a, copy=True).view(np.uint8)).pin_memory()
    host_parts = [pin(np.concatenate(bufs)), pin(np.concatenate([pl[1] for pl in plans])), pin(np.concatenate([pl[3] for pl in plans])),
                  pin(np.concatenate([pl[4] for pl in plans])), pin(np.frombuffer(bytes(scans), dtype=np.uint8))]
    dev_parts = [torch.empty(h.numel() + 16, dtype=torch.uint8, device=dev)[:h.numel()] for h in host_parts]
    ups = []
    for _ in range(5):
      e0.record()
      for d, h in zip(dev_parts, host_parts):
        d.copy_(h, non_blocking=True)
      e1.record()
      torch.cuda.synchronize()
      ups.append(e0.elapsed_time(e1) * 1e3)
    bytes_d, huff_d, seg_d, sub_d, scan_d = dev_parts
    coef_e = torch.empty(n_coef, dtype=torch.int16, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)

    def call(rounds, ws):
      _lib.check(L.mmt_jpeg_entropy(B, bytes_d.data_ptr(), at_b, img_d.data_ptr(), scan_d.data_ptr(), huff_d.data_ptr(), seg_d.data_ptr(),
                                    at_seg, sub_d.data_ptr(), at_sub, max_sub, sb, rounds, coef_e.data_ptr(), n_coef, status.data_ptr(),
                                    ws.data_ptr(), ws.numel(), stream))

    ws = torch.empty(L.mmt_jpeg_entropy_workspace_bytes(B, at_sub, max_sub, sb, generous), dtype=torch.uint8, device=dev)
    coef_e.fill_(0x5555)
    call(generous, ws)
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0, status.tolist()
    assert torch.equal(coef_e, coef_d), 'the device entropy decode differs from mmt_jpeg_coefficients'
    changed = ws[:generous * B * 4].view(torch.int32).reshape(generous, B).cpu().numpy()
    needed = [int(np.nonzero(changed[:, b])[0].max()) + 1 for b in range(B)]         # rounds that changed a state of the file
    most = max(needed)
    assert most < generous
    call(most, ws)                                              # the smallest max_rounds at which no file falls back
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0, (most, status.tolist())
    fallbacks_below = 0
    if most > 1:
      call(most - 1, ws)
      torch.cuda.synchronize()
      fallbacks_below = int((status != 0).sum())
    rounds = most + 2
    ws = torch.empty(L.mmt_jpeg_entropy_workspace_bytes(B, at_sub, max_sub, sb, rounds), dtype=torch.uint8, device=dev)
    for _ in range(3):
      call(rounds, ws)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.rounds):
      e0.record()
      for _ in range(args.calls):
        call(rounds, ws)
      e1.record()
      torch.cuda.synchronize()
      ts.append(e0.elapsed_time(e1) / args.calls * 1e3)
    assert int(status.abs().max()) == 0 and torch.equal(coef_e, coef_d)
    med = statistics.median(ts)
    out[str(sb)] = {
        'plan_ms_by_workers': plan_ms, 'upload_bytes': sum(h.numel() for h in host_parts), 'upload_us_median': round(statistics.median(ups), 1),
        'subsequences': at_sub, 'segments': at_seg, 'rounds_needed_histogram': {str(k): needed.count(k) for k in sorted(set(needed))},
        'smallest_max_rounds_without_fallback': most, 'files_falling_back_one_round_below': fallbacks_below, 'max_rounds_timed': rounds,
        'launches': rounds + 5, 'entropy_us_median': round(med, 1), 'entropy_us_min': round(min(ts), 1), 'entropy_us_max': round(max(ts), 1),
        'workspace_bytes': ws.numel()}
    print(f'  device entropy, subseq_bytes {sb:>3}: plan {plan_ms["1"]} / {plan_ms["8"]} / {plan_ms["16"]} ms at 1 / 8 / 16 workers, upload '
          f'{out[str(sb)]["upload_us_median"]} us, rounds needed {out[str(sb)]["rounds_needed_histogram"]}, mmt_jpeg_entropy {round(med, 1)} us '
          f'({round(min(ts), 1)}..{round(max(ts), 1)}) at max_rounds {rounds}')
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--size', type=int, default=1008)
  ap.add_argument('--quality', type=int, default=90)
  ap.add_argument('--distinct', type=int, default=8, help='contents encoded; repeated to fill the batch')
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=4, help='calls per round (at least 20 calls over all rounds)')
  ap.add_argument('--host-rounds', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_decode_timing.json'))
  args = ap.parse_args()
  assert args.rounds * args.calls >= 20

  import torch
  from mmt_amd import _lib
  from mmt_amd import feature_pipeline as fp
  assert torch.cuda.is_available(), 'jpeg_decode_timing needs a GPU'
  dev = 'cuda:0'
  L = _lib.lib()
  B, S = args.batch, args.size
  rng = np.random.default_rng(0)
  t0 = time.perf_counter()
  distinct = [encode_jpeg(rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8), args.quality) for _ in range(min(args.distinct, B))]
  files = [distinct[i % len(distinct)] for i in range(B)]
  print(f'encoded {len(distinct)} contents in {time.perf_counter() - t0:.1f} s; {len(files[0])} bytes per file')
  bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]

  images = (_lib.JpegImage * B)()
  n_coef = n_pix = 0
  for i, a in enumerate(bufs):
    _lib.check(L.mmt_jpeg_info(a.ctypes.data, a.size, ctypes.byref(images[i])))
    for c in range(3):
      images[i].coef_offset[c] += n_coef
    images[i].pixel_offset = n_pix
    n_coef += images[i].coef_elems
    n_pix += images[i].width * images[i].height * 3
  coef = torch.empty(n_coef, dtype=torch.int16, pin_memory=True)
  qtab = torch.empty(B * 192, dtype=torch.int16, pin_memory=True)

  def entropy(i):
    return L.mmt_jpeg_coefficients(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(images[i]), coef.data_ptr(), n_coef,
                                   qtab.data_ptr() + i * 384)

  host = {}
  for workers in (1, 8, 16):
    best = None
    for _ in range(args.host_rounds):
      t0 = time.perf_counter()
      if workers == 1:
        rcs = [entropy(i) for i in range(B)]
      else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
          rcs = list(pool.map(entropy, range(B)))
      dt = time.perf_counter() - t0
      assert not any(rcs), L.mmt_last_error()
      best = dt if best is None else min(best, dt)
    host[str(workers)] = {'batch_ms': round(best * 1e3, 1), 'per_image_ms': round(best * 1e3 / B, 2)}
    print(f'  host entropy decode, workers {workers:>2}: {best * 1e3:8.1f} ms per batch, {best * 1e3 / B:6.2f} ms per image')

  meta = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8)
  coef_d, qtab_d, meta_d = coef.to(dev), qtab.to(dev), meta.to(dev)
  out = torch.empty(n_pix, dtype=torch.uint8, device=dev)
  need = L.mmt_jpeg_workspace_bytes(n_coef)
  ws = torch.empty(need, dtype=torch.uint8, device=dev)
  stream = torch.cuda.current_stream(dev).cuda_stream

  def call():
    _lib.check(L.mmt_jpeg_pixels(B, meta_d.data_ptr(), coef_d.data_ptr(), n_coef, qtab_d.data_ptr(), out.data_ptr(), n_pix,
                                 ws.data_ptr(), need, stream))

  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for _ in range(3):
    call()
  torch.cuda.synchronize()
  ts = []
  for _ in range(args.rounds):
    e0.record()
    for _ in range(args.calls):
      call()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / args.calls * 1e3)
  # bytes the two passes move at the least: coefficients in, planes out and in again, pixels out
  moved = n_coef * 2 + n_coef * 2 + n_pix
  med = statistics.median(ts)
  device = {'us_median': round(med, 1), 'us_min': round(min(ts), 1), 'us_max': round(max(ts), 1), 'bytes_min': moved,
            'gb_per_s': round(moved / med / 1e3, 1), 'per_image_us': round(med / B, 1)}
  print(f'  device mmt_jpeg_pixels: {device["us_median"]} us ({device["us_min"]}..{device["us_max"]}) per batch of {B}, '
        f'{device["gb_per_s"]} GB/s over {moved} bytes')

  ups = []
  for _ in range(5):                                            # the asynchronous upload of what stage 2 takes
    e0.record()
    coef_d.copy_(coef, non_blocking=True); qtab_d.copy_(qtab, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    ups.append(e0.elapsed_time(e1) * 1e3)
  upload = {'coef_bytes': n_coef * 2, 'table_bytes': B * 384, 'metadata_bytes': meta.numel(), 'file_bytes': sum(len(f) for f in files),
            'pixel_bytes': n_pix, 'us_median': round(statistics.median(ups), 1)}
  print(f'  upload: {upload["coef_bytes"]} coefficient bytes ({upload["us_median"]} us) against {n_pix} pixel bytes')

  record = {'device': torch.cuda.get_device_name(0), 'shape': dict(B=B, size=S, quality=args.quality, sampling='4:2:0', distinct=len(distinct)),
            'host_entropy_decode': host, 'upload': upload, 'device_stage': device, 'rounds': args.rounds, 'calls_per_round': args.calls}
  record['device_entropy'] = entropy_leg(torch, _lib, L, bufs, images, n_coef, coef_d, dev, args)
  fastest = min(record['device_entropy'], key=lambda k: record['device_entropy'][k]['entropy_us_median'])
  best = record['device_entropy'][fastest]
  record['device_entropy_summary'] = {
      'fastest_subseq_bytes': int(fastest), 'max_rounds_default': best['smallest_max_rounds_without_fallback'] + 2,
      'host_path_ms': round(host['16']['batch_ms'] + upload['us_median'] / 1e3, 2),
      'device_path_ms': round(best['plan_ms_by_workers']['16'] + (best['upload_us_median'] + best['entropy_us_median']) / 1e3, 2),
      'note': 'host_path: mmt_jpeg_coefficients at 16 workers + coefficient upload; device_path: mmt_jpeg_scan_plan at 16 workers + upload of '
              'bytes and plans + mmt_jpeg_entropy; both in front of the same mmt_jpeg_pixels'}
  print('  ', record['device_entropy_summary'])
  got = fp.decode_jpeg_images(files[:2], dev)[0].cpu().numpy()
  got_device = fp.decode_jpeg_images(files[:2], dev, entropy='device')[0].cpu().numpy()
  assert np.array_equal(got, got_device), "entropy='device' differs from entropy='host'"
  try:
    from PIL import Image
  except ImportError:
    record['pillow'] = None
    print('  Pillow: not installed on this machine')
  else:
    want = np.concatenate([np.asarray(Image.open(io.BytesIO(f)).convert('RGB')).reshape(-1) for f in files[:2]])
    assert np.array_equal(got, want), 'the decode differs from Pillow on the synthesised files'
    pin = torch.empty(n_pix, dtype=torch.uint8, pin_memory=True)
    view = pin.numpy()
    t0 = time.perf_counter()
    at = 0
    for f in files:
      a = np.asarray(Image.open(io.BytesIO(f)).convert('RGB')).reshape(-1)
      view[at:at + a.size] = a
      at += a.size
    out.copy_(pin, non_blocking=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    record['pillow'] = {'decode_and_upload_ms': round(dt * 1e3, 1), 'per_image_ms': round(dt * 1e3 / B, 2), 'threads': 1}
    print(f'  Pillow decode (1 thread) + pixel upload: {dt * 1e3:.1f} ms per batch, {dt * 1e3 / B:.2f} ms per image')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
