"""Times of the PNG decode (csrc/png_decode.hip, mmt_amd.feature_pipeline.decode_png_images) on a batch a data loader
would hand over: 64 files of 1008 x 1008 RGB (BASELINE config 3).  The files are synthesised here with Python's zlib --
no file is read and no library is needed: smooth content plus noise, so that the filters and LZ77 both matter; the filter
type is chosen per row by the smallest sum of absolute differences, as an encoder would.  `--distinct` contents (default
8) are encoded and repeated to fill the batch.

Reported:
  host     mmt_png_inflate over the batch at workers 1 and 16 (wall clock, best of --host-rounds), and Python's
           zlib.decompress of the same streams at the same worker counts: the yardstick for the library's own inflate
  upload   the filtered scanlines, palettes and metadata the device stage takes, by HIP events
  device   mmt_png_pixels by HIP events: warm-up, then rounds of calls; median and range over the rounds; beside it the
           time the bytes it reads and writes would take at the sustained HBM rate that profiles/record_loader_timing.json
           records.  The pixels are checked against the synthesised images before anything is timed.

  inflate  the device inflate (csrc/png_inflate.hip) on the same files in the same run, so that its yardstick -- the host
           rows above: mmt_png_inflate at 16 workers plus its upload -- is measured beside it: mmt_png_gather at workers 1
           and 16, the upload of compressed bytes, palettes, metadata and stream descriptors, mmt_png_scanlines at
           subseq_bytes 16, 32, 64 and 128 by HIP events (median and range over the rounds), and
           decode_png_images(inflate='device') end to end.  Status 0 and the scanlines' bytes are checked against the host
           inflate's before anything is timed.  A second record (--inflate-out).

A record, not a gate: nothing is asserted on the times.  Writes the JSON records (--out, --inflate-out)."""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))


def content(size, seed):
  """uint8 [size, size, 3]: low-frequency waves plus noise of a few levels."""
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
  planes = []
  for c in range(3):
    a, b, p = rng.uniform(1, 6, size=3)
    planes.append(128 + 90 * np.sin(2 * np.pi * (a * xx + p)) * np.cos(2 * np.pi * b * yy) + rng.integers(-3, 4, size=(size, size)))
  return np.clip(np.stack(planes, axis=2), 0, 255).astype(np.uint8)


def encode_png(rgb, level=6):
  """An 8-bit RGB PNG, not interlaced, one IDAT; per row the filter with the smallest sum of absolute differences."""
  h, w = rgb.shape[:2]
  cur = rgb.reshape(h, w * 3).astype(np.int16)
  up = np.concatenate([np.zeros((1, w * 3), dtype=np.int16), cur[:-1]])
  left = np.concatenate([np.zeros((h, 3), dtype=np.int16), cur[:, :-3]], axis=1)
  corner = np.concatenate([np.zeros((h, 3), dtype=np.int16), up[:, :-3]], axis=1)
  p = left + up - corner
  pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - corner)
  paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, corner))
  cands = np.stack([(cur - pred).astype(np.uint8) for pred in (0 * cur, left, up, (left + up) >> 1, paeth)])      # [5, h, w * 3]
  cost = np.abs(cands.view(np.int8).astype(np.int32)).sum(axis=2)                                              # [5, h]
  best = cost.argmin(axis=0)
  rows = cands[best, np.arange(h)]
  raw = np.concatenate([best.astype(np.uint8)[:, None], rows], axis=1).tobytes()
  chunk = lambda t, d: struct.pack('>I', len(d)) + t + d + struct.pack('>I', zlib.crc32(t + d))
  stream = zlib.compress(raw, level)
  png = b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', stream) + chunk(b'IEND', b'')
  return png, stream, np.bincount(best, minlength=5).tolist()


def best_of(rounds, fn):
  best = None
  for _ in range(rounds):
    t0 = time.perf_counter()
    fn()
    dt = time.perf_counter() - t0
    best = dt if best is None else min(best, dt)
  return best


def over(workers, fn, n):
  if workers == 1:
    return [fn(i) for i in range(n)]
  with ThreadPoolExecutor(max_workers=workers) as pool:
    return list(pool.map(fn, range(n)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--size', type=int, default=1008)
  ap.add_argument('--distinct', type=int, default=8, help='contents encoded; repeated to fill the batch')
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=4, help='calls per round (at least 20 calls over all rounds)')
  ap.add_argument('--host-rounds', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_decode_timing.json'))
  ap.add_argument('--inflate-out', default=os.path.join(ROOT, 'profiles', 'png_inflate_timing.json'))
  args = ap.parse_args()
  assert args.rounds * args.calls >= 20

  import torch
  from mmt_amd import _lib
  from mmt_amd import feature_pipeline as fp
  assert torch.cuda.is_available(), 'png_decode_timing needs a GPU'
  L = _lib.lib()
  dev = torch.device('cuda')
  with open(os.path.join(ROOT, 'profiles', 'record_loader_timing.json')) as f:
    hbm = float(json.load(f)['hbm_sustained_gb_per_s'])

  t0 = time.perf_counter()
  made = [(content(args.size, 100 + k),) for k in range(args.distinct)]
  made = [(rgb,) + encode_png(rgb) for (rgb,) in made]
  B = args.batch
  rgbs = [made[i % args.distinct][0] for i in range(B)]
  files = [np.frombuffer(made[i % args.distinct][1], dtype=np.uint8) for i in range(B)]
  streams = [made[i % args.distinct][2] for i in range(B)]
  print(f'{args.distinct} files of {args.size} x {args.size} encoded in {time.perf_counter() - t0:.1f} s: {[len(m[1]) for m in made]} bytes, '
        f'filters per file (None, Sub, Up, Average, Paeth) {[m[3] for m in made]}')

  images = (_lib.PngImage * B)()
  n_raw = n_pix = 0
  for i, a in enumerate(files):
    _lib.check(L.mmt_png_info(a.ctypes.data, a.size, ctypes.byref(images[i])))
    images[i].raw_offset, images[i].pixel_offset = n_raw, n_pix
    n_raw += images[i].raw_bytes
    n_pix += images[i].width * images[i].height * 3
  raw = torch.empty(n_raw, dtype=torch.uint8).pin_memory()
  pal = torch.empty(B * 768, dtype=torch.uint8).pin_memory()
  meta = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8).pin_memory()

  def inflate(i):
    _lib.check(L.mmt_png_inflate(files[i].ctypes.data, files[i].size, ctypes.byref(images[i]), raw.data_ptr(), n_raw, pal.data_ptr() + i * 768))

  host = {}
  for workers in (1, 16):
    host[str(workers)] = {'mmt_png_inflate_ms': round(best_of(args.host_rounds, lambda: over(workers, inflate, B)) * 1e3, 2),
                          'zlib_decompress_ms': round(best_of(args.host_rounds, lambda: over(workers, lambda i: zlib.decompress(streams[i]), B)) * 1e3, 2)}
  for i in range(B):
    assert bytes(raw[images[i].raw_offset:images[i].raw_offset + images[i].raw_bytes].numpy()) == zlib.decompress(streams[i]) or i >= args.distinct
  print(f'  host: mmt_png_inflate {host["1"]["mmt_png_inflate_ms"]} / {host["16"]["mmt_png_inflate_ms"]} ms at 1 / 16 workers; '
        f'zlib.decompress {host["1"]["zlib_decompress_ms"]} / {host["16"]["zlib_decompress_ms"]} ms')

  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  raw_d, pal_d, meta_d = (torch.empty(t.numel(), dtype=torch.uint8, device=dev) for t in (raw, pal, meta))
  ups = []
  for _ in range(6):
    e0.record()
    for d, h in ((raw_d, raw), (pal_d, pal), (meta_d, meta)):
      d.copy_(h, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    ups.append(e0.elapsed_time(e1) * 1e3)
  ups = ups[1:]

  out = torch.empty(n_pix, dtype=torch.uint8, device=dev)
  need = L.mmt_png_workspace_bytes(n_raw)
  work = torch.empty(need, dtype=torch.uint8, device=dev)
  stream = torch.cuda.current_stream(dev).cuda_stream

  def call():
    _lib.check(L.mmt_png_pixels(B, meta_d.data_ptr(), raw_d.data_ptr(), n_raw, pal_d.data_ptr(), out.data_ptr(), n_pix, work.data_ptr(), need, stream))

  for _ in range(3):
    call()
  torch.cuda.synchronize()
  got = out.cpu().numpy()
  for i in range(args.distinct):
    assert np.array_equal(got[images[i].pixel_offset:images[i].pixel_offset + rgbs[i].size], rgbs[i].reshape(-1)), i
  whole = fp.decode_png_images(files, dev, workers=16)[0]
  assert torch.equal(whole, out)
  ts = []
  for _ in range(args.rounds):
    e0.record()
    for _ in range(args.calls):
      call()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / args.calls * 1e3)
  med = statistics.median(ts)
  moved = n_raw + n_pix
  hbm_us = moved / (hbm * 1e3)
  t_all = best_of(args.host_rounds, lambda: (fp.decode_png_images(files, dev, workers=16), torch.cuda.synchronize()))
  rec = {
      'tool': 'tools/png_decode_timing.py', 'device': torch.cuda.get_device_name(0), 'batch': B, 'size': args.size, 'distinct_contents': args.distinct,
      'file_bytes': [len(m[1]) for m in made], 'filters_per_file_none_sub_up_average_paeth': [m[3] for m in made],
      'raw_bytes': n_raw, 'pixel_bytes': n_pix, 'host_ms_by_workers': host,
      'inflate_over_zlib': {w: round(host[w]['mmt_png_inflate_ms'] / host[w]['zlib_decompress_ms'], 2) for w in host},
      'upload_bytes': raw.numel() + pal.numel() + meta.numel(), 'upload_us_median': round(statistics.median(ups), 1),
      'upload_us_min': round(min(ups), 1), 'upload_us_max': round(max(ups), 1),
      'pixels_us_median': round(med, 1), 'pixels_us_min': round(min(ts), 1), 'pixels_us_max': round(max(ts), 1),
      'pixels_rounds': args.rounds, 'pixels_calls_per_round': args.calls, 'launches': 1, 'workspace_bytes': need,
      'hbm_sustained_gb_per_s': hbm, 'bytes_read_and_written': moved, 'hbm_bound_us': round(hbm_us, 1),
      'pixels_over_hbm_bound': round(med / hbm_us, 1),
      'decode_png_images_ms_workers_16': round(t_all * 1e3, 2),
      'host_share_of_stages_workers_16': round(host['16']['mmt_png_inflate_ms'] * 1e3 /
                                               (host['16']['mmt_png_inflate_ms'] * 1e3 + statistics.median(ups) + med), 3)}
  print(f'  upload {rec["upload_bytes"]} bytes: {rec["upload_us_median"]} us; mmt_png_pixels {rec["pixels_us_median"]} us '
        f'({rec["pixels_us_min"]}..{rec["pixels_us_max"]}), HBM bound {rec["hbm_bound_us"]} us; decode_png_images {rec["decode_png_images_ms_workers_16"]} ms')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
    f.write('\n')
  print('wrote', args.out)

  # ---- the device inflate, against the host rows above ----
  streams_c = (_lib.PngStream * B)()
  n_comp = 0
  for i, a in enumerate(files):
    streams_c[i].comp_offset = n_comp
    n_comp += a.size
  comp = torch.empty(n_comp, dtype=torch.uint8).pin_memory()

  def gather(i):
    _lib.check(L.mmt_png_gather(files[i].ctypes.data, files[i].size, ctypes.byref(images[i]), comp.data_ptr(), n_comp, ctypes.byref(streams_c[i]),
                                pal.data_ptr() + i * 768))

  gather_ms = {str(w): round(best_of(args.host_rounds, lambda: over(w, gather, B)) * 1e3, 2) for w in (1, 16)}
  smeta = torch.frombuffer(bytearray(bytes(streams_c)), dtype=torch.uint8).pin_memory()
  comp_d, smeta_d = (torch.empty(t.numel(), dtype=torch.uint8, device=dev) for t in (comp, smeta))
  ups_c = []
  for _ in range(6):
    e0.record()
    for d, h in ((comp_d, comp), (pal_d, pal), (meta_d, meta), (smeta_d, smeta)):
      d.copy_(h, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    ups_c.append(e0.elapsed_time(e1) * 1e3)
  ups_c = ups_c[1:]
  lines_d = torch.empty(n_raw, dtype=torch.uint8, device=dev)
  status_d = torch.empty(B, dtype=torch.int32, device=dev)
  need_inf = L.mmt_png_scanlines_workspace_bytes(B)
  work_inf = torch.empty(need_inf, dtype=torch.uint8, device=dev)
  scan = {}
  for sb in (16, 32, 64, 128):
    def inflate_call():
      _lib.check(L.mmt_png_scanlines(B, meta_d.data_ptr(), smeta_d.data_ptr(), comp_d.data_ptr(), n_comp, lines_d.data_ptr(), n_raw,
                                     status_d.data_ptr(), sb, work_inf.data_ptr(), need_inf, stream))
    lines_d.zero_()
    inflate_call()
    torch.cuda.synchronize()
    assert not bool(status_d.any()), status_d.cpu().tolist()
    assert torch.equal(lines_d, raw_d), sb                      # the host inflate's scanlines, uploaded above
    inflate_call()
    ts = []
    for _ in range(args.rounds):
      e0.record()
      for _ in range(args.calls):
        inflate_call()
      e1.record()
      torch.cuda.synchronize()
      ts.append(e0.elapsed_time(e1) / args.calls * 1e3)
    scan[str(sb)] = {'us_median': round(statistics.median(ts), 1), 'us_min': round(min(ts), 1), 'us_max': round(max(ts), 1)}
    print(f'  mmt_png_scanlines subseq_bytes {sb}: {scan[str(sb)]}')
  one = {}
  for sb in (16, 32, 64, 128):                                  # a single image: the latency of one workgroup
    ts = []
    for _ in range(args.rounds):
      e0.record()
      _lib.check(L.mmt_png_scanlines(1, meta_d.data_ptr(), smeta_d.data_ptr(), comp_d.data_ptr(), n_comp, lines_d.data_ptr(), n_raw,
                                     status_d.data_ptr(), sb, work_inf.data_ptr(), need_inf, stream))
      e1.record()
      torch.cuda.synchronize()
      ts.append(e0.elapsed_time(e1) * 1e3)
    one[str(sb)] = {'us_median': round(statistics.median(ts[1:]), 1), 'us_min': round(min(ts[1:]), 1), 'us_max': round(max(ts[1:]), 1)}
  whole_dev = fp.decode_png_images(files, dev, workers=16, inflate='device')[0]
  assert torch.equal(whole_dev, out)
  t_dev = {str(sb): round(best_of(args.host_rounds, lambda: (fp.decode_png_images(files, dev, workers=16, inflate='device', subseq_bytes=sb),
                                                             torch.cuda.synchronize())) * 1e3, 2) for sb in (16, 32, 64, 128)}
  best_sb = min(scan, key=lambda k: scan[k]['us_median'])
  rec2 = {
      'tool': 'tools/png_decode_timing.py', 'device': torch.cuda.get_device_name(0), 'batch': B, 'size': args.size, 'distinct_contents': args.distinct,
      'file_bytes': [len(m[1]) for m in made], 'raw_bytes': n_raw, 'compressed_bytes': int(sum(s.comp_bytes for s in streams_c)),
      'host_yardstick_same_run': {'mmt_png_inflate_ms_by_workers': {w: host[w]['mmt_png_inflate_ms'] for w in host},
                                  'upload_bytes': rec['upload_bytes'], 'upload_us_median': rec['upload_us_median'],
                                  'pixels_us_median': rec['pixels_us_median'], 'decode_png_images_ms_workers_16': rec['decode_png_images_ms_workers_16']},
      'gather_ms_by_workers': gather_ms,
      'upload_bytes': comp.numel() + pal.numel() + meta.numel() + smeta.numel(), 'upload_us_median': round(statistics.median(ups_c), 1),
      'upload_us_min': round(min(ups_c), 1), 'upload_us_max': round(max(ups_c), 1),
      'scanlines_us_by_subseq_bytes': scan, 'scanlines_one_image_us_by_subseq_bytes': one,
      'scanlines_rounds': args.rounds, 'scanlines_calls_per_round': args.calls, 'launches': 1, 'best_subseq_bytes': int(best_sb),
      'decode_png_images_device_inflate_ms_workers_16_by_subseq_bytes': t_dev,
      'device_stages_ms': round(gather_ms['16'] + statistics.median(ups_c) / 1e3 + scan[best_sb]['us_median'] / 1e3, 2),
      'host_stages_ms': round(host['16']['mmt_png_inflate_ms'] + rec['upload_us_median'] / 1e3, 2)}
  print(f'  gather {gather_ms} ms; upload {rec2["upload_bytes"]} bytes {rec2["upload_us_median"]} us; one image {one}; '
        f'decode_png_images(inflate=device) {t_dev} ms against {rec["decode_png_images_ms_workers_16"]} ms')
  os.makedirs(os.path.dirname(os.path.abspath(args.inflate_out)), exist_ok=True)
  with open(args.inflate_out, 'w') as f:
    json.dump(rec2, f, indent=1)
    f.write('\n')
  print('wrote', args.inflate_out)


if __name__ == '__main__':
  main()
