"""Call times of mmt_rand_augment (csrc/rand_augment.hip) on a batch a data loader would hand over: 256 decoded images
of 384 x 512, packed back to back.  One variant per operation (the whole batch under that operation) and one mixed plan
(`rand_augment_plan` with a seeded generator), timed alternately in one process with HIP events: warm-up, then rounds
of calls; median and range over the rounds.

Bytes moved per call are counted from the shapes: every pixel byte is read once and written once (2 x the pixels);
AutoContrast, Equalize and Contrast read the image a second time for their statistics (3 x).  The affine gather and
the 3 x 3 window re-read neighbours through the caches; those reads are not counted.  For the mixed plan the count
follows the drawn operations.

A record, not a gate: nothing is asserted on the times.  Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

STATS_OPS = (0, 1, 6)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--height', type=int, default=384)
  ap.add_argument('--width', type=int, default=512)
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=20, help='calls per round')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rand_augment_timing.json'))
  args = ap.parse_args()

  import torch
  from mmt_amd import _lib
  from mmt_amd import feature_pipeline as fp
  assert torch.cuda.is_available(), 'rand_augment_timing needs a GPU'
  dev = 'cuda:0'
  B, h, w = args.batch, args.height, args.width
  per_image = h * w * 3
  g = torch.Generator(dev).manual_seed(0)
  pixels = torch.randint(0, 256, (B * per_image,), dtype=torch.uint8, device=dev, generator=g)
  offsets = torch.arange(B, dtype=torch.int64, device=dev) * per_image
  heights = torch.full((B,), h, dtype=torch.int32, device=dev)
  widths = torch.full((B,), w, dtype=torch.int32, device=dev)
  out = torch.empty_like(pixels)
  L = _lib.lib()
  need = L.mmt_rand_augment_workspace_bytes(B)
  ws = torch.empty(need, dtype=torch.uint8, device=dev)
  stream = torch.cuda.current_stream(dev).cuda_stream

  plans = {}
  for i, name in enumerate(fp.RAND_AUGMENT_OPS):
    plans[name] = fp.rand_augment_plan(heights, widths, ops=torch.full((B,), i, device=dev), generator=g)
  plans['mixed'] = fp.rand_augment_plan(heights, widths, generator=g)
  plans['copy'] = (torch.full((B,), -1, dtype=torch.int32, device=dev), torch.zeros(B, 8, device=dev))

  def call(plan):
    op, arg = plan
    _lib.check(L.mmt_rand_augment(B, pixels.data_ptr(), pixels.numel(), offsets.data_ptr(), heights.data_ptr(),
                                  widths.data_ptr(), op.data_ptr(), arg.data_ptr(), out.data_ptr(), ws.data_ptr(), need, stream))

  def bytes_moved(plan):
    ops = plan[0].tolist()
    return sum(per_image * (3 if i in STATS_OPS else 2) for i in ops)

  for plan in plans.values():          # warm-up
    for _ in range(2):
      call(plan)
  torch.cuda.synchronize()
  times = {name: [] for name in plans}
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for _ in range(args.rounds):
    for name, plan in plans.items():
      e0.record()
      for _ in range(args.calls):
        call(plan)
      e1.record()
      torch.cuda.synchronize()
      times[name].append(e0.elapsed_time(e1) / args.calls * 1e3)
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls,
            'shape': dict(B=B, height=h, width=w, pixel_bytes=B * per_image),
            'bytes_rule': '2 x pixels; 3 x for AutoContrast, Equalize, Contrast (statistics pass)', 'variants': {}}
  print(f'  {"plan":<14} {"us (min..max)":>28} {"GB/s":>8}')
  for name, ts in times.items():
    med, nbytes = statistics.median(ts), bytes_moved(plans[name])
    rec = {'us_median': round(med, 1), 'us_min': round(min(ts), 1), 'us_max': round(max(ts), 1), 'bytes': nbytes,
           'gb_per_s': round(nbytes / med / 1e3, 1)}
    record['variants'][name] = rec
    print(f'  {name:<14} {rec["us_median"]:>10} ({rec["us_min"]}..{rec["us_max"]}) {rec["gb_per_s"]:>8}')
  if 'mixed' in plans:
    drawn = plans['mixed'][0].tolist()
    record['mixed_ops'] = {name: drawn.count(i) for i, name in enumerate(fp.RAND_AUGMENT_OPS)}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
