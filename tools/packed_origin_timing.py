"""Attention forward / backward call times of packed multimodal examples (`example_starts=`, MMT_FLAG_EXAMPLE_STARTS) at
B=4, S=4096, N=12, D=64, bf16, 2-D ids (P = 14, r = 2, R = 49, m = 12), radius >= S: 16 examples of 256 tokens per row.
Routes, timed alternately in one process (HIP events, warm-up, rounds of calls):

  origin  : example ids + starts, the ORG instantiations (per-example 2-D ids)
  ids     : example ids alone, the PACK instantiations (same tiles, row-aligned ids: not the same result)
  dense   : the dense operator on the materialised per-example mask and ids -- the only correct route before

and one grid line, two 2048-token examples per row, P = 44, grid radius 1, 1-D ids, radius 64:

  grid-origin : ids + starts with the image grid on the structured kernels
  grid-dense  : the dense operator on the composed mask and ids

and one line for the walk of blocks inside one example when the band spans the row: 16 x 256 as above with the grid on
(P = 14, grid radius 1, 2-D ids, radius >= S).  The grid adds no pair there, so `grid16-origin` should cost what `origin`
costs; a walk that were not cut to the example would visit 128 tiles per block instead of 8.

Nothing is asserted on the times.  Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=5, help='calls per round of the structured routes (the dense ones: 1)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_origin_timing.json'))
  args = ap.parse_args()

  import torch
  import mmt_amd
  from mmt_amd import ops
  assert torch.cuda.is_available(), 'packed_origin_timing needs a GPU'
  dev, dt = 'cuda:0', torch.bfloat16
  B, S, N, D, R, m = 4, 4096, 12, 64, 49, 12
  torch.manual_seed(0)
  q, k, v, dout = (torch.randn(B, S, N, D, device=dev, dtype=dt) for _ in range(4))
  emb = (torch.randn(R, N, D, device=dev) * 0.5).to(dt)
  bias = (torch.randn(R, N, device=dev) * 0.5).to(dt)
  P = mmt_amd.AttentionPattern

  def layout(L):
    rows = [[L] * (S // L)] * B
    ids, starts, _, _ = mmt_amd.packed_example_layout(rows, [[True] * len(r) for r in rows], S, device=dev)
    return ids, starts

  variants = {}
  ids, starts = layout(256)
  pat = P(local_radius=1 << 30, id_mode=2, max_dist=m, patches_per_row=14, core_layers=2)
  variants['origin'] = dict(pattern=pat, example_ids=ids, example_starts=starts)
  variants['ids'] = dict(pattern=pat, example_ids=ids)
  mask, rel = ops._materialized(pat, None, B, S, torch.device(dev), ids, starts)
  variants['dense'] = dict(att_mask=mask, relative_att_ids=rel)
  variants['grid16-origin'] = dict(pattern=P(local_radius=1 << 30, id_mode=2, max_dist=m, patches_per_row=14, core_layers=2,
                                             grid_radius=1, grid_start=2), example_ids=ids, example_starts=starts)
  gids, gstarts = layout(2048)
  gpat = P(local_radius=64, id_mode=1, max_dist=m, patches_per_row=44, grid_radius=1, grid_start=2)
  variants['grid-origin'] = dict(pattern=gpat, example_ids=gids, example_starts=gstarts)
  gmask, grel = ops._materialized(gpat, None, B, S, torch.device(dev), gids, gstarts)
  variants['grid-dense'] = dict(att_mask=gmask, relative_att_ids=grel)

  calls, outs = {}, {}
  for name, kw in variants.items():
    e, bs = (emb, bias) if not name.startswith('grid-') else (emb[:32].contiguous(), bias[:32].contiguous())
    out, lse = mmt_amd.relative_attention_forward(q, k, v, e, bs, **kw)
    outs[name] = out.float()
    calls[name] = (lambda kw=kw, e=e, bs=bs: mmt_amd.relative_attention_forward(q, k, v, e, bs, **kw),
                   lambda kw=kw, e=e, bs=bs, out=out, lse=lse: mmt_amd.relative_attention_backward(dout, q, k, v, e, bs, out, lse, **kw))
  parity = {'origin_vs_dense': float((outs['origin'] - outs['dense']).abs().max()),
            'grid_origin_vs_dense': float((outs['grid-origin'] - outs['grid-dense']).abs().max()),
            'grid16_origin_vs_dense': float((outs['grid16-origin'] - outs['dense']).abs().max()),
            'ids_vs_dense': float((outs['ids'] - outs['dense']).abs().max())}
  del outs
  times = {name: {'fwd': [], 'bwd': []} for name in calls}
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for name, (f, b) in calls.items():           # warm-up
    for _ in range(2):
      f(); b()
  torch.cuda.synchronize()
  for _ in range(args.rounds):
    for name, (f, b) in calls.items():
      n_calls = 1 if name.endswith('dense') else args.calls
      for kind, fn in (('fwd', f), ('bwd', b)):
        e0.record()
        for _ in range(n_calls):
          fn()
        e1.record()
        torch.cuda.synchronize()
        times[name][kind].append(e0.elapsed_time(e1) / n_calls * 1e3)
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls,
            'shape': dict(B=B, S=S, N=N, D=D, R=R, dtype='bf16'), 'max_abs_diff': parity, 'variants': {}}
  for name in variants:
    rec = {}
    for kind in ('fwd', 'bwd'):
      ts = times[name][kind]
      rec.update({f'{kind}_us_median': round(statistics.median(ts), 1), f'{kind}_us_min': round(min(ts), 1),
                  f'{kind}_us_max': round(max(ts), 1)})
    record['variants'][name] = rec
  g = record['variants']
  record['time_ratios'] = {kind: {'origin_vs_ids': round(g['origin'][f'{kind}_us_median'] / g['ids'][f'{kind}_us_median'], 3),
                                  'grid16_origin_vs_origin': round(g['grid16-origin'][f'{kind}_us_median'] / g['origin'][f'{kind}_us_median'], 3),
                                  'dense_vs_origin': round(g['dense'][f'{kind}_us_median'] / g['origin'][f'{kind}_us_median'], 1),
                                  'grid_dense_vs_origin': round(g['grid-dense'][f'{kind}_us_median'] / g['grid-origin'][f'{kind}_us_median'], 1)}
                           for kind in ('fwd', 'bwd')}
  print(f'  {"route":<12} {"fwd us (min..max)":>28} {"bwd us (min..max)":>30}')
  for name, rec in g.items():
    print(f'  {name:<12} {rec["fwd_us_median"]:>10} ({rec["fwd_us_min"]}..{rec["fwd_us_max"]}) {rec["bwd_us_median"]:>12} ({rec["bwd_us_min"]}..{rec["bwd_us_max"]})')
  print('  max |diff|', json.dumps(parity))
  print('  ratios', json.dumps(record['time_ratios']))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
