"""Attention forward / backward call times with packed examples (`example_ids=`, MMT_FLAG_EXAMPLE_IDS) at
B=4, S=4096, N=12, D=64, bf16, 1-D ids (R = 32, m = 12), no global tokens: 16 examples of 256 tokens per row.
Variants, timed alternately in one process (HIP events, warm-up, rounds of calls):

  (a) radius 64 -- the price of the id compare
    r64-packed   : example ids, the general kernels' PACK instantiations
    r64-general  : valid_len on the general kernels (reached, as tools/grid_attn_timing.py does, with a grid that adds no
                   pair: a = 1 over a one-patch image at position 0)
    r64-default  : valid_len on today's default (lean bf16) kernels, for scale
  (b) radius >= S -- full attention inside each example, what tile skipping is for
    full-packed   : example ids: 16 * 8 * 8 = 1024 key tiles per plane visited
    full-unpacked : the same PACK kernels with one example per row (ids all 1): 128 * 128 = 16384 tiles
    full-dense    : the dense operator on the materialised [B,S,S] mask of the packed rows (the only route before)

The one condition checked here: full-packed is faster than both other (b) variants, forward and backward.  Writes one
JSON record (--out)."""
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
  ap.add_argument('--calls', type=int, default=5, help='calls per round (50 per point over the default rounds)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_attn_timing.json'))
  args = ap.parse_args()

  import torch
  import mmt_amd
  assert torch.cuda.is_available(), 'packed_attn_timing needs a GPU'
  dev, dt = 'cuda:0', torch.bfloat16
  B, S, N, D, R, m, L = 4, 4096, 12, 64, 32, 12, 256
  n_ex, n_tiles = S // L, S // 32
  torch.manual_seed(0)
  q, k, v, dout = (torch.randn(B, S, N, D, device=dev, dtype=dt) for _ in range(4))
  emb = (torch.randn(R, N, D, device=dev) * 0.5).to(dt)
  bias = (torch.randn(R, N, device=dev) * 0.5).to(dt)
  ids = mmt_amd.example_ids_from_lengths([[L] * n_ex] * B, S, device=dev)
  ones = torch.ones_like(ids)
  P = mmt_amd.AttentionPattern
  band, full = dict(local_radius=64, id_mode=1, max_dist=m), dict(local_radius=1 << 30, id_mode=1, max_dist=m)
  band_tiles = sum(min(x0 + 31 + 64, S - 1) // 32 - max(x0 - 64, 0) // 32 + 1 for x0 in range(0, S, 32))
  variants = {        # name: (keywords, key tiles visited per plane)
      'r64-packed': (dict(pattern=P(**band), example_ids=ids), band_tiles),
      'r64-general': (dict(pattern=P(**band, patches_per_row=1, grid_radius=1, grid_start=0)), band_tiles),
      'r64-default': (dict(pattern=P(**band)), band_tiles),
      'full-packed': (dict(pattern=P(**full), example_ids=ids), n_ex * (L // 32) ** 2),
      'full-unpacked': (dict(pattern=P(**full), example_ids=ones), n_tiles ** 2),
  }
  att = (ids[:, :, None] == ids[:, None, :]).to(torch.int32)
  rel = mmt_amd.side_inputs(P(**full), torch.full((B,), S, dtype=torch.int32, device=dev),
                            torch.zeros(B, dtype=torch.int32, device=dev), S, want_mask=False,
                            want_segment_ids=False)['relative_att_ids']
  variants['full-dense'] = (dict(att_mask=att, relative_att_ids=rel), n_tiles ** 2)
  calls, outs = {}, {}
  for name, (kw, _) in variants.items():
    out, lse = mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw)
    outs[name] = out.float()
    calls[name] = (lambda kw=kw: mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw),
                   lambda kw=kw, out=out, lse=lse: mmt_amd.relative_attention_backward(dout, q, k, v, emb, bias, out, lse, **kw))
  parity = {'full_packed_vs_dense': float((outs['full-packed'] - outs['full-dense']).abs().max())}
  del outs
  times = {name: {'fwd': [], 'bwd': []} for name in calls}
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for name, (f, b) in calls.items():           # warm-up
    for _ in range(2):
      f(); b()
  torch.cuda.synchronize()
  for _ in range(args.rounds):
    for name, (f, b) in calls.items():
      n_calls = 1 if name == 'full-dense' else args.calls       # (milliseconds per call: one call is a long interval already)
      for kind, fn in (('fwd', f), ('bwd', b)):
        e0.record()
        for _ in range(n_calls):
          fn()
        e1.record()
        torch.cuda.synchronize()
        times[name][kind].append(e0.elapsed_time(e1) / n_calls * 1e3)
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls,
            'shape': dict(B=B, S=S, N=N, D=D, R=R, dtype='bf16', examples_per_row=n_ex, example_len=L),
            'max_abs_diff': parity, 'variants': {}}
  for name, (_, tiles) in variants.items():
    rec = {'tiles_per_plane': tiles}
    for kind in ('fwd', 'bwd'):
      ts = times[name][kind]
      rec.update({f'{kind}_us_median': round(statistics.median(ts), 1), f'{kind}_us_min': round(min(ts), 1),
                  f'{kind}_us_max': round(max(ts), 1)})
    record['variants'][name] = rec
  g = record['variants']
  ratios = {}
  for kind in ('fwd', 'bwd'):
    t = lambda name: g[name][f'{kind}_us_median']
    ratios[kind] = {'r64_packed_vs_general': round(t('r64-packed') / t('r64-general'), 2),
                    'r64_packed_vs_default': round(t('r64-packed') / t('r64-default'), 2),
                    'full_unpacked_vs_packed': round(t('full-unpacked') / t('full-packed'), 2),
                    'full_dense_vs_packed': round(t('full-dense') / t('full-packed'), 2)}
  record['time_ratios'] = ratios
  record['tile_ratio_full_unpacked_vs_packed'] = g['full-unpacked']['tiles_per_plane'] / g['full-packed']['tiles_per_plane']
  print(f'B={B} S={S} N={N} D={D} bf16, {n_ex} x {L} packed  (full packed vs dense max |diff| {parity["full_packed_vs_dense"]:.2e})')
  print(f'  {"variant":<14} {"tiles/plane":>11} {"fwd us":>10} {"bwd us":>10}')
  for name, rec in g.items():
    print(f'  {name:<14} {rec["tiles_per_plane"]:>11} {rec["fwd_us_median"]:>10} {rec["bwd_us_median"]:>10}')
  print('  ratios', json.dumps(ratios))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)
  for kind in ('fwd', 'bwd'):
    assert ratios[kind]['full_unpacked_vs_packed'] > 1 and ratios[kind]['full_dense_vs_packed'] > 1, \
        f'{kind}: packing with tile skipping must beat the unpacked kernels and the dense operator'


if __name__ == '__main__':
  main()
