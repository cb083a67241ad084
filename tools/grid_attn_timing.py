"""Attention forward / backward call times with the image-grid term (SURVEY.md App. A.5 `grid_radius`) at the
config-3 and config-5 shapes of bench.get_config (B and N as the benchmark uses them, bf16, radius 64, 8 global tokens,
1-D ids, R = 32).  Variants, timed alternately in one process (HIP events, warm-up, rounds of calls):

  a0-default : a = 0, today's default kernels (lean bf16 / window)
  a0-general : a = 0 on the route the grid calls take -- the general structured kernels' grid instantiations, reached
               with a grid that adds no pair (a = 1 over a one-patch image at position 0, which the band covers)
  a1, a2     : the grid of the data layout (g = 2, P = image_size // patch_size)
  a1-dense   : a = 1 through the dense operator on the [B,S,S] mask + ids from mmt_side_inputs (today's only route)

It also prints the key tiles each call visits (forward; the backward's dQ and dK/dV passes visit as many), counted on
the host from the walk definition (band U global tiles U one interval per image-row offset; the global rows' split
items over every tile), next to the dense operator's.  Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))


def visited_tiles(S, radius, g0, ng, a, P, g=2):
  """Key tiles one (b, n) plane's forward visits: the 32-row blocks' walks (GridWalk in csrc/attn_tile.h) plus the
  split items of the global rows (every tile once per 32 global rows)."""
  n_tiles = (S + 31) // 32
  total = 0
  for x0 in range(0, S, 32):
    tiles = set(range(max(x0 - radius, 0) // 32, min(x0 + 31 + radius, S - 1) // 32 + 1))
    if ng:
      tiles.update(range(g0 // 32, (g0 + ng - 1) // 32 + 1))
    ia, ib = max(x0, g), min(x0 + 31, g + P * P - 1)
    if a > 0 and ia <= ib:
      for dr in range(-a, a + 1):
        lo, hi = max(ia + dr * P - a, g), min(ib + dr * P + a, g + P * P - 1)
        if lo <= hi:
          tiles.update(range(lo // 32, hi // 32 + 1))
    total += len(tiles)
  if ng and radius < S:
    total += (ng + 31) // 32 * n_tiles
  return total


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--configs', default='3,5')
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=10, help='calls per round (>= 50 per point over the rounds)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grid_attn_timing.json'))
  ap.add_argument('--no-dense', action='store_true', help='skip the dense-operator variant')
  args = ap.parse_args()

  import torch
  import bench
  import mmt_amd
  assert torch.cuda.is_available(), 'grid_attn_timing needs a GPU'
  dev = 'cuda:0'
  dt = torch.bfloat16
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls, 'shapes': []}
  for n in (int(c) for c in args.configs.split(',')):
    cfg = bench.get_config(n)
    B, S, N, R, P, W, m, g0, ng = cfg['B'], cfg['S'], cfg['N'], cfg['R'], cfg['P'], cfg['radius'], cfg['m'], cfg['g0'], cfg['ng']
    torch.manual_seed(0)
    q, k, v = (torch.randn(B, S, N, 64, device=dev, dtype=dt) for _ in range(3))
    emb = (torch.randn(R, N, 64, device=dev) * 0.5).to(dt)
    bias = (torch.randn(R, N, device=dev) * 0.5).to(dt)
    dout = torch.randn(B, S, N, 64, device=dev, dtype=dt)
    base = dict(local_radius=W, global_start=g0, n_global=ng, id_mode=1, max_dist=m)
    pats = {
        'a0-default': mmt_amd.AttentionPattern(**base),
        'a0-general': mmt_amd.AttentionPattern(**base, patches_per_row=1, grid_radius=1, grid_start=0),
        'a1': mmt_amd.AttentionPattern(**base, patches_per_row=P, grid_radius=1, grid_start=2),
        'a2': mmt_amd.AttentionPattern(**base, patches_per_row=P, grid_radius=2, grid_start=2),
    }
    calls = {}
    for name, pat in pats.items():
      out, lse = mmt_amd.relative_attention_forward(q, k, v, emb, bias, pattern=pat)
      calls[name] = (lambda pat=pat: mmt_amd.relative_attention_forward(q, k, v, emb, bias, pattern=pat),
                     lambda pat=pat, out=out, lse=lse: mmt_amd.relative_attention_backward(
                         dout, q, k, v, emb, bias, out, lse, pattern=pat))
    if not args.no_dense:
      valid = torch.full((B,), S, dtype=torch.int32, device=dev)
      si = mmt_amd.side_inputs(pats['a1'], valid, torch.zeros_like(valid), S, materialize_pattern=True,
                               want_segment_ids=False)
      dk = dict(att_mask=si['att_mask'], relative_att_ids=si['relative_att_ids'])
      out, lse = mmt_amd.relative_attention_forward(q, k, v, emb, bias, **dk)
      calls['a1-dense'] = (lambda: mmt_amd.relative_attention_forward(q, k, v, emb, bias, **dk),
                           lambda out=out, lse=lse: mmt_amd.relative_attention_backward(dout, q, k, v, emb, bias, out, lse, **dk))
    # parity of the a0 routes (same pattern, two kernel families) and of the dense route against a1
    ref0 = calls['a0-default'][0]()[0].float()
    err_general = float((calls['a0-general'][0]()[0].float() - ref0).abs().max())
    err_dense = float((calls['a1-dense'][0]()[0].float() - calls['a1'][0]()[0].float()).abs().max()) if 'a1-dense' in calls else None
    times = {name: {'fwd': [], 'bwd': []} for name in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, (f, b) in calls.items():           # warm-up
      for _ in range(3):
        f(); b()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
      for name, (f, b) in calls.items():
        for kind, fn in (('fwd', f), ('bwd', b)):
          e0.record()
          for _ in range(args.calls):
            fn()
          e1.record()
          torch.cuda.synchronize()
          times[name][kind].append(e0.elapsed_time(e1) / args.calls * 1e3)
    tiles = {'a0-default': visited_tiles(S, W, g0, ng, 0, P), 'a0-general': visited_tiles(S, W, g0, ng, 0, P),
             'a1': visited_tiles(S, W, g0, ng, 1, P), 'a2': visited_tiles(S, W, g0, ng, 2, P),
             'a1-dense': ((S + 31) // 32) ** 2}
    shape = {'config': n, 'B': B, 'S': S, 'N': N, 'P': P, 'radius': W, 'n_global': ng, 'R': R, 'dtype': 'bf16',
             'max_abs_diff_a0_general_vs_default': err_general, 'max_abs_diff_a1_dense_vs_structured': err_dense,
             'variants': {}}
    for name in calls:
      rec = {'tiles_per_plane': tiles[name], 'tiles_per_call': tiles[name] * B * N}
      for kind in ('fwd', 'bwd'):
        ts = times[name][kind]
        rec[f'{kind}_us_median'] = round(statistics.median(ts), 1)
        rec[f'{kind}_us_min'] = round(min(ts), 1)
        rec[f'{kind}_us_max'] = round(max(ts), 1)
      shape['variants'][name] = rec
    g = shape['variants']
    for name in calls:
      g[name]['fwd_vs_a0_general'] = round(g[name]['fwd_us_median'] / g['a0-general']['fwd_us_median'], 2)
      g[name]['bwd_vs_a0_general'] = round(g[name]['bwd_us_median'] / g['a0-general']['bwd_us_median'], 2)
      g[name]['tiles_vs_a0_general'] = round(tiles[name] / tiles['a0-general'], 2)
    record['shapes'].append(shape)
    print(f'config {n}: B={B} S={S} N={N} P={P} radius={W} ng={ng}  (a0 general vs default max |diff| {err_general:.2e}'
          + ('' if err_dense is None else f', a1 dense vs structured {err_dense:.2e}') + ')')
    print(f'  {"variant":<11} {"tiles/plane":>11} {"fwd us":>9} {"bwd us":>9}  fwd/bwd/tiles vs a0-general')
    for name, rec in g.items():
      print(f'  {name:<11} {rec["tiles_per_plane"]:>11} {rec["fwd_us_median"]:>9} {rec["bwd_us_median"]:>9}  '
            f'{rec["fwd_vs_a0_general"]} / {rec["bwd_vs_a0_general"]} / {rec["tiles_vs_a0_general"]}')
    del calls, q, k, v, dout
    if not args.no_dense:
      del si, dk
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
