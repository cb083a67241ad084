"""Attention forward / backward call times at head size 128 against head size 64 at the same hidden size (768), at the
config-3 and config-5 shapes of bench.get_config (B as the benchmark uses it, bf16, radius 64, 8 global tokens, 1-D ids,
R = 32).  Routes, timed alternately in one process (HIP events, warm-up, rounds of calls):

  d128          : D = 128, N = 6 -- the general structured kernels (the only route head size 128 takes)
  d64-default   : D = 64, N = 12 on today's default kernels (lean bf16 / window)
  d64-general   : D = 64, N = 12 on the general structured kernels, reached as tools/grid_attn_timing.py does: with a
                  grid term that adds no pair (a = 1 over a one-patch image at position 0, which the band covers)
  d128-dense    : D = 128, N = 6 through the dense operator on the [B,S,S] mask + ids from mmt_side_inputs

Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

HIDDEN = 768


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--configs', default='3,5')
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=10, help='calls per round (>= 50 per point over the rounds)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'head128_timing.json'))
  ap.add_argument('--no-dense', action='store_true', help='skip the dense-operator route')
  args = ap.parse_args()

  import torch
  import bench
  import mmt_amd
  assert torch.cuda.is_available(), 'head128_timing needs a GPU'
  dev = 'cuda:0'
  dt = torch.bfloat16
  record = {'device': torch.cuda.get_device_name(0), 'hidden_size': HIDDEN, 'rounds': args.rounds,
            'calls_per_round': args.calls, 'shapes': []}
  for n in (int(c) for c in args.configs.split(',')):
    cfg = bench.get_config(n)
    B, S, R, W, m, g0, ng = cfg['B'], cfg['S'], cfg['R'], cfg['radius'], cfg['m'], cfg['g0'], cfg['ng']
    base = dict(local_radius=W, global_start=g0, n_global=ng, id_mode=1, max_dist=m)
    pat = mmt_amd.AttentionPattern(**base)
    pat_general = mmt_amd.AttentionPattern(**base, patches_per_row=1, grid_radius=1, grid_start=0)
    torch.manual_seed(0)
    tensors = {}
    for D in (64, 128):
      N = HIDDEN // D
      q, k, v, dout = (torch.randn(B, S, N, D, device=dev, dtype=dt) for _ in range(4))
      emb = (torch.randn(R, N, D, device=dev) * 0.5).to(dt)
      bias = (torch.randn(R, N, device=dev) * 0.5).to(dt)
      tensors[D] = (q, k, v, emb, bias, dout)

    def route(D, **kw):
      q, k, v, emb, bias, dout = tensors[D]
      out, lse = mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw)
      return (lambda: mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw),
              lambda: mmt_amd.relative_attention_backward(dout, q, k, v, emb, bias, out, lse, **kw))

    calls = {'d128': route(128, pattern=pat), 'd64-default': route(64, pattern=pat),
             'd64-general': route(64, pattern=pat_general)}
    if not args.no_dense:
      valid = torch.full((B,), S, dtype=torch.int32, device=dev)
      si = mmt_amd.side_inputs(pat, valid, torch.zeros_like(valid), S, materialize_pattern=True, want_segment_ids=False)
      calls['d128-dense'] = route(128, att_mask=si['att_mask'], relative_att_ids=si['relative_att_ids'])
    err_dense = None
    if 'd128-dense' in calls:
      err_dense = float((calls['d128-dense'][0]()[0].float() - calls['d128'][0]()[0].float()).abs().max())
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
    shape = {'config': n, 'B': B, 'S': S, 'radius': W, 'n_global': ng, 'R': R, 'dtype': 'bf16',
             'max_abs_diff_d128_dense_vs_structured': err_dense, 'routes': {}}
    for name in calls:
      rec = {'D': 128 if name.startswith('d128') else 64, 'N': HIDDEN // (128 if name.startswith('d128') else 64)}
      for kind in ('fwd', 'bwd'):
        ts = times[name][kind]
        rec[f'{kind}_us_median'] = round(statistics.median(ts), 1)
        rec[f'{kind}_us_min'] = round(min(ts), 1)
        rec[f'{kind}_us_max'] = round(max(ts), 1)
      shape['routes'][name] = rec
    r_ = shape['routes']
    for name in calls:
      r_[name]['fwd_vs_d64_general'] = round(r_[name]['fwd_us_median'] / r_['d64-general']['fwd_us_median'], 2)
      r_[name]['bwd_vs_d64_general'] = round(r_[name]['bwd_us_median'] / r_['d64-general']['bwd_us_median'], 2)
    record['shapes'].append(shape)
    print(f'config {n}: B={B} S={S} radius={W} ng={ng} hidden={HIDDEN}'
          + ('' if err_dense is None else f'  (d128 dense vs structured max |diff| {err_dense:.2e})'))
    print(f'  {"route":<12} {"fwd us":>9} {"bwd us":>9}  fwd / bwd vs d64-general')
    for name, rec in r_.items():
      print(f'  {name:<12} {rec["fwd_us_median"]:>9} {rec["bwd_us_median"]:>9}  '
            f'{rec["fwd_vs_d64_general"]} / {rec["bwd_vs_d64_general"]}')
    del calls, tensors
    if not args.no_dense:
      del si
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
