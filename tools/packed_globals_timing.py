"""Attention forward / backward call times of packed multimodal examples with PER-EXAMPLE GLOBAL TOKENS (`example_starts=`
with a global range, MMT_FLAG_EXAMPLE_GLOBALS) at B=4, S=4096, N=12, D=64, bf16, radius 64, 8 global tokens at
2 + 14^2 = 198 of every example, 1-D ids (R = 32, m = 12).  Three packings of the row:

  a : 16 examples of 256 tokens
  b : 2 examples of 2048 tokens
  c : one example that fills the row -- the long-walk case: a block with a global row walks all 128 tiles in one wave

and for each, timed alternately in one process (HIP events, warm-up, rounds of calls):

  globals : ids + starts + the global range on the structured kernels (the GLB instantiations)
  origin  : the same call with n_global = 0 (the ORG instantiations): what the global term costs
  dense   : the dense operator on the composed mask and ids -- the only route of `globals` before

Nothing is asserted on the times.  Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

PACKINGS = {'a': 256, 'b': 2048, 'c': 4096}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=5, help='calls per round of the structured routes (the dense ones: 1)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'packed_globals_timing.json'))
  args = ap.parse_args()

  import dataclasses
  import torch
  import mmt_amd
  from mmt_amd import ops
  assert torch.cuda.is_available(), 'packed_globals_timing needs a GPU'
  dev, dt = 'cuda:0', torch.bfloat16
  B, S, N, D, R, m = 4, 4096, 12, 64, 32, 12
  torch.manual_seed(0)
  q, k, v, dout = (torch.randn(B, S, N, D, device=dev, dtype=dt) for _ in range(4))
  emb = (torch.randn(R, N, D, device=dev) * 0.5).to(dt)
  bias = (torch.randn(R, N, device=dev) * 0.5).to(dt)
  pat = mmt_amd.AttentionPattern(local_radius=64, global_start=2 + 14 * 14, n_global=8, id_mode=1, max_dist=m)
  pat0 = dataclasses.replace(pat, global_start=0, n_global=0)

  variants = {}
  for tag, L in PACKINGS.items():
    rows = [[L] * (S // L)] * B
    ids, starts, _, _ = mmt_amd.packed_example_layout(rows, [[True] * len(r) for r in rows], S, device=dev)
    structured = dict(pattern=pat, example_ids=ids, example_starts=starts)
    assert ops._resolve_pattern(pat, None, None, None, q, ids, starts)[0] is pat, 'the globals call left the structured route'
    variants[f'{tag}-globals'] = structured
    variants[f'{tag}-origin'] = dict(pattern=pat0, example_ids=ids, example_starts=starts)
    mask, rel = ops._materialized(pat, None, B, S, torch.device(dev), ids, starts)
    variants[f'{tag}-dense'] = dict(att_mask=mask, relative_att_ids=rel)

  calls, outs = {}, {}
  for name, kw in variants.items():
    out, lse = mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw)
    outs[name] = out.float()
    calls[name] = (lambda kw=kw: mmt_amd.relative_attention_forward(q, k, v, emb, bias, **kw),
                   lambda kw=kw, out=out, lse=lse: mmt_amd.relative_attention_backward(dout, q, k, v, emb, bias, out, lse, **kw))
  parity = {f'{tag}_globals_vs_dense': float((outs[f'{tag}-globals'] - outs[f'{tag}-dense']).abs().max()) for tag in PACKINGS}
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
            'shape': dict(B=B, S=S, N=N, D=D, R=R, dtype='bf16', radius=64, global_start=198, n_global=8),
            'packings': {tag: f'{S // L} x {L}' for tag, L in PACKINGS.items()}, 'max_abs_diff': parity, 'variants': {}}
  for name in variants:
    rec = {}
    for kind in ('fwd', 'bwd'):
      ts = times[name][kind]
      rec.update({f'{kind}_us_median': round(statistics.median(ts), 1), f'{kind}_us_min': round(min(ts), 1),
                  f'{kind}_us_max': round(max(ts), 1)})
    record['variants'][name] = rec
  g = record['variants']
  record['time_ratios'] = {
      kind: {f'{tag}_{a}_vs_{b}': round(g[f'{tag}-{a}'][f'{kind}_us_median'] / g[f'{tag}-{b}'][f'{kind}_us_median'], 2)
             for tag in PACKINGS for a, b in (('dense', 'globals'), ('globals', 'origin'))}
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
