"""Times of the two flat optimizer steps on the slabs of the BASELINE config-3 model (12 layers, hidden 768: 111 M
parameters in 48 MB gradient buckets): `FusedLamb.step` (csrc/lamb.hip, three launches per slab) and `FusedAdamW.step`
(one launch per slab), back to back in one process on two identically built models.

Every timed call is one `step(grad_scale=...)` between two HIP events; the gradient slabs are refilled with noise in
front of the first event (a step clears them, and LAMB uses them for its update direction).  Warm-up calls first, then
`--rounds` rounds that alternate the two optimizers, `--calls` calls each; a round's figure is the mean of its calls,
reported are the median and the range over the rounds, the ratio of the medians, and the rate at which the bytes the
step has to move (AdamW 34 B per element, LAMB 46 B: 28 in the moments pass, 18 in the apply pass) were moved.

A record, not a gate: nothing is asserted on the times.  Writes the JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

BYTES_PER_ELEMENT = {'adamw': 34, 'lamb': 46}


def build(optimizer_type, device):
  import torch
  import bench
  from mmt_amd import configs, distribute, optimization, tasks
  cfg = bench.config3()
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {'model': {'encoder': {'mmt': {'relative_pos_max_distance': cfg['m'], 'relative_vocab_size': cfg['R']}},
                                   'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]}},
                'trainer': {'optimizer_config': {'optimizer_type': optimizer_type}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16, num_replicas=1)
  torch.manual_seed(0)
  model = task.build_model().to(device)
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()))
  opt = optimization.create_optimizer(model, exp.trainer.optimizer_config, reducer=reducer)
  want = optimization.FusedLamb if optimizer_type == 'lamb' else optimization.FusedAdamW
  assert type(opt) is want, type(opt)
  return model, reducer, opt


def timed_calls(opt, reducer, scale, calls):
  """Mean device time of `calls` steps, in microseconds."""
  import torch
  total = 0.0
  for _ in range(calls):
    for b in reducer.buckets:
      b.normal_(std=0.01)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    opt.step(grad_scale=scale)
    end.record()
    end.synchronize()
    total += start.elapsed_time(end) * 1e3
  return total / calls


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lamb_step_timing.json'))
  args = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('lamb_step_timing needs a GPU: nothing is measured without one')
  device = torch.device('cuda', 0)
  built = {name: build(name, device) for name in ('adamw', 'lamb')}
  scale = torch.full((), 0.5, dtype=torch.float32, device=device)
  elements = {name: sum(s['grad'].numel() for s in b[2].slabs) for name, b in built.items()}
  rounds = {name: [] for name in built}
  for name, (_, reducer, opt) in built.items():
    timed_calls(opt, reducer, scale, args.warmup)
  for _ in range(args.rounds):
    for name, (_, reducer, opt) in built.items():
      rounds[name].append(timed_calls(opt, reducer, scale, args.calls))
  for name, (model, _, opt) in built.items():        # the steps did run: finite parameters that moved
    flat = torch.cat([s['param'] for s in opt.slabs])
    assert bool(torch.isfinite(flat).all()) and opt.t == args.warmup + args.rounds * args.calls, name
  rec = {'model': 'BASELINE config 3 (MmtPretrainingModel, 12 layers, hidden 768), mlm+itm heads',
         'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls, 'warmup_calls': args.warmup,
         'timer': 'HIP events around one step() call; gradient slabs refilled in front of the first event'}
  for name in built:
    opt = built[name][2]
    med = statistics.median(rounds[name])
    rec[name] = {'slabs': len(opt.slabs), 'elements': elements[name],
                 'segments': sum(s.get('n_segments', 0) for s in opt.slabs) or None,
                 'launches_per_step': len(opt.slabs) * (3 if name == 'lamb' else 1),
                 'step_us_median': round(med, 1), 'step_us_min': round(min(rounds[name]), 1), 'step_us_max': round(max(rounds[name]), 1),
                 'bytes_per_element': BYTES_PER_ELEMENT[name],
                 'moved_TB_per_s': round(elements[name] * BYTES_PER_ELEMENT[name] / med / 1e6, 2)}
  rec['lamb_over_adamw'] = round(rec['lamb']['step_us_median'] / rec['adamw']['step_us_median'], 3)
  rec['bytes_ratio'] = round(BYTES_PER_ELEMENT['lamb'] / BYTES_PER_ELEMENT['adamw'], 3)
  print(json.dumps(rec))
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
