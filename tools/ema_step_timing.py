"""Times of the weight averages (`trainer.optimizer_config.ema`, csrc/ema.hip) on the slabs of the BASELINE config-3
model (12 layers, hidden 768: 111 M parameters in 48 MB gradient buckets), in one process:

  launches  on one FusedAdamW with averages: the `mmt_adamw_step` launches alone (the yardstick: 34 bytes per element --
            four fp32 reads, three fp32 writes, the bf16 shadow, the gradient clear), the `mmt_ema_step` launches alone
            (12 bytes per element) and a swap pair (two `mmt_ema_swap` per slab: 2 x 18 bytes per element).  Each timed
            call is between two HIP events; `--rounds` rounds alternate the three, `--calls` calls each; a round's
            figure is the mean of its calls; reported are the median and the range over the rounds.
  step      the whole train step at the config-3 shape, replayed from its HIP graph, with the `ema` block on and off: two
            steps built side by side, rounds alternating, `--step-calls` steps per round between two events.

A record, not a gate: nothing is asserted on the times.  Writes the JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

BYTES_PER_ELEMENT = {'adamw': 34, 'ema': 12, 'swap_pair': 36}


def build(device):
  import torch
  import bench
  from mmt_amd import configs, distribute, optimization, tasks
  cfg = bench.config3()
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {'model': {'encoder': {'mmt': {'relative_pos_max_distance': cfg['m'], 'relative_vocab_size': cfg['R']}},
                                   'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]}},
                'trainer': {'optimizer_config': {'ema': {}}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16, num_replicas=1)
  torch.manual_seed(0)
  model = task.build_model().to(device)
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()))
  opt = optimization.create_optimizer(model, exp.trainer.optimizer_config, reducer=reducer)
  assert type(opt) is optimization.FusedAdamW and opt.ema_enabled, type(opt)
  return model, reducer, opt


def timed(fn, calls, before=None):
  """Mean device time of `calls` calls of `fn`, in microseconds; `before` runs in front of each first event."""
  import torch
  total = 0.0
  for _ in range(calls):
    if before is not None:
      before()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    total += start.elapsed_time(end) * 1e3
  return total / calls


def summary(values, digits=1):
  return {'median': round(statistics.median(values), digits), 'min': round(min(values), digits), 'max': round(max(values), digits)}


def launches_leg(device, rounds, calls, warmup):
  import torch
  from mmt_amd import optimization
  model, reducer, opt = build(device)
  scale = torch.full((), 0.5, dtype=torch.float32, device=device)
  L = opt._lib.lib()

  def refill():
    for b in reducer.buckets:
      b.normal_(std=0.01)

  def adamw_alone():                       # FusedAdamW.step without its averages: the parent's launches on these slabs
    opt.ema_enabled = False
    try:
      opt.step(grad_scale=scale)
    finally:
      opt.ema_enabled = True

  def ema_alone():
    d = opt._lib.EmaDesc()
    d.one_minus_decay = optimization.ema_one_minus_decay(opt.cfg, 1000)
    for slab in opt.slabs:
      opt._queue_ema(L, d, slab, slab['param'].device)

  def swap_pair():
    opt.swap_weights()
    opt.swap_weights()

  legs = {'adamw': (adamw_alone, refill), 'ema': (ema_alone, None), 'swap_pair': (swap_pair, None)}
  for fn, before in legs.values():
    timed(fn, warmup, before)
  out = {name: [] for name in legs}
  for _ in range(rounds):
    for name, (fn, before) in legs.items():
      out[name].append(timed(fn, calls, before))
  flat = torch.cat([s['param'] for s in opt.slabs] + [s['avg'] for s in opt.slabs])
  assert bool(torch.isfinite(flat).all())
  elements = sum(s['param'].numel() for s in opt.slabs)
  rec = {'slabs': len(opt.slabs), 'elements': elements}
  for name, values in out.items():
    s = summary(values)
    rec[name] = {'us': s, 'bytes_per_element': BYTES_PER_ELEMENT[name],
                 'moved_TB_per_s': round(elements * BYTES_PER_ELEMENT[name] / s['median'] / 1e6, 2)}
  rec['ema_over_adamw'] = round(rec['ema']['us']['median'] / rec['adamw']['us']['median'], 3)
  rec['bytes_ratio'] = round(12 / 34, 3)
  rec['budget_ratio'] = round(12 / 34 * 1.25, 3)
  return rec


def step_leg(device, rounds, calls, warmup):
  import torch
  import bench
  from mmt_amd import benchmarks
  steps = {}
  for name, ema in (('ema_off', None), ('ema_on', {})):
    cfg = dict(bench.config3(), ema=ema)
    steps[name] = benchmarks.make_train_step_bench(cfg, device, 0, 1, dtype=torch.bfloat16, graph=True)[0]
  assert steps['ema_on'].optimizer.ema_enabled and not steps['ema_off'].optimizer.ema_enabled

  def run(step, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
      out = step()
    end.record()
    end.synchronize()
    assert bool(torch.isfinite(out['loss']))
    return start.elapsed_time(end) / n

  for step in steps.values():
    run(step, warmup)
  out = {name: [] for name in steps}
  for _ in range(rounds):
    for name, step in steps.items():
      out[name].append(run(step, calls))
  rec = {name: {'step_ms': summary(values, 3)} for name, values in out.items()}
  rec['ema_on_minus_off_ms'] = round(rec['ema_on']['step_ms']['median'] - rec['ema_off']['step_ms']['median'], 3)
  for step in steps.values():
    step.close()
  return rec


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--calls', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--step-calls', type=int, default=20)
  ap.add_argument('--skip-step', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema_step_timing.json'))
  args = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('ema_step_timing needs a GPU: nothing is measured without one')
  device = torch.device('cuda', 0)
  rec = {'model': 'BASELINE config 3 (MmtPretrainingModel, 12 layers, hidden 768), mlm+itm heads',
         'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls, 'warmup_calls': args.warmup,
         'timer': 'HIP events; launches: around one call, gradient slabs refilled in front of the first event; step: around step_calls replays',
         'launches': launches_leg(device, args.rounds, args.calls, args.warmup)}
  if not args.skip_step:
    rec['step_calls_per_round'] = args.step_calls
    rec['train_step'] = step_leg(device, args.rounds, args.step_calls, args.warmup)
  print(json.dumps(rec))
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(rec, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
