"""Per-batch time of the validation step on one MI355X, eager against replayed, at the BASELINE config-3 shape (BERT-base
dims, S = 4096 = 2 + 63^2 patches + 125 text, radius 64 + 8 global tokens, bf16, per-GPU batch 4, `mlm,itm`; the model
and the fused optimizer of `bench.py`'s train step, so the forward reads the bf16 shadow weights as it does between train
steps):

  eager    : `evaluation.EvalStep` -- `task.validation_step` under no_grad, one launch per kernel
  replayed : `evaluation.GraphedEvalStep` -- the same step recorded once as a HIP graph; a batch is copied into the
             step's input buffers and the graph replayed

A round is `--batches` batches back to back (a new batch each, no host wait between them, as in `evaluation.evaluate`),
timed on the host from before the first to the end of the last (one device synchronisation), divided by the batch count.
The routes alternate round by round in one process after a warm-up of each (which records the graph).  Nothing is
asserted on the times; the two routes' metric sums are asserted equal bit for bit.  Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=25)
  ap.add_argument('--batches', type=int, default=4, help='batches per round')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_timing.json'))
  args = ap.parse_args()

  import torch
  import bench
  from mmt_amd import configs, distribute, evaluation, optimization, tasks
  assert torch.cuda.is_available(), 'eval_timing needs a GPU'
  dev = torch.device('cuda:0')
  cfg = bench.config3()
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {
      'model': {'encoder': {'mmt': {'relative_pos_max_distance': cfg['m'], 'relative_vocab_size': cfg['R']}},
                'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]},
      'train_data': {'max_seq_len': cfg['S'], 'image_size': 16 * cfg['P'], 'patch_size': 16, 'global_batch_size': cfg['B'],
                     'tasks': 'mlm,itm', 'mpp_fraction_to_mask': 0.0, 'relative_pos_max_distance': cfg['m'],
                     'local_radius': cfg['radius'], 'num_global_tokens': cfg['ng']}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = task.build_model().to(dev)
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()), reduce=tasks.gradient_reduce_mode(exp.task))
  optimization.create_optimizer(model, exp.trainer.optimizer_config, reducer=reducer)       # the bf16 shadows the forward reads
  data = task.build_inputs(exp.task.train_data, device=dev, batch_size=cfg['B'])
  batches = [next(data) for _ in range(args.batches)]            # resident before the timed region, distinct tensors
  routes = {'eager': evaluation.EvalStep(task, model), 'replayed': evaluation.GraphedEvalStep(task, model, graph=True)}

  def run(step):
    for b in batches:
      step(b)

  for step in routes.values():                                   # warm-up: two rounds each (the second batch records the graph)
    run(step); run(step)
  torch.cuda.synchronize()
  assert routes['replayed'].graph is not None, 'the validation step was not captured'
  for step in routes.values():
    for m in step.all_metrics():
      m.reset_state()
  times = {name: [] for name in routes}
  for rnd in range(args.rounds):
    for name, step in routes.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      run(step)
      torch.cuda.synchronize()
      times[name].append((time.perf_counter() - t0) * 1e3 / len(batches))
    print(f'  round {rnd}: ' + '  '.join(f'{name} {ts[-1]:.3f} ms' for name, ts in times.items()), flush=True)
  same = all(torch.equal(a.state, b.state) for a, b in zip(routes['eager'].all_metrics(), routes['replayed'].all_metrics())
             if a.state is not None)
  assert same, 'the replayed step did not accumulate the eager step\'s sums'
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'batches_per_round': len(batches),
            'batches_timed_per_route': args.rounds * len(batches),
            'config': dict(name=cfg['name'].format(ng=cfg['ng']), S=cfg['S'], P=cfg['P'], B=cfg['B'], dtype='bf16', tasks='mlm,itm'),
            'sums_equal_bitwise': bool(same), 'ms_per_batch': {}}
  for name, ts in times.items():
    rec = {'median': round(statistics.median(ts), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}
    record['ms_per_batch'][name] = rec
    print(f'  {name:<9} {rec["median"]} ms per batch ({rec["min"]}..{rec["max"]})')
  record['replayed_median_below_eager_median'] = record['ms_per_batch']['replayed']['median'] < record['ms_per_batch']['eager']['median']
  routes['replayed'].close()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
