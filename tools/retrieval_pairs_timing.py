"""Pairs per second of retrieval scoring, every image of a set against every text of a set, on one MI355X: the
`mmt/retrieval` experiment at S = 256, P = 14 (224 / 16), bf16, BERT-base encoder, I = 64 images x T = 512 texts in
batches of 512 pairs.  Routes, whole `score_all`-sized runs timed with device events, alternating in one process after a
warm-up run of each:

  host      : every batch materialised on the host from host-resident sets, copied, and run through `predict.predict`
              (one RawResult per pair) -- the only route before `mmt_amd/retrieval.py`
  device    : every batch materialised on the device with torch gathers (`RetrievalSets.materialize`), the patch
              projection run per batch, scores scattered into the [I, T] matrix
  pairs     : `PairScorer(graph=False)`: the pair kernel gathers from the resident tables, the image table projected once per run
  pairs-graph : `PairScorer(graph=True)`: the same forward captured once and replayed

Nothing is asserted on the times.  Writes one JSON record (--out).

`--forward-only N` runs N eager batches of the `pairs` route and nothing else: the workload for a
`rocprofv3 --kernel-trace --stats` run of its own (the embedding assembly's share of one forward)."""
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
  ap.add_argument('--images', type=int, default=64)
  ap.add_argument('--texts', type=int, default=512)
  ap.add_argument('--batch', type=int, default=512)
  ap.add_argument('--forward-only', type=int, default=0, metavar='N')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'retrieval_pairs_timing.json'))
  args = ap.parse_args()

  import torch
  import mmt_amd
  from mmt_amd import configs, input_utils, predict
  from mmt_amd.retrieval import PairScorer, RetrievalSets, num_shard_pairs, pair_entries, scores_from_logits
  assert torch.cuda.is_available(), 'retrieval_pairs_timing needs a GPU'
  dev = torch.device('cuda:0')
  I, T, bs = args.images, args.texts, args.batch
  exp = configs.get_exp_config('mmt/retrieval')
  exp.override({'task': {'model': {'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]},
                         'train_data': dict(max_seq_len=256, image_size=224, patch_size=16)}}, strict=False)
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = task.build_model().to(dev).eval()
  g = torch.Generator(device=dev).manual_seed(1)
  sets = input_utils.synthetic_retrieval_sets(exp.task.train_data, I, T, dev, g)

  if args.forward_only:
    scorer = PairScorer(task, model, sets, bs, graph=False)
    for k in range(args.forward_only):
      ie, te = pair_entries(I, T, k * bs, bs, device=dev)
      scorer.score_pairs(ie, te)
    torch.cuda.synchronize()
    print(f'{args.forward_only} eager batches of {bs} pairs')
    return

  import dataclasses
  host_sets = RetrievalSets(**{f.name: (getattr(sets, f.name).cpu() if torch.is_tensor(getattr(sets, f.name))
                                        else getattr(sets, f.name)) for f in dataclasses.fields(sets)})
  total = num_shard_pairs(I, T)
  firsts = range(0, total, bs)

  def route_host():
    def batches():
      for first in firsts:
        inputs, labels = host_sets.materialize(*pair_entries(I, T, first, bs))
        yield ({k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in inputs.items()}, labels)
    results = [r for r in predict.predict(task, batches(), model) if r.image_index >= 0]
    m = torch.full((I, T), -1.0)
    for r in results:
      m[r.image_index, r.text_index] = r.output
    return m.to(dev)

  @torch.no_grad()
  def route_device():
    scores = torch.full((I * T + 1,), -1.0, dtype=torch.float32, device=dev)
    for first in firsts:
      ie, te = pair_entries(I, T, first, bs, device=dev)
      inputs, _ = sets.materialize(ie, te)
      for k in ('image_index', 'text_index', 'gt_image_index'):
        inputs.pop(k)
      flat = torch.where(ie >= 0, ie.long() * T + te.long(), torch.full_like(ie, I * T, dtype=torch.int64))
      scores[flat] = scores_from_logits(model(**inputs, training=False)['itm_logits'])
    return scores[:I * T].view(I, T)

  eager, graphed = PairScorer(task, model, sets, bs, graph=False), PairScorer(task, model, sets, bs, graph=True)
  routes = {'host': route_host, 'device': route_device, 'pairs': lambda: eager.score_all()[0],
            'pairs-graph': lambda: graphed.score_all()[0]}
  outs = {name: fn().float().clone() for name, fn in routes.items()}       # warm-up (and the graph's capture)
  torch.cuda.synchronize()
  assert graphed.graph is not None, 'the forward was not captured'
  parity = {f'{name}_vs_device': float((outs[name] - outs['device']).abs().max()) for name in ('host', 'pairs', 'pairs-graph')}
  parity['pairs-graph_equals_pairs'] = bool(torch.equal(outs['pairs-graph'], outs['pairs']))
  del outs
  times = {name: [] for name in routes}
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for rnd in range(args.rounds):
    for name, fn in routes.items():
      e0.record()
      fn()
      e1.record()
      torch.cuda.synchronize()
      times[name].append(total / (e0.elapsed_time(e1) * 1e-3))
    print(f'  round {rnd}: ' + '  '.join(f'{name} {ts[-1]:.0f}' for name, ts in times.items()), flush=True)
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
            'config': dict(experiment='mmt/retrieval', S=256, P=14, dtype='bf16', encoder='BERT-base', images=I, texts=T,
                           batch=bs, pairs=total),
            'max_abs_score_diff': parity, 'pairs_per_second': {}}
  print(f'  {"route":<12} {"pairs/s median (min..max)":>34}')
  for name, ts in times.items():
    rec = {'median': round(statistics.median(ts), 1), 'min': round(min(ts), 1), 'max': round(max(ts), 1)}
    record['pairs_per_second'][name] = rec
    print(f'  {name:<12} {rec["median"]:>12} ({rec["min"]}..{rec["max"]})')
  print('  max |score diff|', json.dumps(parity))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
