"""Step time of packed batches against unpacked ones on the same examples (mmt_amd/input_utils.py `pack_batch`,
csrc/pack_rows.hip; DESIGN.md section 4, "Packed batches", and section 5).  A record, not a gate: nothing is asserted
on the times, and `pack_rows` stays off by default whatever they say.

Workload: the pretraining step (mlm + mpp + itm, AdamW on the flat slabs, bf16) at the dimensions of BASELINE config 3
(12 layers, hidden 768, 12 heads, intermediate 3072, radius 64 + 8 global tokens, 1-D ids, dropout 0.1) on examples
`[CLS][PATCH]` + 196 patches (image 224, patch 16) + `[ATT]` caption `[SEP]`.  A pool of --examples examples is drawn
once; the same pool is served
  unpacked   [--batch, 512] rows, one example per row, valid_len skips the padding in the attention kernels only
  packed     rows of 2048 and of 4096 positions holding the same number of positions per step as the unpacked batch
             (--batch * 512 / row length rows), next-fit in arrival order until the pool is empty
Caption lengths (wordpieces behind the image, field token and [SEP] included):
  fixture    the captions of the test shards (tests/_record_cases.py `loader_records` over the corpus of
             tests/_text_cases.py, tokenised with the tests' vocabulary by the CPU route of `text_frontend`), cycled
  lognormal  round(exp(N(ln 16, 0.6^2))) clipped to [4, 310], seed 7 -- a named stand-in for alt-text-like captions

Method (the measuring guide): every mode's batches are resident before the timed region; three warm-up passes over every
mode; then --rounds rounds in which the modes ALTERNATE, each pass over a mode's batches bracketed by device events;
median and range over the rounds.  Steps are eager `task.train_step` calls with a new batch every step, or with --graph
one `GraphedTrainStep` per mode (its own model and optimizer, recorded after one eager step).  Reported per mode: steps,
examples, positions per step, the padding share (1 - example positions / positions processed), milliseconds per step
and microseconds per example.  Beside them the cost of the packing call itself: its device time by events, and the
host's wait for the one `consumed` word with nothing else queued -- the floor of what the loader's stage waits per
batch (`RecordStages.pack_wait_seconds` is the wait in a real pass; stage times of the loaders:
tools/record_loader_timing.py, same JSON layout of {median, min, max}).

Readings (one MI355X, 512 examples, unpacked batch 32, 7 rounds; us per example, eager / graph replay; padding share):
  fixture    unpacked 491.3 / 490.9 (0.524)   rows of 2048: 416.3 / 450.8 (0.048)   rows of 4096: 417.1 / 449.8 (0.048)
  lognormal  unpacked 489.5 / 489.6 (0.580)   rows of 2048: 449.5 / 487.1 (0.159)   rows of 4096: 389.8 / 419.8 (0.039)
  a packed step of the same 16384 positions takes 26.6-28.8 ms eager (28.8-31.2 ms replayed) against 15.7 ms unpacked:
  it holds twice the live positions.  The packing call: medians 0.10-0.12 ms on the device (0.23 in one cell), 0.017-0.025 ms of host wait for
  `consumed` with nothing else queued.  --loader (the pretraining loader on records, batch 32): next(loader) 5.66 ms
  for 32 examples unpacked, 10.72 ms for 64 examples with 8 rows of 2048, of which 0.213 ms wait for `consumed`
  (profiles/pack_loader_timing.json).  Discussion: DESIGN.md section 5, "Packed batches: readings".  Writes one JSON record (--out, default profiles/pack_timing.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

S, IMAGE, PATCH = 512, 224, 16
N_IMG = 2 + (IMAGE // PATCH) ** 2
MAX_TEXT = S - N_IMG
ROW_LENS = (2048, 4096)


def fixture_lengths(n):
  from tests import _record_cases as R
  from mmt_amd import text_frontend
  recs = R.loader_records(24)
  with tempfile.TemporaryDirectory() as d:
    vocab = text_frontend.WordpieceVocab(R.write_vocab(os.path.join(d, 'vocab.txt')))
    out = text_frontend.texts_to_token_features(vocab, [[r['caption'] for r in recs], [r['alt_text'] for r in recs]],
                                                list(R.FIELD_DICT.values()), S, N_IMG - 2)
  counts = [int(c) for c in out['num_text_wordpieces']]
  return [counts[i % len(counts)] for i in range(n)]


def lognormal_lengths(n):
  import numpy as np
  x = np.exp(np.random.default_rng(7).normal(np.log(16.0), 0.6, n))
  return [int(v) for v in np.clip(np.rint(x), 4, 310)]


def summary(values):
  return {'median': round(statistics.median(values), 3), 'min': round(min(values), 3), 'max': round(max(values), 3)}


def build(graph, B):
  """(experiment, step function (batch, step index) -> loss dict, close); the unpacked batch of B rows is one micro step."""
  import torch
  import bench
  from mmt_amd import configs, distribute, graphed, optimization, tasks
  c = bench.config3()
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {'micro_batch_size': B,
                         'model': {'encoder': {'mmt': {'relative_pos_max_distance': c['m'], 'relative_vocab_size': c['R']}},
                                   'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]},
                         'train_data': {'max_seq_len': S, 'image_size': IMAGE, 'patch_size': PATCH, 'tasks': 'mlm,mpp,itm',
                                        'relative_pos_max_distance': c['m'], 'local_radius': c['radius'], 'num_global_tokens': c['ng'],
                                        'mlm_max_selections_per_seq': 48, 'mpp_max_selections_per_seq': 98}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt_cfg = exp.trainer.optimizer_config
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()), reduce=tasks.gradient_reduce_mode(exp.task))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  if graph:
    g = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, clip_norm=opt_cfg.gradient_clip_norm, eager_steps=1)
    return exp, g, g.close

  def step(batch, i):
    optimization.set_learning_rate(optimizer, optimization.learning_rate_at(opt_cfg, i - 1))
    return task.train_step(batch, model, optimizer, reducer=reducer, clip_norm=opt_cfg.gradient_clip_norm, step=i)
  return exp, step, lambda: None


def mode_batches(data_cfg, pool, B):
  """({mode: (batches, positions per step)}, examples, example positions, {mode: cost of its packing calls}) over one pool."""
  import torch
  from mmt_amd import input_utils
  inputs, labels = pool
  N = inputs['word_ids'].shape[0]
  live = int(inputs['valid_len'].sum())
  is_t = torch.is_tensor
  modes = {'unpacked_512': ([({k: (v[i:i + B].contiguous() if is_t(v) else v) for k, v in inputs.items()},
                              {k: v[i:i + B].contiguous() for k, v in labels.items()}) for i in range(0, N - B + 1, B)], B * S)}
  pack_cost = {}
  for L in ROW_LENS:
    rows = B * S // L
    M = input_utils.pack_max_examples(data_cfg, rows, L)          # the packed batch's own size: rows times the examples a row can hold
    batches, at, device_ms, wait_ms = [], 0, [], []
    while at < N:
      head_in = {k: (v[at:at + M] if is_t(v) else v) for k, v in inputs.items()}
      head_lab = {k: v[at:at + M] for k, v in labels.items()}
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      pin, plab, consumed = input_utils.pack_batch(head_in, head_lab, rows, L, M)
      e1.record()
      t0 = time.perf_counter()
      taken = int(consumed)
      wait_ms.append((time.perf_counter() - t0) * 1e3)
      torch.cuda.synchronize()
      device_ms.append(e0.elapsed_time(e1))
      batches.append((pin, plab))
      at += taken
    modes[f'packed_{L}'] = (batches, rows * L)
    pack_cost[f'packed_{L}'] = {'max_examples': M, 'rows': rows, 'pack_batch_device_ms': summary(device_ms[1:] or device_ms),
                                'consumed_readback_wait_ms': summary(wait_ms[1:] or wait_ms)}
  return modes, N, live, pack_cost


def loader_leg(rounds):
  """The pretraining loader on records (24 records over 2 shards written here from the committed JPEG fixtures and the
  test corpus, training mode so the pass repeats; batch 32, max_seq_len 512, image 224, tasks mlm) without and with the
  packing stage (8 rows of 2048): a whole `next(loader)` ending in a device synchronise, in record_loader_timing.py's
  `loader_next_ms` layout, and the stage's own wait for `consumed` per packed batch."""
  import torch
  from tests import _record_cases as R
  from mmt_amd import configs, pretrain_dataloader as pd
  out = {}
  with tempfile.TemporaryDirectory() as d:
    vocab = R.write_vocab(os.path.join(d, 'vocab.txt'))
    R.write_shards(d, R.loader_records(24), 2)
    for name, extra in (('unpacked', {}), ('packed_2048', dict(pack_rows=8, pack_row_len=2048))):
      cfg = configs.MmtPretrainDataConfig(input_path=os.path.join(d, '*.tfrecord'), vocab_filename=vocab, is_training=True,
                                          global_batch_size=32, image_size=IMAGE, patch_size=PATCH, max_seq_len=S, tasks='mlm',
                                          text_special_token_field_dict=json.dumps(R.FIELD_DICT), mlm_max_selections_per_seq=MAX_TEXT,
                                          seed=3, **extra)
      loader = pd.MmtPretrainDataLoader(cfg, device='cuda', shuffle_buffer=8)
      it = loader.load()
      for _ in range(3):
        next(it)
      torch.cuda.synchronize()
      waited, packed_before = loader.pack_wait_seconds, loader.pack_batches
      ts, examples = [], 0
      for _ in range(max(rounds, 5)):
        t0 = time.perf_counter()
        inputs, _ = next(it)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        examples += int(inputs['example_ids'].max(1).values.sum()) if 'example_ids' in inputs else inputs['word_ids'].shape[0]
      out[name] = {'loader_next_ms': summary(ts), 'examples_per_batch': round(examples / len(ts), 1),
                   'loader_ms_per_example': round(sum(ts) / examples, 3)}
      if loader.pack_batches > packed_before:
        out[name]['pack_consumed_wait_ms_per_batch'] = round((loader.pack_wait_seconds - waited) * 1e3 / (loader.pack_batches - packed_before), 3)
  print('loader', json.dumps(out, indent=1), flush=True)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--examples', type=int, default=512)
  ap.add_argument('--batch', type=int, default=32)
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--graph', action='store_true')
  ap.add_argument('--loader', action='store_true', help='only the loader leg: next(loader) without and with the packing stage')
  ap.add_argument('--lengths', default='fixture,lognormal')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pack_timing.json'))
  a = ap.parse_args()
  import torch
  from mmt_amd import input_utils
  if not torch.cuda.is_available():
    raise SystemExit('pack_timing needs a GPU: a time taken elsewhere says nothing')
  record = {'workload': 'pretraining step mlm+mpp+itm, BERT-base dims, bf16, dropout 0.1, radius 64 + 8 global tokens, image 224 / patch 16',
            'examples': a.examples, 'unpacked_batch': a.batch, 'rounds': a.rounds,
            'step_launch': 'HIP graph replay, one GraphedTrainStep per mode' if a.graph else 'eager', 'distributions': {}}
  if a.loader:
    record = {'loader': loader_leg(a.rounds)}
    a.lengths = ''
  for dist in filter(None, a.lengths.split(',')):
    n_text = fixture_lengths(a.examples) if dist == 'fixture' else lognormal_lengths(a.examples)
    steps = {}
    exp, first_step, first_close = build(a.graph, a.batch)
    data_cfg = exp.task.train_data
    g = torch.Generator(device='cuda').manual_seed(3)
    pool = input_utils.synthetic_batch(data_cfg, a.examples, 'cuda', g, vocab_size=exp.task.model.encoder.get().vocab_size,
                                       text_lengths=n_text)
    modes, N, live, pack_cost = mode_batches(data_cfg, pool, a.batch)
    for i, name in enumerate(modes):        # a graph holds the addresses of its model: one model per mode then
      steps[name] = (first_step, first_close) if (i == 0 or not a.graph) else build(True, a.batch)[1:]
    counter = {name: 0 for name in modes}

    def run_mode(name):
      batches = modes[name][0]
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for b in batches:
        counter[name] += 1
        steps[name][0](b, counter[name])
      e1.record()
      torch.cuda.synchronize()
      return e0.elapsed_time(e1)

    for _ in range(3):
      for name in modes:
        run_mode(name)
    times = {name: [] for name in modes}
    for _ in range(a.rounds):
      for name in modes:
        times[name].append(run_mode(name))
    out = {'caption_wordpieces': {'min': min(n_text), 'median': statistics.median(n_text), 'max': max(n_text)},
           'example_positions': live, 'modes': {}}
    for name, (batches, positions) in modes.items():
      n_steps = len(batches)
      used = n_steps * a.batch if name.startswith('unpacked') else N
      share_live = live * (used / N) if name.startswith('unpacked') else live
      out['modes'][name] = {'steps': n_steps, 'examples': used, 'positions_per_step': positions,
                            'padding_share': round(1.0 - share_live / (n_steps * positions), 4),
                            'ms_per_step': summary([t / n_steps for t in times[name]]),
                            'us_per_example': summary([t * 1e3 / used for t in times[name]])}
      out['modes'][name].update(pack_cost.get(name, {}))
    record['distributions'][dist] = out
    print(dist, json.dumps(out, indent=1), flush=True)
    for _, close in steps.values():
      close()
    del modes, pool, steps
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  with open(a.out, 'w') as f:
    json.dump(record, f, indent=1)


if __name__ == '__main__':
  main()
