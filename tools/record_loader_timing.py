"""Times of the record container and the pretraining loader (csrc/records.hip, mmt_amd/records.py,
mmt_amd/pretrain_dataloader.py).  Device stages by HIP events: warm-up, then rounds of calls, median and range over the
rounds; host stages by wall clock, best of 3.  A record, not a gate: nothing is asserted on the times.

  (a) mmt_records_crc against its host mirror (one thread) on two blobs: the 64 synthesised JPEG files of
      tools/jpeg_decode_timing.py as one record each, and 4096 records of 100 bytes; bytes per second against the HBM rate
      the microarchitecture guide gives as sustained (6.3 TB/s).  The words are checked against the mirror's first.
  (b) the loader per batch at the benchmark's shape (BASELINE config 3: batch 4, max_seq_len 4096, image 1008, patch 16),
      on shards written here from the same synthesised files: host milliseconds for read + scan, copy + field lookup and
      the JPEG plan; the upload; the device stages one by one; and a whole `next(loader)`.  tasks = 'mlm': the matching
      step needs more than 7 examples in a batch (ratio 1, min_shift 5), which a per-replica batch of 4 does not give.
  (c) with --finetune, alone: the fine-tuning loader (mmt_amd/classification_dataloader.py) per batch and the retrieval
      set build (mmt_amd/retrieval_dataloader.py, 64 images and 512 texts) at the fine-tuning shape (batch 64,
      max_seq_len 256, image 224, patch 16, ratio 1), beside the fine-tuning step of the same run.
  (d) with --masking, alone: the masking stage of (b), `random_item_masking` over [4, 3971] and [4, 125] together, and the
      fine-tuning shape [64, 256]: the one launch of csrc/item_masking.hip against the torch ops (`kernel=False`) in the
      same call, the two routes alternating, after their outputs were compared bit for bit.

  (e) with --prefetch, alone: the train step at the shape of (b), recorded as a HIP graph, fed by one resident batch, by the
      plain loader on the training thread, and by the loader behind a `prefetch.Prefetcher` of depth 2; three readings of
      --steps steps each, alternating, host clock around a final synchronise.

Writes one JSON record (--out, default profiles/record_loader_timing.json; profiles/finetune_loader_timing.json for (c),
profiles/masking_timing.json for (d), profiles/prefetch_timing.json for (e))."""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))

from tools.jpeg_decode_timing import encode_jpeg  # noqa: E402

HBM_SUSTAINED_GB_S = 6300.0
VOCAB = ['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '[PATCH]', '[ATT]', '[REF]'] + [f'[unused{i}]' for i in range(1100)]
WORDS = ['a', 'photo', 'of', 'the', 'old', 'bridge', 'over', 'river', 'at', 'dawn', 'with', 'two', 'boats', 'and', 'fog', '##s', '##ing', ',', '.']


def _table():
  t = []
  for v in range(256):
    c = v
    for _ in range(8):
      c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    t.append(c)
  return np.asarray(t, dtype=np.uint32)


def crc32c(data: bytes) -> int:
  """Bytewise, through numpy per byte position is not possible (a recurrence): plain Python, used on headers only."""
  t, c = _table(), 0xFFFFFFFF
  for b in data:
    c = int(t[(c ^ b) & 0xFF]) ^ (c >> 8)
  return c ^ 0xFFFFFFFF


def mask(c):
  return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


def varint(v):
  out = bytearray()
  while v >= 0x80:
    out.append((v & 0x7F) | 0x80)
    v >>= 7
  out.append(v)
  return bytes(out)


def ld(field, body):
  return varint(field << 3 | 2) + varint(len(body)) + body


def example(feats):
  return ld(1, b''.join(ld(1, ld(1, k.encode()) + ld(2, ld(1, ld(1, v)))) for k, v in feats))


def event_times(torch, call, rounds, calls, warmup=3):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for _ in range(warmup):
    call()
  torch.cuda.synchronize()
  ts = []
  for _ in range(rounds):
    e0.record()
    for _ in range(calls):
      call()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / calls * 1e3)
  return {'us_median': round(statistics.median(ts), 1), 'us_min': round(min(ts), 1), 'us_max': round(max(ts), 1)}


def wall_best(call, n=3):
  best = None
  for _ in range(n):
    t0 = time.perf_counter()
    call()
    dt = time.perf_counter() - t0
    best = dt if best is None else min(best, dt)
  return round(best * 1e3, 3)


def crc_leg(torch, _lib, name, payloads, args):
  """mmt_records_crc by events against mmt_records_crc_host by wall clock on one blob of back-to-back payloads."""
  L = _lib.lib()
  n = len(payloads)
  blob = np.frombuffer(b''.join(payloads), dtype=np.uint8).copy()
  recs = (_lib.Record * n)()
  at = 0
  for i, p in enumerate(payloads):
    recs[i].offset, recs[i].length = at, len(p)
    at += len(p)
  need = L.mmt_records_crc_workspace_bytes(n)
  crc_h, bad_h = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
  ws_h = np.zeros(need // 8 + 2, dtype=np.int64)
  ws_ptr = (ws_h.ctypes.data + 15) & ~15
  host = lambda: _lib.check(L.mmt_records_crc_host(blob.ctypes.data, blob.size, n, ctypes.addressof(recs), crc_h.ctypes.data,
                                                    bad_h.ctypes.data, ws_ptr, need))
  host_ms = wall_best(host)
  blob_d = torch.from_numpy(blob).cuda()
  recs_d = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).cuda()
  crc_d = torch.empty(n, dtype=torch.int32, device='cuda')
  bad_d = torch.empty(n, dtype=torch.int32, device='cuda')
  ws_d = torch.empty(need, dtype=torch.uint8, device='cuda')
  stream = torch.cuda.current_stream().cuda_stream
  dev = lambda: _lib.check(L.mmt_records_crc(blob_d.data_ptr(), blob.size, n, recs_d.data_ptr(), crc_d.data_ptr(), bad_d.data_ptr(),
                                              ws_d.data_ptr(), need, stream))
  dev()
  torch.cuda.synchronize()
  assert np.array_equal(crc_d.cpu().numpy().view(np.uint32), crc_h), 'the kernels and the host mirror disagree'
  t = event_times(torch, dev, args.rounds, args.calls)
  gbs = blob.size / t['us_median'] / 1e3
  out = {'records': n, 'bytes': int(blob.size), 'host_mirror_ms_one_thread': host_ms, 'host_gb_per_s': round(blob.size / host_ms / 1e6, 2),
         'device': t, 'device_gb_per_s': round(gbs, 1), 'fraction_of_hbm_sustained': round(gbs / HBM_SUSTAINED_GB_S, 4),
         'device_over_host': round(host_ms * 1e3 / t['us_median'], 1)}
  print(f'  crc {name}: {n} records, {blob.size} bytes: host mirror {host_ms} ms (1 thread), device {t["us_median"]} us '
        f'({t["us_min"]}..{t["us_max"]}), {out["device_gb_per_s"]} GB/s = {out["fraction_of_hbm_sustained"]:.2%} of {HBM_SUSTAINED_GB_S:.0f} GB/s')
  return out


def config3_shard(torch, _lib, files):
  """One shard of 16 records at the benchmark's shape (batch 4, max_seq_len 4096, image 1008, patch 16) from the
  synthesised files, with its vocabulary: (shard, vocab_path, fields, payloads, (B, S, IMG, PATCH))."""
  from mmt_amd import records
  L = _lib.lib()
  B, S, IMG, PATCH = 4, 4096, 1008, 16
  rng = np.random.default_rng(1)
  text = lambda n: ' '.join(WORDS[int(i)] for i in rng.integers(0, 15, size=n))
  work = tempfile.mkdtemp(prefix='record_loader_timing_')
  vocab_path = os.path.join(work, 'vocab.txt')
  with open(vocab_path, 'w') as f:
    f.write('\n'.join(VOCAB + WORDS) + '\n')
  fields = {'caption_attribution_description': '[ATT]', 'caption_reference_description': '[REF]'}
  payloads = [example([('image_key', f'k{i}'.encode()), ('image_data', files[i % len(files)]), ('caption_attribution_description', text(60).encode()),
                       ('caption_reference_description', text(80).encode())]) for i in range(4 * B)]
  shard = os.path.join(work, 'timing-00000-of-00001.tfrecord')
  with open(shard, 'wb') as f:
    for p in payloads:
      head = struct.pack('<Q', len(p))
      f.write(head + struct.pack('<I', mask(crc32c(head))) + p + struct.pack('<I', 0))     # payload checksums: see below
  # the stored payload checksums come from the library's host mirror (plain Python over megabytes would take minutes)
  raw = [(p, c) for p, c in records.read_shard(shard)]
  blob, recs, _ = records.pack_records([p for p, _ in raw], [0] * len(raw), [])
  crc = torch.empty(len(raw), dtype=torch.int32); bad = torch.empty(len(raw), dtype=torch.int32)
  need = L.mmt_records_crc_workspace_bytes(len(raw))
  ws = torch.empty(need + 16, dtype=torch.uint8)
  _lib.check(L.mmt_records_crc_host(blob.data_ptr(), blob.numel(), len(raw), ctypes.addressof(recs), crc.data_ptr(), bad.data_ptr(),
                                    (ws.data_ptr() + 15) & ~15, need))
  with open(shard, 'wb') as f:
    for p, c in zip(payloads, crc.numpy().view(np.uint32).tolist()):
      head = struct.pack('<Q', len(p))
      f.write(head + struct.pack('<I', mask(crc32c(head))) + p + struct.pack('<I', mask(c)))

  return shard, vocab_path, fields, payloads, (B, S, IMG, PATCH)


def loader_leg(torch, _lib, files, args):
  from mmt_amd import configs, feature_pipeline as fp, input_utils, pretrain_dataloader as pd, records, text_frontend
  from mmt_amd.ops import side_inputs
  L = _lib.lib()
  shard, vocab_path, fields, payloads, (B, S, IMG, PATCH) = config3_shard(torch, _lib, files)
  cfg = configs.MmtPretrainDataConfig(input_path=shard, vocab_filename=vocab_path, is_training=True, global_batch_size=B, image_size=IMG,
                                      patch_size=PATCH, max_seq_len=S, tasks='mlm', text_special_token_field_dict=json.dumps(fields), seed=3)
  loader = pd.MmtPretrainDataLoader(cfg, device='cuda', shuffle_buffer=8)
  dev = torch.device('cuda')
  out = {'shape': dict(batch=B, max_seq_len=S, image_size=IMG, patch_size=PATCH, tasks='mlm'), 'record_bytes': len(payloads[0])}

  # host stages
  out['host_read_scan_ms_per_batch'] = round(wall_best(lambda: list(records.read_shard(shard))) * B / len(payloads), 3)
  group = [(p, c) for p, c in records.read_shard(shard)][:B]
  pack = lambda: records.pack_records([g[0] for g in group], [g[1] for g in group], loader.names)
  out['host_copy_lookup_ms_per_batch'] = wall_best(pack)
  blob, recs, fl = pack()
  view = blob.numpy()
  bufs = [view[f[0].offset:f[0].offset + f[0].length] for f in fl]

  def plan():
    for a in bufs:
      im, scan = _lib.JpegImage(), _lib.JpegScan()
      _lib.check(L.mmt_jpeg_info(a.ctypes.data, a.size, ctypes.byref(im)))
      _lib.check(L.mmt_jpeg_scan_plan(a.ctypes.data, a.size, ctypes.byref(im), fp.JPEG_ENTROPY_SUBSEQ_BYTES, ctypes.byref(scan), None, None,
                                      None, 0, None, 0))
      huff, qt = np.empty(6 * _lib.MMT_JPEG_HUFF_WORDS, dtype=np.uint32), np.empty(192, dtype=np.uint16)
      seg, sub = np.empty(scan.n_segments * 4, dtype=np.int32), np.empty(scan.n_subseq, dtype=np.int32)
      _lib.check(L.mmt_jpeg_scan_plan(a.ctypes.data, a.size, ctypes.byref(im), fp.JPEG_ENTROPY_SUBSEQ_BYTES, ctypes.byref(scan), huff.ctypes.data,
                                      qt.ctypes.data, seg.ctypes.data, scan.n_segments, sub.ctypes.data, scan.n_subseq))
  out['host_jpeg_plan_ms_per_batch_one_thread'] = wall_best(plan)

  # upload and device stages
  blob_d = blob.to(dev)
  out['upload'] = dict(bytes=int(blob.numel()), **event_times(torch, lambda: blob_d.copy_(blob, non_blocking=True), args.rounds, args.calls))
  out['device_records_crc'] = event_times(torch, lambda: records.payload_checksums(blob_d, recs, B), args.rounds, args.calls)
  at = [int(f[0].offset) for f in fl]
  decode = lambda: fp.decode_jpeg_images(bufs, dev, entropy='device', uploaded=(blob_d, at))
  out['jpeg_decode_call_wall_ms'] = wall_best(lambda: (decode(), torch.cuda.synchronize()))     # plans on the host, kernels, one read-back
  packed = decode()
  gen = torch.Generator(device=dev).manual_seed(1)
  out['device_image_features'] = event_times(torch, lambda: fp.decode_image_features(cfg, packed, generator=gen, keep_unnormalized=True),
                                             args.rounds, args.calls)
  meta = lambda v, dt: torch.tensor(v, dtype=dt).to(dev)
  t_off = meta([int(f[j].offset) for f in fl for j in (2, 3)], torch.int64)
  t_len = meta([int(f[j].length) for f in fl for j in (2, 3)], torch.int32)
  vocab = loader.vocab()
  out['device_text_tokens'] = event_times(torch, lambda: text_frontend.decode_text_features(cfg, vocab, (blob_d, t_off, t_len)),
                                          args.rounds, args.calls)
  feats = loader._decode([(p, c, shard, i) for i, (p, c) in enumerate(group)], gen)
  out['device_masking'] = event_times(torch, lambda: loader._mask(dict(feats), gen), args.rounds, args.calls)
  ex = loader._mask(dict(feats), gen)
  out['device_side_inputs_and_split'] = event_times(torch, lambda: loader._finish(dict(ex), False), args.rounds, args.calls)

  it = loader.load()
  for _ in range(3):
    next(it)
  torch.cuda.synchronize()
  ts = []
  for _ in range(max(args.rounds, 5)):
    t0 = time.perf_counter()
    next(it)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
  out['loader_next_ms'] = {'median': round(statistics.median(ts), 2), 'min': round(min(ts), 2), 'max': round(max(ts), 2)}
  for k, v in out.items():
    print(f'  loader {k}: {v}')
  return out


def example_with_ints(feats):
  """feats: (name, bytes | int) in wire order; an int becomes an int64 list of one value."""
  def feature(v):
    return ld(3, ld(1, varint(v))) if isinstance(v, int) else ld(1, ld(1, v))
  return ld(1, b''.join(ld(1, ld(1, k.encode()) + ld(2, feature(v))) for k, v in feats))


def write_shard(torch, _lib, path, payloads):
  """A TFRecord file of the payloads; the payload checksums come from the library's host mirror (plain Python over
  megabytes would take minutes)."""
  from mmt_amd import records
  L = _lib.lib()
  n = len(payloads)
  blob, recs, _ = records.pack_records(payloads, [0] * n, [])
  crc, bad = torch.empty(n, dtype=torch.int32), torch.empty(n, dtype=torch.int32)
  need = L.mmt_records_crc_workspace_bytes(n)
  ws = torch.empty(need + 16, dtype=torch.uint8)
  _lib.check(L.mmt_records_crc_host(blob.data_ptr(), blob.numel(), n, ctypes.addressof(recs), crc.data_ptr(), bad.data_ptr(),
                                    (ws.data_ptr() + 15) & ~15, need))
  with open(path, 'wb') as f:
    for p, c in zip(payloads, crc.numpy().view(np.uint32).tolist()):
      head = struct.pack('<Q', len(p))
      f.write(head + struct.pack('<I', mask(crc32c(head))) + p + struct.pack('<I', mask(c)))
  return path


def finetune_leg(torch, _lib, args):
  """(c) the fine-tuning loader per batch and the retrieval set build at the fine-tuning shape (max_seq_len 256, image
  224, patch 16, per-replica batch 64, ratio 1), beside the fine-tuning step of the same run: the base encoder in
  bfloat16 with one ITM head, one `train_step` on loader batches.  The loader decodes a matching group (128 records)
  at a time and hands it out as four batches, so `next(loader)` is timed over whole groups: the mean per batch, and the
  longest single call (the one that decodes).  The set build is 64 images and 512 texts from separate files, the sets
  of tools/retrieval_pairs_timing.py; decode time is taken around the two decode stages with a device synchronisation."""
  import mmt_amd
  from mmt_amd import classification_dataloader as cd, configs, optimization, retrieval_dataloader as rd
  B, S, IMG, PATCH, I, T = 64, 256, 224, 16, 64, 512
  rng = np.random.default_rng(2)
  text = lambda n: ' '.join(WORDS[int(i)] for i in rng.integers(0, 15, size=n))
  t0 = time.perf_counter()
  files = [encode_jpeg(rng.integers(0, 256, size=(IMG, IMG, 3), dtype=np.uint8), args.quality) for _ in range(16)]
  print(f'encoded 16 contents of {IMG} x {IMG} in {time.perf_counter() - t0:.1f} s; {len(files[0])} bytes per file')
  work = tempfile.mkdtemp(prefix='finetune_loader_timing_')
  vocab_path = os.path.join(work, 'vocab.txt')
  with open(vocab_path, 'w') as f:
    f.write('\n'.join(VOCAB + WORDS) + '\n')
  fields = {'caption_attribution_description': '[ATT]', 'caption_reference_description': '[REF]'}
  texts = lambda: [('caption_attribution_description', text(20).encode()), ('caption_reference_description', text(30).encode())]
  n_rec = 4 * 2 * B
  for s in range(2):
    write_shard(torch, _lib, os.path.join(work, f'train-{s}.tfrecord'),
                [example([('image_key', f'k{i}'.encode()), ('image_data', files[i % len(files)])] + texts()) for i in range(s, n_rec, 2)])
  write_shard(torch, _lib, os.path.join(work, 'image.tfrecord'),
              [example_with_ints([('image_index', 3 * i + 1), ('image_data', files[i % len(files)])]) for i in range(I)])
  write_shard(torch, _lib, os.path.join(work, 'text.tfrecord'),
              [example_with_ints([('text_index', 5 * t + 2), ('gt_image_index', 3 * (t % I) + 1)] + texts()) for t in range(T)])

  exp = configs.get_exp_config('mmt/classification')
  exp.override({'task': {'model': {'num_classes': 2, 'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]},
                         'train_data': dict(input_path=os.path.join(work, 'train-*.tfrecord'), vocab_filename=vocab_path, is_training=True,
                                            global_batch_size=B, max_seq_len=S, image_size=IMG, patch_size=PATCH,
                                            negative_positive_ratio=1, text_special_token_field_dict=json.dumps(fields), seed=3,
                                            label_field='itm_label_ids', label_weights_field='itm_label_weights',
                                            pos_weights_field='itm_pos_weights')}}, strict=False)
  d = exp.task.train_data
  out = {'shape': dict(batch=B, max_seq_len=S, image_size=IMG, patch_size=PATCH, negative_positive_ratio=1,
                       matching_group=int(2 * B)), 'image_file_bytes': len(files[0])}
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt = optimization.create_optimizer(model, exp.trainer.optimizer_config)
  it = task.build_inputs(d, device='cuda', batch_size=B)
  assert task.input_source == 'records'
  for _ in range(8):                                             # two groups: warm-up of every stage
    next(it)
  torch.cuda.synchronize()
  ts = []
  for _ in range(16):
    t0 = time.perf_counter()
    batch = next(it)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
  out['loader_next_ms'] = {'mean_per_batch': round(sum(ts) / len(ts), 2), 'longest_call': round(max(ts), 2),
                           'median_call': round(statistics.median(ts), 2), 'calls': len(ts)}
  out['loader_examples_per_s'] = round(B * len(ts) / (sum(ts) / 1e3), 1)
  steps = []
  for k in range(3 + 5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    task.train_step(batch, model, opt, clip_norm=1.0, step=k + 1, micro_batch_size=B)
    torch.cuda.synchronize()
    steps.append((time.perf_counter() - t0) * 1e3)
  out['finetune_step_ms'] = {'median': round(statistics.median(steps[3:]), 2), 'min': round(min(steps[3:]), 2),
                             'max': round(max(steps[3:]), 2), 'steps': len(steps) - 3, 'model': 'base encoder, bfloat16, one ITM head'}
  del model, opt

  rcfg = configs.MmtRetrievalDataConfig(image_input_path=os.path.join(work, 'image.tfrecord'), text_input_path=os.path.join(work, 'text.tfrecord'),
                                        vocab_filename=vocab_path, is_training=False, max_seq_len=S, image_size=IMG, patch_size=PATCH,
                                        text_special_token_field_dict=json.dumps(fields))
  builds = []
  for _ in range(3):                                             # the first build warms up; the best of the others is kept
    loader = rd.MmtRetrievalDataLoader(rcfg, device='cuda', chunk=64)
    spent = {'images': 0.0, 'texts': 0.0}

    def timed(call, key):
      def run(*a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(*a)
        torch.cuda.synchronize()
        spent[key] += time.perf_counter() - t0
      return run
    loader._decode_images = timed(loader._decode_images, 'images')
    loader._decode_text_rows = timed(loader._decode_text_rows, 'texts')
    t0 = time.perf_counter()
    sets = loader.sets()
    torch.cuda.synchronize()
    builds.append((time.perf_counter() - t0, spent['images'], spent['texts']))
  assert sets.num_images == I and sets.num_texts == T
  total, t_img, t_txt = min(builds[1:])
  out['retrieval_set_build'] = {'images': I, 'texts': T, 'chunk': 64, 'whole_build_ms': round(total * 1e3, 2),
                                'image_decode_ms': round(t_img * 1e3, 2), 'text_decode_ms': round(t_txt * 1e3, 2),
                                'images_per_s': round(I / t_img, 1), 'texts_per_s': round(T / t_txt, 1)}
  for k, v in out.items():
    print(f'  finetune {k}: {v}')
  return out


def masking_leg(torch, args):
  """The masking stage alone, `random_item_masking` through its one launch against `kernel=False` (the torch ops) in the
  same call, HIP events: the config-3 pair of calls -- the patch row [4, 3971], every token an item, and the text row
  [4, 125] with whole words -- timed together, as `device_masking` of leg (b) holds them, and the fine-tuning shape
  [64, 256]."""
  from mmt_amd import feature_pipeline as fp
  g = torch.Generator(device='cuda').manual_seed(5)

  def inputs(B, T, whole_word, rate, cap):
    tok = torch.randint(1000, 30000, (B, T), device='cuda', generator=g).to(torch.int32)
    tok[:, 0] = 101
    kw = dict(selection_rate=rate, max_selections=cap, unselectable_ids=[101, 102, 5, 6], mask_token_id=103,
              item_keys=torch.rand(B, T, device='cuda', generator=g), value_u=torch.rand(B, T, device='cuda', generator=g),
              random_ids=torch.randint(0, 30000, (B, T), device='cuda', generator=g).to(torch.int32),
              word_start=(torch.rand(B, T, device='cuda', generator=g) < 0.6) if whole_word else None)
    n = torch.randint(T // 2, T + 1, (B,), device='cuda', generator=g) if whole_word else torch.full((B,), T, device='cuda')
    return tok, n, kw

  shapes = {'config3_patches_4x3971_and_text_4x125': [inputs(4, 3971, False, 0.5, 1985), inputs(4, 125, True, 0.15, 125)],
            'finetune_64x256': [inputs(64, 256, True, 0.15, 20)]}
  out = {}
  for name, calls in shapes.items():
    def run(kernel):
      return [fp.random_item_masking(tok, n, kernel=kernel, **kw) for tok, n, kw in calls]
    for a, b in zip(run(True), run(False)):
      assert all(torch.equal(x, y) for x, y in zip(a, b)), name
    # alternate the two routes, so that a drift of the clocks falls on both
    rec = {'kernel': [], 'torch_ops': []}
    for _ in range(3):
      rec['kernel'].append(event_times(torch, lambda: run(True), args.rounds, args.calls))
      rec['torch_ops'].append(event_times(torch, lambda: run(False), args.rounds, args.calls))
    out[name] = {k: {'us_median': statistics.median(r['us_median'] for r in v), 'us_min': min(r['us_min'] for r in v),
                     'us_max': max(r['us_max'] for r in v), 'repeats_us_median': [r['us_median'] for r in v]} for k, v in rec.items()}
    print(name, json.dumps(out[name]))
  return out


def prefetch_leg(torch, _lib, files, args):
  """The train step at the config-3 shape (bench.py's model and optimizer, recorded as a HIP graph; tasks = 'mlm', as in
  leg (b)) fed three ways, alternating in one process, `--steps` steps each after warm-up, host clock around a final
  synchronise: one resident batch; the plain loader on the training thread; the loader behind a Prefetcher of depth 2."""
  import bench
  from mmt_amd import distribute, graphed, optimization, tasks, configs
  shard, vocab_path, fields, _, (B, S, IMG, PATCH) = config3_shard(torch, _lib, files)
  c = bench.get_config(3)
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {'micro_batch_size': B,
                         'model': {'encoder': {'mmt': {'relative_pos_max_distance': c['m'], 'relative_vocab_size': c['R']}},
                                   'cls_heads': [{'inner_dim': 768, 'num_classes': 2, 'name': 'itm'}]},
                         'train_data': dict(input_path=shard, vocab_filename=vocab_path, max_seq_len=S, image_size=IMG, patch_size=PATCH,
                                            global_batch_size=B, tasks='mlm', mpp_fraction_to_mask=0.0, seed=3,
                                            text_special_token_field_dict=json.dumps(fields), relative_pos_max_distance=c['m'],
                                            local_radius=c['radius'], num_global_tokens=c['ng'])}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt_cfg = exp.trainer.optimizer_config
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()), reduce=tasks.gradient_reduce_mode(exp.task))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  step = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, clip_norm=opt_cfg.gradient_clip_norm)
  d = exp.task.train_data
  plain = task.build_inputs(d, device='cuda', batch_size=B, loader_args=dict(shuffle_buffer=8))
  d.prefetch_buffer_size = 2
  ahead = task.build_inputs(d, device='cuda', batch_size=B, loader_args=dict(shuffle_buffer=8))
  ahead.timeout = 120
  resident = next(plain)
  feeds = {'resident_batch': lambda: resident, 'plain_loader': lambda: next(plain), 'prefetched_depth_2': lambda: next(ahead)}
  n = {'i': 0}

  def run(feed, steps):
    for _ in range(steps):
      n['i'] += 1
      step(feed(), n['i'])
    torch.cuda.synchronize()
  out = {'shape': dict(batch=B, max_seq_len=S, image_size=IMG, patch_size=PATCH, tasks='mlm'), 'steps_per_reading': args.steps}
  try:
    for feed in feeds.values():                                    # warm-up: the eager steps, the recording, every feed
      run(feed, 6)
    assert step.graph is not None, 'the step was not recorded'
    ms = {k: [] for k in feeds}
    for _ in range(3):
      for k, feed in feeds.items():
        t0 = time.perf_counter()
        run(feed, args.steps)
        ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for k, v in ms.items():
      out[k] = {'ms_per_step_median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
      print(f'  prefetch {k}: {out[k]}')
  finally:
    ahead.close()
    step.close()
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--finetune', action='store_true', help='run leg (c) alone and write profiles/finetune_loader_timing.json')
  ap.add_argument('--masking', action='store_true', help='time the masking stage alone and write profiles/masking_timing.json')
  ap.add_argument('--prefetch', action='store_true', help='time the train step fed three ways and write profiles/prefetch_timing.json')
  ap.add_argument('--steps', type=int, default=100, help='steps of one reading of --prefetch')
  ap.add_argument('--batch', type=int, default=64)
  ap.add_argument('--size', type=int, default=1008)
  ap.add_argument('--quality', type=int, default=90)
  ap.add_argument('--distinct', type=int, default=8, help='contents encoded; repeated to fill the batch')
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=4)
  ap.add_argument('--bench-ms-per-step', type=float, default=None, help="bench.py's ms_per_step at the parent commit, recorded beside (b)")
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'record_loader_timing.json'))
  args = ap.parse_args()
  import torch
  from mmt_amd import _lib
  assert torch.cuda.is_available(), 'record_loader_timing needs a GPU'
  if args.masking:
    out = args.out if args.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'masking_timing.json')
    record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls,
              'masking': masking_leg(torch, args)}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(record, f, indent=1)
    print('wrote', out)
    return
  if args.prefetch:
    out = args.out if args.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'prefetch_timing.json')
    rng = np.random.default_rng(0)
    distinct = [encode_jpeg(rng.integers(0, 256, size=(args.size, args.size, 3), dtype=np.uint8), args.quality) for _ in range(min(args.distinct, 4))]
    record = {'device': torch.cuda.get_device_name(0), 'prefetch': prefetch_leg(torch, _lib, distinct, args)}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(record, f, indent=1)
    print('wrote', out)
    return
  if args.finetune:
    out = args.out if args.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'finetune_loader_timing.json')
    record = {'device': torch.cuda.get_device_name(0), 'finetune': finetune_leg(torch, _lib, args)}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
      json.dump(record, f, indent=1)
    print('wrote', out)
    return
  rng = np.random.default_rng(0)
  t0 = time.perf_counter()
  distinct = [encode_jpeg(rng.integers(0, 256, size=(args.size, args.size, 3), dtype=np.uint8), args.quality)
              for _ in range(min(args.distinct, args.batch))]
  files = [distinct[i % len(distinct)] for i in range(args.batch)]
  print(f'encoded {len(distinct)} contents in {time.perf_counter() - t0:.1f} s; {len(files[0])} bytes per file')
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls,
            'hbm_sustained_gb_per_s': HBM_SUSTAINED_GB_S,
            'crc': {'jpeg_files': crc_leg(torch, _lib, 'jpeg files', files, args),
                    'short_records': crc_leg(torch, _lib, 'short records', [rng.integers(0, 256, size=100, dtype=np.uint8).tobytes()
                                                                            for _ in range(4096)], args)},
            'loader': loader_leg(torch, _lib, distinct, args), 'bench_ms_per_step_at_parent': args.bench_ms_per_step}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
