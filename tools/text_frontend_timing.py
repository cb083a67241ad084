"""Call times of mmt_text_tokens (csrc/text_tokens.hip) on a batch a data loader would hand over: 256 examples, two
fields of caption-like text glued from the pieces of the tests' synthetic vocabulary, max_seq_len 512 behind 196
patches.  The device call is timed with HIP events on resident buffers: warm-up, then rounds of calls; median and range
over the rounds.  Where the `tokenizers` package is installed, its `encode_batch` over the same strings (BertNormalizer,
BertPreTokenizer, WordPiece; tokenisation only, no trim and no rows) is timed on the host in the same rounds.

A record, not a gate: nothing is asserted on the times.  Writes one JSON record (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'multimodal-long-transformer-2021_amd'))


def captions(tokens, batch, words_lo, words_hi, seed):
  import numpy as np
  rng = np.random.default_rng(seed)
  pieces = [t[2:] if t.startswith('##') and len(t) > 2 else t for t in tokens if not t.startswith('[') and len(t) < 12]
  out = []
  for _ in range(batch):
    words = []
    for _ in range(int(rng.integers(words_lo, words_hi))):
      w = ''.join(pieces[int(i)] for i in rng.integers(0, len(pieces), size=int(rng.integers(1, 4))))
      words.append(w.capitalize() if rng.random() < 0.15 else w)
    out.append(' '.join(words))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--max-seq-len', type=int, default=512)
  ap.add_argument('--num-patches', type=int, default=196)
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--calls', type=int, default=20, help='calls per round')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'text_frontend_timing.json'))
  args = ap.parse_args()

  import ctypes
  import torch
  from mmt_amd import _lib
  from mmt_amd import text_frontend as tf
  from tests import _text_cases as tc
  assert torch.cuda.is_available(), 'text_frontend_timing needs a GPU'
  dev = torch.device('cuda:0')
  B, F = args.batch, 2
  T = args.max_seq_len - args.num_patches - 2
  budget = T - F - 1
  tokens = tc.vocab_tokens()
  vocab = tf.WordpieceVocab(list(tokens)).to(dev)
  fields = [captions(tokens, B, 8, 40, 1), captions(tokens, B, 20, 120, 2)]        # a short and a long caption field
  (data, offsets, lengths), _ = tf._pack_fields(fields, dev)
  ids = torch.empty(B, T, dtype=torch.int32, device=dev)
  count = torch.empty(B, dtype=torch.int32, device=dev)
  start = torch.empty(B, T, dtype=torch.uint8, device=dev)
  L = _lib.lib()
  need = L.mmt_text_tokens_workspace_bytes(B, F, budget)
  ws = torch.empty(need, dtype=torch.uint8, device=dev)
  ftok = (ctypes.c_int32 * F)(vocab.id('[ATT]'), vocab.id('[REF]'))
  sep, unk = vocab.id('[SEP]'), vocab.id('[UNK]')
  stream = torch.cuda.current_stream(dev).cuda_stream

  def call():
    _lib.check(L.mmt_text_tokens(B, F, data.data_ptr(), data.numel(), offsets.data_ptr(), lengths.data_ptr(), vocab.image.data_ptr(),
                                 vocab.image.numel(), vocab.codepoints.data_ptr(), vocab.codepoints.numel(), ftok, sep, unk, T, budget,
                                 ids.data_ptr(), count.data_ptr(), start.data_ptr(), ws.data_ptr(), need, stream))

  hf = None
  try:
    import tokenizers
    hf = tokenizers.Tokenizer(tokenizers.models.WordPiece(dict(tc.vocab_dict()), unk_token='[UNK]', max_input_chars_per_word=100))
    hf.normalizer = tokenizers.normalizers.BertNormalizer()
    hf.pre_tokenizer = tokenizers.pre_tokenizers.BertPreTokenizer()
  except ImportError:
    pass
  strings = [s for col in fields for s in col]

  for _ in range(3):
    call()
    if hf is not None:
      hf.encode_batch(strings, add_special_tokens=False)
  torch.cuda.synchronize()
  dev_us, hf_us = [], []
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for _ in range(args.rounds):
    e0.record()
    for _ in range(args.calls):
      call()
    e1.record()
    torch.cuda.synchronize()
    dev_us.append(e0.elapsed_time(e1) / args.calls * 1e3)
    if hf is not None:
      t0 = time.perf_counter()
      for _ in range(args.calls):
        hf.encode_batch(strings, add_special_tokens=False)
      hf_us.append((time.perf_counter() - t0) / args.calls * 1e6)
  n_pieces = int(count.sum()) - B * (F + 1)
  summary = lambda ts: {'us_median': round(statistics.median(ts), 1), 'us_min': round(min(ts), 1), 'us_max': round(max(ts), 1)}
  record = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_round': args.calls,
            'shape': dict(B=B, F=F, T=T, budget=budget, text_bytes=int(data.numel()), kept_wordpieces=n_pieces,
                          rows_trimmed=int((count == T).sum())),
            'mmt_text_tokens': summary(dev_us)}
  if hf_us:
    record['tokenizers_encode_batch'] = dict(summary(hf_us), version=tokenizers.__version__, host_threads=os.cpu_count(),
                                             note='host, tokenisation only (no trim, no rows)')
  print(json.dumps(record, indent=1))
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(record, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
