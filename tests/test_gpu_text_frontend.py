"""mmt_text_tokens on the GPU, through the ctypes boundary on caller-owned buffers, against the oracle of
tests/_text_cases.py.  Parity is bit-exact.  The strings sit at odd offsets with sentinel bytes between them and a
guard behind the byte buffer; the three outputs are pre-filled with a sentinel and have a guard behind them, and every
comparison covers the whole buffer, so an element written outside [B, T] (or left unwritten inside) fails the test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _text_cases as tc

pytestmark = pytest.mark.gpu

FIELD_IDS = [5, 6, 7]            # [ATT], [REF], [ALT] of the synthetic vocabulary


@functools.lru_cache(maxsize=None)
def device_vocab():
  from mmt_amd import text_frontend as tf
  host = tf.WordpieceVocab(list(tc.vocab_tokens()))
  return host, host.to('cuda')


class Call:
  """Device buffers of one packed batch; run() is one mmt_text_tokens on them."""

  def __init__(self, examples, F, T, budget, workspace_fill=None):
    from mmt_amd import _lib
    self.lib = _lib
    blob, offsets, lengths, n = tc.pack(examples)
    self.B, self.F, self.T, self.budget, self.n = len(examples), F, T, budget, n
    self.bytes = torch.from_numpy(blob).cuda()
    self.offsets, self.lengths = torch.from_numpy(offsets).cuda(), torch.from_numpy(lengths).cuda()
    self.vocab = device_vocab()[1]
    fill32 = int(np.frombuffer(bytes([tc.SENTINEL]) * 4, dtype=np.int32)[0])
    self.ids = torch.full((self.B * T + tc.GUARD,), fill32, dtype=torch.int32, device='cuda')
    self.count = torch.full((self.B + tc.GUARD,), fill32, dtype=torch.int32, device='cuda')
    self.start = torch.full((self.B * T + tc.GUARD,), tc.SENTINEL, dtype=torch.uint8, device='cuda')
    self.fill32 = fill32
    self.need = _lib.lib().mmt_text_tokens_workspace_bytes(self.B, F, budget)
    self.ws = torch.empty(self.need, dtype=torch.uint8, device='cuda')
    if workspace_fill is not None:
      self.ws.fill_(workspace_fill)
    self.ftok = (ctypes.c_int32 * F)(*FIELD_IDS[:F])
    self.sep, self.unk = tc.special_ids()

  def run(self):
    v = self.vocab
    self.lib.check(self.lib.lib().mmt_text_tokens(
        self.B, self.F, self.bytes.data_ptr(), self.n, self.offsets.data_ptr(), self.lengths.data_ptr(), v.image.data_ptr(),
        v.image.numel(), v.codepoints.data_ptr(), v.codepoints.numel(), self.ftok, self.sep, self.unk, self.T, self.budget,
        self.ids.data_ptr(), self.count.data_ptr(), self.start.data_ptr(), self.ws.data_ptr(), self.need,
        torch.cuda.current_stream().cuda_stream))

  def result(self):
    torch.cuda.synchronize()
    return self.ids.cpu().numpy(), self.count.cpu().numpy(), self.start.cpu().numpy()

  def check(self, want, got=None):
    ids, count, start = got or self.result()
    guard32 = np.full(tc.GUARD, self.fill32, dtype=np.int32)
    assert np.array_equal(count, np.concatenate([want[1], guard32])), (count[:self.B], want[1])
    bad = np.nonzero(ids != np.concatenate([want[0].reshape(-1), guard32]))[0]
    assert bad.size == 0, (bad[:8] // self.T, bad[:8] % self.T, ids[bad[:8]])
    assert np.array_equal(start, np.concatenate([want[2].reshape(-1), np.full(tc.GUARD, tc.SENTINEL, dtype=np.uint8)]))


def expected(examples, F, T, budget):
  sep, unk = tc.special_ids()
  return tc.expected_rows(tc.vocab_dict(), examples, FIELD_IDS[:F], sep, unk, T, budget)


@pytest.mark.parametrize('name', sorted(tc.shape_cases()))
def test_shape_cases(name):
  """Word lengths round the 64-lane sweep and the 100-character limit, withdrawn pieces, prefix chains, F = 1, 2, 3 with
  empty, blank and ill-formed fields, the trim at and round the budget, budget 0, 20 KB fields (tests/_text_cases.py)."""
  examples, F, T, budget = tc.shape_cases()[name]
  c = Call(examples, F, T, budget)
  c.run()
  c.check(expected(examples, F, T, budget))


def test_every_token_of_a_colliding_vocabulary_finds_its_own_id():
  """1100 tokens in 4096 slots: some probe chains are longer than one slot (asserted on the image).  Every plain token as
  a field of its own gives its id; every `##` token gives its id behind the carrier `j`, which starts no other token.
  Tokens that are not in mapped form (upper case, accents) are left out: no text reaches them."""
  host, _ = device_vocab()
  words = host.image.numpy().view(np.uint32)
  nslots = int(words[2])
  slots = words[8:8 + 4 * nslots].reshape(nslots, 4)

  def home(key):
    x = int(key)
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    return x & (nslots - 1)
  displaced = sum(1 for s in range(nslots) if slots[s, 0] and home(slots[s, 1]) != s)
  assert displaced > 20, displaced
  v = tc.vocab_dict()
  assert not any(t.startswith('j') and t != 'j' for t in v)
  examples, own = [], []
  for tok, i in v.items():
    if tok.startswith('##') and len(tok) > 2:
      if tc.basic_tokens(tc.enc('j' + tok[2:])) != ['j' + tok[2:]]:
        continue                                  # not in mapped form (`##й`): no text reaches it, as in BERT's own files
      examples.append([tc.enc('j' + tok[2:])]); own.append([v['j'], i])
    elif tc.basic_tokens(tc.enc(tok)) == [tok]:
      examples.append([tc.enc(tok)]); own.append([i])
  assert len(examples) > 1000
  c = Call(examples, 1, 8, 6)
  c.run()
  want = expected(examples, 1, 8, 6)
  for b, o in enumerate(own):
    assert want[0][b, 1:1 + len(o)].tolist() == o and want[1][b] == 2 + len(o), (b, o)
  c.check(want)


def test_corpus_batch_and_python_paths():
  """The corpus as two-field examples in one call, then the Python entry on device tensors against the same entry on CPU
  tensors (and decode_text_features on the device against the oracle)."""
  from mmt_amd import configs
  from mmt_amd import text_frontend as tf
  cor = tc.corpus()
  examples = [[cor[i].encode('utf-8'), cor[i + 1].encode('utf-8')] for i in range(0, len(cor), 2)]
  c = Call(examples, 2, 24, 21)
  c.run()
  c.check(expected(examples, 2, 24, 21))
  host, dev = device_vocab()
  fields = [[ex[f] for ex in examples] for f in range(2)]
  on_cpu = tf.texts_to_token_features(host, fields, ['[ATT]', '[REF]'], 64, 6)
  on_dev = tf.texts_to_token_features(dev, fields, ['[ATT]', '[REF]'], 64, 6)
  for k, t in on_cpu.items():
    assert on_dev[k].is_cuda and on_dev[k].dtype == t.dtype and torch.equal(on_dev[k].cpu(), t), k
  cfg = configs.MmtPretrainDataConfig(max_seq_len=40, image_size=32, patch_size=16)
  got = tf.decode_text_features(cfg, dev, {'caption_attribution_description': fields[0], 'caption_reference_description': fields[1]})
  want = expected(examples, 2, 34, 31)
  assert np.array_equal(got['text_token_ids'].cpu().numpy(), want[0]) and np.array_equal(got['num_text_wordpieces'].cpu().numpy(), want[1])
  assert np.array_equal(got['text_word_start'].cpu().numpy().astype(np.uint8), want[2])


def test_repeatable_and_independent_of_the_workspace_contents():
  """Two calls on the same buffers give identical bytes, and a workspace pre-filled with 0xFF or 0x00 changes nothing."""
  examples, F, T, budget = tc.shape_cases()['trim']
  want = expected(examples, F, T, budget)
  first = Call(examples, F, T, budget)
  first.run()
  a = [x.copy() for x in first.result()]
  first.run()
  for x, y in zip(first.result(), a):
    assert np.array_equal(x, y)
  for fill in (0xFF, 0x00):
    other = Call(examples, F, T, budget, workspace_fill=fill)
    other.run()
    other.check(want)
  first.check(want, a)


def test_metadata_outside_the_buffer_is_clamped():
  """Offsets and lengths that leave the byte buffer: the row is that of the clamped field (here: what is left of the
  buffer, or nothing), and nothing outside the outputs is written."""
  examples = [[tc.enc('ab c')], [tc.enc('kk ab')], [tc.enc('abc')], [tc.enc('c')]]
  c = Call(examples, 1, 8, 6)
  host_off, host_len = c.offsets.cpu().numpy().copy(), c.lengths.cpu().numpy().copy()
  host_len[1] = 1 << 30                       # runs to the end of the buffer: the sentinels in between are dropped bytes
  host_off[2], host_len[2] = 1 << 40, 5       # behind the buffer: empty
  host_off[3], host_len[3] = -7, -3           # in front of it, negative length: empty
  c.offsets.copy_(torch.from_numpy(host_off)); c.lengths.copy_(torch.from_numpy(host_len))
  c.run()
  rest = c.bytes.cpu().numpy()[int(host_off[1]):c.n].tobytes()
  assert rest.startswith(b'kk ab') and rest.endswith(b'c') and bytes([tc.SENTINEL]) in rest
  clamped = [examples[0], [rest], [b''], [b'']]
  c.check(expected(clamped, 1, 8, 6))


def test_recorded_graph_follows_new_bytes():
  """One call recorded with torch.cuda.graph on a single stream; the bytes are overwritten in place (same offsets) and
  the replay is compared with the oracle for the new text."""
  old = [[tc.enc('abc kk, ab'), tc.enc('c 一')], [tc.enc('kq'), tc.enc('abcbc')]]
  new = [[tc.enc('kk ab, abc'), tc.enc('一 c')], [tc.enc('ab'), tc.enc('cbcab')]]
  assert [[len(f) for f in ex] for ex in old] == [[len(f) for f in ex] for ex in new]
  c = Call(old, 2, 16, 13)
  c.run()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    c.run()
  graph.replay()
  c.check(expected(old, 2, 16, 13))
  c.bytes.copy_(torch.from_numpy(tc.pack(new)[0]))
  graph.replay()
  c.check(expected(new, 2, 16, 13))
