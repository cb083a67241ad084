"""Text front end without a GPU: the oracle of tests/_text_cases.py against the `tokenizers` package, the plain-Python
path of mmt_amd.text_frontend and its code-point table against the oracle, the refusals of the C ABI and of the Python
functions, the vocabulary builder, and `decode_text_features` down to `make_mlm_and_mpp_features`."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _text_cases as tc


@pytest.fixture(scope='module')
def tf():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  from mmt_amd import text_frontend
  return text_frontend


@pytest.fixture(scope='module')
def vocab(tf):
  return tf.WordpieceVocab(list(tc.vocab_tokens()))


def test_oracle_agrees_with_the_tokenizers_package_on_the_whole_corpus():
  """Every string of the corpus: the oracle's ids are those of WordPiece(max_input_chars_per_word=100) behind
  BertNormalizer and BertPreTokenizer.  At most half of the ids are [UNK], so agreement is not agreement on [UNK]."""
  tokenizers = pytest.importorskip('tokenizers')
  vd = tc.vocab_dict()
  _, unk = tc.special_ids()
  hf = tokenizers.Tokenizer(tokenizers.models.WordPiece(dict(vd), unk_token='[UNK]', max_input_chars_per_word=100))
  hf.normalizer = tokenizers.normalizers.BertNormalizer()
  hf.pre_tokenizer = tokenizers.pre_tokenizers.BertPreTokenizer()
  total = unknown = 0
  for s in tc.corpus():
    mine = [p for p, _ in tc.field_pieces(vd, s.encode('utf-8'), unk)]
    assert mine == hf.encode(s, add_special_tokens=False).ids, repr(s)
    total += len(mine)
    unknown += mine.count(unk)
  assert total > 20000 and 0 < unknown <= total // 2, (total, unknown)
  for s in ('豈豈', 'áb [SEP]', 'x' * 101 + ' ' + 'k' * 100):     # a compatibility ideograph maps to its unified one
    assert [p for p, _ in tc.field_pieces(vd, s.encode('utf-8'), unk)] == hf.encode(s, add_special_tokens=False).ids, repr(s)


def _check(got, want):
  assert got['text_token_ids'].dtype == torch.int32 and got['num_text_wordpieces'].dtype == torch.int32
  assert got['text_word_start'].dtype == torch.bool
  assert np.array_equal(got['text_token_ids'].cpu().numpy(), want[0])
  assert np.array_equal(got['num_text_wordpieces'].cpu().numpy(), want[1])
  assert np.array_equal(got['text_word_start'].cpu().numpy().astype(np.uint8), want[2])


@pytest.mark.parametrize('name', sorted(tc.shape_cases()))
def test_cpu_path_equals_the_oracle_on_the_shape_cases(tf, vocab, name):
  examples, F, T, budget = tc.shape_cases()[name]
  sep, unk = tc.special_ids()
  field_ids = [5, 6, 7][:F]
  want = tc.expected_rows(tc.vocab_dict(), examples, field_ids, sep, unk, T, budget)
  fields = [[ex[f] for ex in examples] for f in range(F)]
  assert budget == T - F - 1
  _check(tf.texts_to_token_features(vocab, fields, field_ids, T + 2 + 4, 4), want)
  blob, offsets, lengths, n = tc.pack(examples)                      # the packed form, strings at odd offsets
  packed = (torch.from_numpy(blob[:n]), torch.from_numpy(offsets), torch.from_numpy(lengths))
  _check(tf.texts_to_token_features(vocab, packed, ['[ATT]', '[REF]', '[ALT]'][:F], T + 2, 0), want)


def test_cpu_path_and_code_point_table_equal_the_oracle_on_the_corpus(tf, vocab):
  cor = tc.corpus()
  sep, unk = tc.special_ids()
  table = tf.codepoint_table()
  for s in cor:                                                       # the table, word by word
    words = [''.join(chr(c) for c in w) for w in tf._words(table, s)]
    assert words == tc.basic_tokens(s.encode('utf-8')), repr(s)
  examples = [[cor[i].encode('utf-8'), cor[i + 1].encode('utf-8')] for i in range(0, len(cor), 2)]
  want = tc.expected_rows(tc.vocab_dict(), examples, [5, 6], sep, unk, 24, 21)
  fields = [[ex[f] for ex in examples] for f in range(2)]
  _check(tf.texts_to_token_features(vocab, fields, [5, 6], 26, 0), want)
  assert int((want[1] == 24).sum()) > 50 and int((want[1] < 24).sum()) > 50      # trimmed and untrimmed rows both occur


def test_code_point_table_on_single_code_points(tf):
  """Every code point below U+3100 and every 89th above, between two letters: the table's words are the oracle's."""
  table = tf.codepoint_table()
  assert table.dtype == np.uint32 and len(table) > 0x110000
  expanding = int((((table[:0x110000] >> 22) & 3) >= 2).sum())
  assert expanding > 11000                                            # the Hangul syllables alone are 11172
  for c in list(range(0, 0x3100)) + list(range(0x3100, 0x110000, 89)):
    if 0xD800 <= c <= 0xDFFF:
      continue
    s = 'A' + chr(c) + 'b'
    words = [''.join(chr(m) for m in w) for w in tf._words(table, s)]
    assert words == tc.basic_tokens(s.encode('utf-8')), hex(c)


def test_builder_refuses_duplicates_empty_and_ill_formed_tokens(tf):
  from mmt_amd import _lib
  with pytest.raises(_lib.MmtError, match='token 3 duplicates token 1'):
    tf.WordpieceVocab(['[UNK]', 'ab', '##ab', 'ab'])
  with pytest.raises(_lib.MmtError, match='token 2 is empty'):
    tf.WordpieceVocab(['[UNK]', 'ab', '', 'c'])
  with pytest.raises(_lib.MmtError, match='not well-formed'):
    tf.WordpieceVocab([b'[UNK]', b'a\xc0\x80'])
  with pytest.raises(ValueError, match='empty'):
    tf.WordpieceVocab([])
  v = tf.WordpieceVocab(['[UNK]', 'ab', '##ab', '##', '#', b'\xc3\xa9'])      # `##ab` and `ab` are different tokens
  assert len(v) == 6 and v.id('##ab') == 2 and v.id(b'\xc3\xa9') == 5 and v.id('é') == 5
  words = v.image.numpy().view(np.uint32)
  assert words[0] == 0x5650574D and words[1] == 6 and words[2] == 16 and words[3] == 8 + 4 * 16
  assert int((words[8:8 + 64:4] != 0).sum()) == 6
  with pytest.raises(KeyError):
    v.id('abc')


def test_vocab_file_round_trip(tf, tmp_path):
  path = tmp_path / 'vocab.txt'
  path.write_bytes('\n'.join(tc.vocab_tokens()).encode('utf-8') + b'\n')
  v = tf.WordpieceVocab(str(path))
  assert len(v) == len(tc.vocab_tokens()) and v.id('[SEP]') == tc.special_ids()[0]
  direct = tf.WordpieceVocab(list(tc.vocab_tokens()))
  assert torch.equal(v.image, direct.image) and torch.equal(v.codepoints, direct.codepoints)


def test_abi_refusals(tf, vocab):
  """Every refusal of mmt_text_tokens happens on the host, before any launch: host buffers stand in for device ones."""
  from mmt_amd import _lib
  L = _lib.lib()
  buf = np.zeros(64, dtype=np.int64)
  p = buf.ctypes.data
  ftok = (ctypes.c_int32 * 2)(5, 6)
  img, cps = vocab.image, vocab.codepoints
  base = dict(B=2, F=2, bytes=p, n=64, off=p, len=p, vocab=img.data_ptr(), vb=img.numel(), cp=cps.data_ptr(), cpn=cps.numel(),
              ftok=ftok, sep=3, unk=1, T=16, budget=13, ids=p, cnt=p, st=p, ws=p, wsb=1 << 20)

  def call(**kw):
    a = dict(base, **kw)
    return L.mmt_text_tokens(a['B'], a['F'], a['bytes'], a['n'], a['off'], a['len'], a['vocab'], a['vb'], a['cp'], a['cpn'], a['ftok'],
                             a['sep'], a['unk'], a['T'], a['budget'], a['ids'], a['cnt'], a['st'], a['ws'], a['wsb'], None)

  for kw, code, text in ((dict(B=0), -1, b'must be positive'), (dict(F=0), -1, b'must be positive'), (dict(T=0, budget=0), -1, b'must be positive'),
                         (dict(budget=14), -1, b'must fit T'), (dict(budget=-1), -1, b'must fit T'), (dict(F=17, T=64), -2, b'above 16 fields'),
                         (dict(bytes=None), -1, b'NULL argument'), (dict(off=None), -1, b'NULL'), (dict(len=None), -1, b'NULL'),
                         (dict(vocab=None), -1, b'NULL'), (dict(cp=None), -1, b'NULL'), (dict(ftok=None), -1, b'NULL'), (dict(ids=None), -1, b'NULL'),
                         (dict(cnt=None), -1, b'NULL'), (dict(st=None), -1, b'NULL'), (dict(n=-1), -1, b'bytes_len'),
                         (dict(vb=40), -1, b'no vocabulary image'), (dict(cpn=0x10FFFF), -1, b'codepoint_entries'),
                         (dict(sep=-1), -1, b'negative'), (dict(off=p + 4), -1, b'aligned'), (dict(len=p + 2), -1, b'aligned'),
                         (dict(ids=p + 1), -1, b'aligned'), (dict(ws=p + 2), -1, b'4-byte aligned'), (dict(ws=None), -3, b'bytes needed'),
                         (dict(wsb=2 * 2 * 14 * 4 - 1), -3, b'224 bytes needed')):
    assert call(**kw) == code, kw
    assert text in L.mmt_last_error(), (kw, L.mmt_last_error())
  assert L.mmt_text_tokens_workspace_bytes(2, 2, 13) == 2 * 2 * 14 * 4
  assert L.mmt_text_tokens_workspace_bytes(0, 2, 13) == 0 and L.mmt_text_tokens_workspace_bytes(2, 2, -1) == 0
  assert L.mmt_wordpiece_vocab_bytes(0, 0) == 0 and L.mmt_wordpiece_vocab_bytes(3, 2) == 0
  assert L.mmt_wordpiece_vocab_bytes(3, 10) == 32 + 8 * 16 + 12


def test_python_refusals(tf, vocab):
  one = [['ab'], ['c']]
  with pytest.raises(ValueError, match='WordpieceVocab'):
    tf.texts_to_token_features(None, one, ['[ATT]', '[REF]'], 16, 0)
  with pytest.raises(ValueError, match='no room'):
    tf.texts_to_token_features(vocab, one, ['[ATT]', '[REF]'], 8, 4)
  with pytest.raises(ValueError, match='no token'):
    tf.texts_to_token_features(vocab, one, ['[ATT]', '[NOPE]'], 16, 0)
  with pytest.raises(ValueError, match='field tokens'):
    tf.texts_to_token_features(vocab, one, [], 16, 0)
  with pytest.raises(ValueError, match='2 fields for 1 field tokens'):
    tf.texts_to_token_features(vocab, one, ['[ATT]'], 16, 0)
  with pytest.raises(ValueError, match='same number of examples'):
    tf.texts_to_token_features(vocab, [['ab'], ['c', 'd']], ['[ATT]', '[REF]'], 16, 0)
  with pytest.raises(ValueError, match='str or bytes'):
    tf.texts_to_token_features(vocab, [[3], ['c']], ['[ATT]', '[REF]'], 16, 0)
  ok = (torch.zeros(4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
  for bad, text in (((ok[0].int(), ok[1], ok[2]), 'uint8'), ((ok[0], ok[1].int(), ok[2]), 'int64'), ((ok[0], ok[1], ok[2].long()), 'int32'),
                    ((ok[0], ok[1][:1], ok[2][:1]), 'int64'), (ok[:2], 'tuple')):
    with pytest.raises(ValueError, match=text):
      tf.texts_to_token_features(vocab, bad, ['[ATT]', '[REF]'], 16, 0)
  # without [SEP] / [UNK] in the vocabulary
  with pytest.raises(ValueError, match='no token'):
    tf.texts_to_token_features(tf.WordpieceVocab(['a', 'b']), [['a']], [0], 16, 0)


def test_decode_text_features_hand_written_rows_and_whole_word_masking(tf, vocab):
  from mmt_amd import configs
  from mmt_amd import feature_pipeline as fp
  cfg = configs.MmtPretrainDataConfig()
  v = tc.vocab_dict()
  fields = {'caption_reference_description': ['Abcbc, ÉTÉ!', ''],
            'caption_attribution_description': ['kq 一ab', 'ab'], 'unused': ['z', 'z']}
  out = tf.decode_text_features(cfg, vocab, fields)
  T = 512 - 196 - 2
  assert out['text_token_ids'].shape == (2, T) and out['text_word_start'].shape == (2, T)
  row0 = [v['[ATT]'], v['[UNK]'], v['一'], v['ab'], v['[REF]'], v['abc'], v['##bc'], v[','], v['e'], v['##t'], v['##e'], v['!'], v['[SEP]']]
  start0 = [1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1]
  row1 = [v['[ATT]'], v['ab'], v['[REF]'], v['[SEP]']]
  ids = out['text_token_ids'].tolist()
  assert ids[0] == row0 + [0] * (T - len(row0)) and ids[1] == row1 + [0] * (T - len(row1))
  assert out['num_text_wordpieces'].tolist() == [len(row0), len(row1)]
  assert out['text_word_start'].int().tolist() == [start0 + [0] * (T - len(row0)), [1] * 4 + [0] * (T - 4)]
  with pytest.raises(ValueError, match='lacks'):
    tf.decode_text_features(cfg, vocab, {'caption_reference_description': ['a']})
  # a small config through the masking: whole words are masked together, field tokens and [SEP] never
  small = configs.MmtPretrainDataConfig(max_seq_len=40, image_size=32, patch_size=16)
  texts = {'caption_attribution_description': ['abcbc kkk ab abcde', 'kk ab, c'], 'caption_reference_description': ['abcbcd ab', 'tete']}
  feats = tf.decode_text_features(small, vocab, texts)
  B, P, Tt = 2, 4, 40 - 4 - 2
  assert feats['text_token_ids'].shape == (B, Tt)
  rng = np.random.default_rng(3)
  feats['patch_token_ids'] = torch.tensor([[v['[CLS]'], 9, 10, 11, 12, 13]] * B, dtype=torch.int32)
  feats['patch_embeddings'] = torch.from_numpy(rng.random((B, P, 12), dtype=np.float32))
  feats['unnormalized_patch_embeddings'] = feats['patch_embeddings'].clone()
  rnd = {'mlm_item_keys': rng.random((B, Tt), dtype=np.float32), 'mlm_value_u': np.zeros((B, Tt), dtype=np.float32),
         'mlm_random_ids': np.zeros((B, Tt), dtype=np.int32), 'mpp_item_keys': rng.random((B, 2 + P), dtype=np.float32),
         'mpp_value_u': rng.random((B, 2 + P), dtype=np.float32), 'mpp_random_ids': np.zeros((B, 2 + P), dtype=np.int32)}
  specials = [v[t] for t in ('[CLS]', '[SEP]', '[ATT]', '[REF]')]
  got = fp.make_mlm_and_mpp_features(feats, {k: torch.from_numpy(x) for k, x in rnd.items()}, max_seq_len=40, num_patches=P,
                                     patch_size=2, vocab_size=len(vocab), mask_token_id=v['[MASK]'], unselectable_ids=specials,
                                     mlm_fraction_to_mask=0.5, mlm_max_selections_per_seq=20, mpp_max_selections_per_seq=4)
  for b in range(B):
    n = int(feats['num_text_wordpieces'][b])
    before, after = feats['text_token_ids'][b, :n].tolist(), got['text_token_ids'][b, :n].tolist()
    starts = feats['text_word_start'][b, :n].tolist()
    word = np.cumsum(starts) - 1
    masked = [a == v['[MASK]'] for a in after]
    assert any(masked)
    for w in range(word[-1] + 1):
      members = [i for i in range(n) if word[i] == w]
      assert len({masked[i] for i in members}) == 1, (b, w)          # a word is masked whole or not at all
      if before[members[0]] in specials:
        assert not masked[members[0]]
    assert all(a == x or m for a, x, m in zip(after, before, masked))
