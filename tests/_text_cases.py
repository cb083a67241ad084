"""Text front end: the oracle, the synthetic vocabulary, the corpus and the packing helper of tests/test_text_frontend.py
(CPU) and tests/test_gpu_text_frontend.py (GPU).

The oracle restates DESIGN.md section 4, "Text front end", the way original BERT's tokenization.py is written: whole
strings through stages (clean, space out CJK, split on spaces, lower, NFD without Mn, split on punctuation, WordPiece),
with unicodedata and nothing else -- no tables, no code of mmt_amd.  Lower-casing is per code point, as the definition
says.  Where the `tokenizers` package is installed, test_text_frontend.py checks this oracle against it on the corpus."""
import functools
import string
import unicodedata as ud

import numpy as np

SEED = 20213
SENTINEL, GUARD = 0xA5, 64
MAX_WORD_CHARS = 100
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
              (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
THAI = 'ก'                      # a 3-byte letter without case or decomposition
CJK_CORPUS = [chr(0x4E00 + i) for i in range(65)]
HANGUL_CORPUS = [chr(0xAC00 + 171 * i) for i in range(65)]


# ---------------------------------------------------------------------------------------------------
# The oracle
# ---------------------------------------------------------------------------------------------------
def is_cjk(c):
  return any(lo <= c <= hi for lo, hi in CJK_RANGES)


def is_punct(ch):
  c = ord(ch)
  return 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126 or ud.category(ch).startswith('P')


def basic_tokens(data: bytes):
  """BERT's BasicTokenizer(do_lower_case=True) on the field's bytes: the list of words (strings of mapped characters)."""
  text = data.decode('utf-8', 'replace')
  cleaned = []
  for ch in text:
    space = ch in '\t\n\r' or ud.category(ch) == 'Zs'
    if ord(ch) == 0 or ord(ch) == 0xFFFD or (not space and ud.category(ch) in ('Cc', 'Cf')):
      continue
    cleaned.append(' ' if space else ch)
  spaced = ''.join(f' {ch} ' if is_cjk(ord(ch)) else ch for ch in cleaned)
  words = []
  for tok in spaced.split(' '):
    tok = ''.join(ch.lower() for ch in tok)
    tok = ''.join(ch for ch in ud.normalize('NFD', tok) if ud.category(ch) != 'Mn')
    cur = ''
    for ch in tok:
      if is_punct(ch):
        if cur:
          words.append(cur)
        words.append(ch)
        cur = ''
      else:
        cur += ch
    if cur:
      words.append(cur)
  return words


def wordpiece(vocab: dict, word: str, unk: int):
  if len(word) > MAX_WORD_CHARS:
    return [unk]
  out, start = [], 0
  while start < len(word):
    end = len(word)
    while end > start:
      piece = ('##' if start else '') + word[start:end]
      if piece in vocab:
        break
      end -= 1
    if end == start:
      return [unk]
    out.append(vocab[piece])
    start = end
  return out


def field_pieces(vocab: dict, data: bytes, unk: int):
  """[(id, first piece of its word)] of the whole field."""
  out = []
  for word in basic_tokens(data):
    out.extend((p, int(i == 0)) for i, p in enumerate(wordpiece(vocab, word, unk)))
  return out


def expected_rows(vocab: dict, examples, field_ids, sep, unk, T, budget):
  """examples: B lists of F byte strings.  Returns (ids int32 [B,T], count int32 [B], word_start uint8 [B,T])."""
  B, F = len(examples), len(field_ids)
  ids = np.zeros((B, T), dtype=np.int32)
  start = np.zeros((B, T), dtype=np.uint8)
  count = np.zeros(B, dtype=np.int32)
  for b, ex in enumerate(examples):
    pieces = [field_pieces(vocab, data, unk) for data in ex]
    kept, left, r = [[] for _ in range(F)], budget, 0
    while left > 0 and any(len(p) > r for p in pieces):
      for f in range(F):
        if len(pieces[f]) > r and left > 0:
          kept[f].append(pieces[f][r])
          left -= 1
      r += 1
    row = []
    for f in range(F):
      row += [(field_ids[f], 1)] + kept[f]
    row.append((sep, 1))
    assert len(row) <= T
    count[b] = len(row)
    ids[b, :len(row)] = [p[0] for p in row]
    start[b, :len(row)] = [p[1] for p in row]
  return ids, count, start


# ---------------------------------------------------------------------------------------------------
# The vocabulary (synthetic, > 1000 tokens) and the corpus
# ---------------------------------------------------------------------------------------------------
SPECIALS = ['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]', '[ATT]', '[REF]', '[ALT]']
MISSING_LETTERS = 'qx'               # neither as a word nor as a `##` piece: words with them become [UNK]
MISSING_PUNCT = '~^'


@functools.lru_cache(maxsize=None)
def vocab_tokens():
  rng = np.random.default_rng(SEED)
  toks = list(SPECIALS)
  toks += [c for c in string.punctuation if c not in MISSING_PUNCT]
  letters = [c for c in string.ascii_lowercase if c not in MISSING_LETTERS]
  toks += letters + ['##' + c for c in letters] + list(string.digits) + ['##' + d for d in string.digits]
  toks += ['ab', 'abc', '##bc', '##bcd', 'abcde']                                      # prefix chains: the longest must win
  toks += ['m' * n for n in (63, 64, 65, 100)] + ['##' + 'm' * 64]
  toks += [THAI, '##' + THAI, THAI * 64, THAI * 100, '##' + THAI * 65]
  greek = [chr(c) for c in range(0x3B1, 0x3CA)]
  cyr = [chr(c) for c in range(0x430, 0x450)]
  toks += greek[:-3] + ['##' + g for g in greek[:-5]] + cyr[:-4] + ['##' + c for c in cyr[:-6]]
  toks += ['αβ', '##βγ', 'да', '##нет']
  toks += ['ß', '##ß', 'æ', '##æ', 'ø', 'ð', 'þ', 'ı', '##ı', 'ł', 'đ', 'été']
  toks += CJK_CORPUS[:49]
  toks += [ud.normalize('NFD', h) for h in HANGUL_CORPUS[:40]] + ['ᄀ', '##ᅡ', '##ᆨ']
  toks += [chr(c) for c in range(0x2010, 0x2021)] + ['、', '。', '¡', '¿', '«']
  toks += ['\U0001f600', '##\U0001f600']                                                 # a 4-byte character
  seen = set(toks)
  pool = 'abcdefghiklnoprstuvw'
  while len(toks) < 1100:
    w = ''.join(pool[i] for i in rng.integers(0, len(pool), size=int(rng.integers(2, 7))))
    w = ('##' + w) if rng.random() < 0.5 else w
    if w not in seen:
      seen.add(w)
      toks.append(w)
  assert len(toks) == len(set(toks)) >= 1000
  return tuple(toks)


@functools.lru_cache(maxsize=None)
def vocab_dict():
  return {t: i for i, t in enumerate(vocab_tokens())}


def special_ids():
  v = vocab_dict()
  return v['[SEP]'], v['[UNK]']


CORPUS_RANGES = (
    [chr(c) for c in range(0x00, 0x80)],                                                    # ASCII
    [chr(c) for c in range(0x80, 0x180) if c not in (0xAD, 0x130)],                         # Latin-1, Latin Extended-A
    [chr(c) for c in list(range(0x386, 0x38B)) + list(range(0x391, 0x3A2)) + list(range(0x3A4, 0x3AA)) + list(range(0x3AC, 0x3CF))],   # Greek, no U+03A3
    [chr(c) for c in range(0x400, 0x460)],                                                  # Cyrillic
    [chr(c) for c in range(0x300, 0x310)],                                                  # combining marks
    [chr(c) for c in range(0x2010, 0x2028)],                                                # general punctuation
    [chr(c) for c in range(0x3000, 0x3003)],                                                # ideographic space, comma, full stop
    CJK_CORPUS, HANGUL_CORPUS)


@functools.lru_cache(maxsize=None)
def corpus(n=2000):
  """n strings: words mostly glued from the vocabulary's own pieces (random case, a combining mark now and then), the
  rest random characters of CORPUS_RANGES; spaces, tabs, ideographic spaces or nothing between them."""
  rng = np.random.default_rng(SEED + 1)
  pieces = [t[2:] if t.startswith('##') and len(t) > 2 else t for t in vocab_tokens() if t not in SPECIALS and len(t) < 12]
  flat = [ch for r in CORPUS_RANGES for ch in r]
  out = []
  for _ in range(n):
    parts = []
    for _ in range(int(rng.integers(0, 13))):
      if rng.random() < 0.75:
        w = ''.join(pieces[int(i)] for i in rng.integers(0, len(pieces), size=int(rng.integers(1, 4))))
        w = ''.join(ch.upper() if rng.random() < 0.2 and len(ch.upper()) == 1 and ch.upper() != 'Σ' else ch for ch in w)
        if rng.random() < 0.2:
          k = int(rng.integers(0, len(w))) + 1
          w = w[:k] + chr(0x300 + int(rng.integers(0, 16))) + w[k:]
      else:
        group = CORPUS_RANGES[int(rng.integers(0, len(CORPUS_RANGES)))] if rng.random() < 0.7 else flat
        w = ''.join(group[int(i)] for i in rng.integers(0, len(group), size=int(rng.integers(1, 9))))
      parts.append(w)
      parts.append((' ', ' ', ' ', '\t', '　', '', '  ')[int(rng.integers(0, 7))])
    out.append(''.join(parts))
  return tuple(out)


# ---------------------------------------------------------------------------------------------------
# Packing for the ctypes calls: strings at odd offsets, sentinel bytes between them, a guard behind
# ---------------------------------------------------------------------------------------------------
def pack(examples, gap=3):
  """examples: B lists of F byte strings -> (bytes uint8 [n + GUARD], offsets int64 [B*F], lengths int32 [B*F], n).  Every
  field starts at an odd offset behind `gap` or `gap + 1` sentinel bytes; 0xA5 is a lone continuation byte, so a read
  outside a field would not pass unnoticed either."""
  chunks, offs, lens, n = [], [], [], 0
  for ex in examples:
    for data in ex:
      pad = gap if (n + gap) % 2 == 1 else gap + 1
      chunks.append(bytes([SENTINEL]) * pad)
      n += pad
      offs.append(n); lens.append(len(data))
      chunks.append(data)
      n += len(data)
  chunks.append(bytes([SENTINEL]) * GUARD)
  blob = np.frombuffer(b''.join(chunks), dtype=np.uint8).copy()
  return blob, np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int32), n


def enc(s):
  return s.encode('utf-8') if isinstance(s, str) else bytes(s)


ILL_FORMED = (b'\xc3', b'\xe2\x82', b'\xf0\x9f\x98', b'\xc0\x80', b'\xed\xa0\x80', b'\xf4\x90\x80\x80', b'\x80', b'\xbf\xbf',
              b'\xe0\x9f\x80', b'\xf0\x8f\x80\x80', b'\xf5\x80\x80\x80', b'\xff', b'\xfe')


@functools.lru_cache(maxsize=None)
def shape_cases():
  """name -> (examples, F, T, budget): the shapes of the issue, the smallest at which the kernel can go wrong."""
  m, k, t = 'm', 'k', THAI
  cases = {}
  lengths = (1, 63, 64, 65, 100, 101)
  cases['word_lengths_ascii'] = ([[enc(m * n)] for n in lengths] + [[enc(k * n)] for n in lengths], 1, 128, 126)
  cases['word_lengths_3byte'] = ([[enc(t * n)] for n in lengths] + [[enc(t * 66 + ' ' + t * 99)]], 1, 128, 126)
  cases['hundred_pieces_then_a_word'] = ([[enc(k * 100 + ' ab')], [enc(t * 100 + ' ' + k * 101 + ' abc')]], 1, 128, 126)
  cases['fails_at_the_last_character'] = ([[enc('abcbkq ab abcdeq. abcde')], [enc('kkkkkkx' + t + ' ' + t + 'q ' + t)]], 1, 16, 14)
  cases['prefix_chains'] = ([[enc('a ab abc abcd abcde abcbc abcbcd abbcd ABĆD')]], 1, 64, 62)
  ill = b''.join(ILL_FORMED)
  for F in (1, 2, 3):
    ex = [[enc('ab c')] * F, [b''] * F, [b' \t\n\r\xc2\xa0\xe3\x80\x80   '] + [b''] * (F - 1), [ill] * F,
          [b'ab' + ILL_FORMED[0] + b'c ' + ILL_FORMED[4] + b' d' + ILL_FORMED[3] + b'e\xe2\x82'] + [enc('k')] * (F - 1),
          ([enc('abc'), b'', enc('kk')])[:F], [enc('[SEP] [unk]')] * F, [enc('一丁k丂 가丿')] * F]
    cases[f'fields_{F}'] = (ex, F, 16, 16 - F - 1)
  words = ' '.join(['ab'] * 10)
  cases['trim'] = ([[enc(' '.join(['ab'] * 6)), enc(' '.join(['k'] * 6))], [enc(' '.join(['ab'] * 7)), enc(' '.join(['k'] * 6))],
                    [enc(words), enc('k')], [enc('k'), enc(words)], [enc('ab ab ab ab ab kkkkkkkkkk'), enc('c c c c')],
                    [enc('kkkkkkkkkkkkkkkk'), b'']], 2, 15, 12)
  cases['budget_zero'] = ([[enc('ab c'), enc('k')], [b'', b'']], 2, 3, 0)
  long_text = ' '.join(['abcbk', t * 3, 'ab,', 'kq', '一'] * 900).encode('utf-8')
  assert len(long_text) > 20000
  spaces = b' ' * 20000 + b'abc'
  cases['long_fields'] = ([[long_text, spaces], [spaces, long_text]], 2, 64, 61)
  cases['long_fields_b1'] = ([[spaces]], 1, 16, 14)
  cases['long_word_over_chunks'] = ([[b' ' * 200 + enc(m * 100) + b' ' + enc(k * 300) + b' ab ' + enc(m * 64 + k)],
                                     [b'k' * 250 + enc(t * 4) + b' ab'] ] , 1, 64, 62)
  return cases
