"""Text front end of the data layer's contract: the text half of the reference's `decode_fn`
(src/data/data_utils.py:241-278) -- BERT tokenisation of each UTF-8 text field, the round-robin trim to the text
budget, the field tokens and [SEP], the padding to max_seq_len - num_patches - 2, and the word starts whole-word
masking reads.  The definition is DESIGN.md section 4, "Text front end".

  WordpieceVocab             a vocab.txt (the data config's `vocab_filename`) as the two tables of include/mmt_layer.h:
                             the vocabulary image (built through the C ABI) and the code-point table (from unicodedata)
  texts_to_token_features    strings or packed bytes -> text_token_ids, num_text_wordpieces, text_word_start;
                             one mmt_text_tokens call on the GPU (csrc/text_tokens.hip), plain Python for CPU tensors
  decode_text_features       the same, driven by the data config (the counterpart of decode_image_features)

The outputs go into `make_mlm_and_mpp_features` and `RetrievalSets` unchanged."""
from __future__ import annotations

import ctypes
import functools
import json
import unicodedata
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np
import torch

CODEPOINTS = 0x110000
MAX_WORD_CHARS = 100          # max_input_chars_per_word
MAX_FIELDS = 16               # include/mmt_layer.h
_VALUE, _SOLO, _COUNT_SHIFT, _SPACE = 0x1FFFFF, 1 << 21, 22, 1 << 24

_CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
               (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))     # BERT's _is_chinese_char


def _is_punctuation(c: int, category: str) -> bool:
  return 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126 or category.startswith('P')


@functools.lru_cache(maxsize=None)
def codepoint_table() -> np.ndarray:
  """The code-point table of include/mmt_layer.h as uint32 [0x110000 + side entries], from this Python's unicodedata.
  Built once per process (a few seconds: it visits every code point)."""
  cat = unicodedata.category
  main = np.zeros(CODEPOINTS, dtype=np.uint32)
  side: List[int] = []
  cjk = np.zeros(CODEPOINTS, dtype=bool)
  for lo, hi in _CJK_RANGES:
    cjk[lo:hi + 1] = True
  for c in range(CODEPOINTS):
    if 0xD800 <= c <= 0xDFFF or c == 0 or c == 0xFFFD:
      continue                                              # surrogates never leave the decoder; dropped
    ch = chr(c)
    k = cat(ch)
    if c in (9, 10, 13) or k == 'Zs':
      main[c] = _SPACE
      continue
    if k in ('Cc', 'Cf'):
      continue
    if k in ('Cn', 'Co') and not cjk[c]:                    # unassigned, private use: themselves, inside a word
      main[c] = c | (1 << _COUNT_SHIFT)
      continue
    mapped = [ord(m) for m in unicodedata.normalize('NFD', ch.lower()) if cat(m) != 'Mn']
    if len(mapped) > 3:
      raise RuntimeError(f'U+{c:04X} maps to {len(mapped)} characters: the table format holds 3')
    flags = [_SOLO if cjk[c] or _is_punctuation(m, cat(chr(m))) else 0 for m in mapped]
    if len(mapped) == 1:
      main[c] = mapped[0] | flags[0] | (1 << _COUNT_SHIFT)
    elif mapped:
      main[c] = len(side) | (len(mapped) << _COUNT_SHIFT)
      side.extend(m | f for m, f in zip(mapped, flags))
  return np.concatenate([main, np.asarray(side, dtype=np.uint32)])


def _as_bytes(s, what: str) -> bytes:
  if isinstance(s, str):
    return s.encode('utf-8', 'surrogatepass')              # a lone surrogate becomes ill-formed bytes, which are dropped
  if isinstance(s, (bytes, bytearray, memoryview)):
    return bytes(s)
  raise ValueError(f'{what} must be str or bytes, got {type(s).__name__}')


class WordpieceVocab:
  """A WordPiece vocabulary ready for the device.  `tokens_or_path`: a sequence of tokens (str or bytes; ids are the
  positions) or the path of a vocab.txt with one token per line.  Empty, duplicated and ill-formed tokens are refused
  (by mmt_wordpiece_vocab_build).  `image` (uint8) and `codepoints` (int32) are the two tables; `.to(device)` returns a
  vocabulary with both on that device."""

  def __init__(self, tokens_or_path):
    if isinstance(tokens_or_path, (str, bytes)):
      with open(tokens_or_path, 'rb') as f:
        lines = f.read().split(b'\n')
      if lines and lines[-1].strip() == b'':
        lines.pop()
      tokens = [ln.strip() for ln in lines]
    else:
      tokens = [_as_bytes(t, 'a token') for t in tokens_or_path]
    if not tokens:
      raise ValueError('the vocabulary is empty')
    from . import _lib
    L = _lib.lib()
    blob = b''.join(tokens)
    offsets = np.zeros(len(tokens) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in tokens], out=offsets[1:])
    need = L.mmt_wordpiece_vocab_bytes(len(tokens), max(len(blob), len(tokens)))
    if need == 0:
      raise ValueError(f'a vocabulary of {len(tokens)} tokens in {len(blob)} bytes is out of range')
    image = np.zeros(need // 4, dtype=np.uint32)
    src = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, dtype=np.uint8)
    _lib.check(L.mmt_wordpiece_vocab_build(len(tokens), src.ctypes.data_as(ctypes.c_void_p),
                                           offsets.ctypes.data_as(ctypes.c_void_p),
                                           image.ctypes.data_as(ctypes.c_void_p), need))
    self.tokens: List[bytes] = tokens
    self._ids: Dict[bytes, int] = {t: i for i, t in enumerate(tokens)}
    self.image = torch.from_numpy(image.view(np.uint8))
    self.codepoints = torch.from_numpy(codepoint_table().view(np.int32))

  def __len__(self) -> int:
    return len(self.tokens)

  @property
  def device(self) -> torch.device:
    return self.image.device

  def id(self, token) -> int:
    """The id of a token (str or bytes); KeyError when the vocabulary does not hold it."""
    return self._ids[_as_bytes(token, 'token')]

  def to(self, device) -> 'WordpieceVocab':
    other = object.__new__(WordpieceVocab)
    other.tokens, other._ids = self.tokens, self._ids
    other.image, other.codepoints = self.image.to(device), self.codepoints.to(device)
    return other


# ---------------------------------------------------------------------------------------------------
# The plain-Python path (CPU tensors): the same definition, read off the same code-point table.
# ---------------------------------------------------------------------------------------------------
def _decode(data: bytes) -> str:
  """Characters of the well-formed sequences; every other byte dropped (the replacement characters Python puts in their
  place are dropped by the table, as a genuine U+FFFD is)."""
  return data.decode('utf-8', 'replace')


def _words(table: np.ndarray, text: str) -> List[List[int]]:
  words: List[List[int]] = []
  cur: List[int] = []
  for ch in text:
    e = int(table[ord(ch)])
    n = (e >> _COUNT_SHIFT) & 3
    if n == 0:
      if e & _SPACE and cur:
        words.append(cur)
        cur = []
      continue
    entries = [e] if n == 1 else [int(table[CODEPOINTS + (e & _VALUE) + j]) for j in range(n)]
    for m in entries:
      if m & _SOLO:
        if cur:
          words.append(cur)
          cur = []
        words.append([m & _VALUE])
      else:
        cur.append(m & _VALUE)
  if cur:
    words.append(cur)
  return words


def _wordpiece(ids: Dict[bytes, int], word: List[int], unk: int) -> List[int]:
  if len(word) > MAX_WORD_CHARS:
    return [unk]
  enc = [chr(c).encode('utf-8') for c in word]
  out, s = [], 0
  while s < len(word):
    for e in range(len(word), s, -1):
      hit = ids.get((b'##' if s else b'') + b''.join(enc[s:e]))
      if hit is not None:
        break
    else:
      return [unk]
    out.append(hit)
    s = e
  return out


def _field_pieces(vocab: WordpieceVocab, table: np.ndarray, data: bytes, limit: int, unk: int) -> List[Tuple[int, int]]:
  """(id, first piece of its word) of the field's first `limit` wordpieces."""
  out: List[Tuple[int, int]] = []
  for word in _words(table, _decode(data)):
    if len(out) >= limit:
      break
    out.extend((p, int(i == 0)) for i, p in enumerate(_wordpiece(vocab._ids, word, unk)))
  return out[:limit]


def _rows_cpu(vocab, data: bytes, offsets, lengths, B, F, field_ids, sep, unk, T, budget):
  table = vocab.codepoints.numpy().view(np.uint32)
  ids = torch.zeros(B, T, dtype=torch.int32)
  start = torch.zeros(B, T, dtype=torch.bool)
  count = torch.zeros(B, dtype=torch.int32)
  for b in range(B):
    pieces = []
    for f in range(F):
      o = min(max(int(offsets[b * F + f]), 0), len(data))
      n = min(max(int(lengths[b * F + f]), 0), len(data) - o)
      pieces.append(_field_pieces(vocab, table, data[o:o + n], budget, unk))
    take, rem, r = [0] * F, budget, 0
    while rem > 0 and any(len(p) > r for p in pieces):       # round r: each field in order takes its r-th piece
      for f in range(F):
        if len(pieces[f]) > r and rem > 0:
          take[f] += 1
          rem -= 1
      r += 1
    row = []
    for f in range(F):
      row.append((field_ids[f], 1))
      row.extend(pieces[f][:take[f]])
    row.append((sep, 1))
    count[b] = len(row)
    ids[b, :len(row)] = torch.tensor([p[0] for p in row], dtype=torch.int32)
    start[b, :len(row)] = torch.tensor([bool(p[1]) for p in row])
  return ids, count, start


def _pack_fields(fields, device):
  F = len(fields)
  if F < 1 or any(not isinstance(col, (list, tuple)) for col in fields):
    raise ValueError('fields must be a list of F lists of B strings, or a packed (bytes, offsets, lengths) tuple')
  B = len(fields[0])
  if B < 1 or any(len(col) != B for col in fields):
    raise ValueError('every field needs the same number of examples, at least one')
  chunks, offs, lens, n = [], [], [], 0
  for b in range(B):
    for f in range(F):
      raw = _as_bytes(fields[f][b], f'fields[{f}][{b}]')
      chunks.append(raw); offs.append(n); lens.append(len(raw))
      n += len(raw)
  blob = b''.join(chunks) or b'\0'                           # a buffer of at least one byte, whatever the fields hold
  data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy())
  return (data.to(device), torch.tensor(offs, dtype=torch.int64).to(device),
          torch.tensor(lens, dtype=torch.int32).to(device)), B


def texts_to_token_features(vocab: WordpieceVocab, fields, field_tokens: Sequence[Union[str, bytes, int]],
                            max_seq_len: int, num_patches: int) -> Dict[str, torch.Tensor]:
  """The text half of `decode_fn` for a batch.

  fields: a list of F lists of B str / bytes (packed here and moved to the vocabulary's device), or an already packed
  (bytes uint8 [n], offsets int64 [B*F], lengths int32 [B*F]) tuple on the vocabulary's device: field f of example b is
  lengths[b*F + f] bytes from bytes[offsets[b*F + f]].  field_tokens: the F special tokens in front of the fields
  (tokens of the vocabulary, or ids).  With T = max_seq_len - num_patches - 2 and budget = T - F - 1 the row is
  tok_0 pieces_0 ... [SEP] padded with 0 to T, the fields sharing the budget round-robin.
  Returns text_token_ids int32 [B, T], num_text_wordpieces int32 [B] and text_word_start bool [B, T] (true on the field
  tokens, [SEP] and the first piece of every word).  On the GPU this is one mmt_text_tokens call; CPU tensors go
  through plain Python of the same definition."""
  if not isinstance(vocab, WordpieceVocab):
    raise ValueError('vocab must be a WordpieceVocab')
  F = len(field_tokens)
  if F < 1 or F > MAX_FIELDS:
    raise ValueError(f'between 1 and {MAX_FIELDS} field tokens are needed, got {F}')
  T = int(max_seq_len) - int(num_patches) - 2
  budget = T - F - 1
  if int(num_patches) < 0 or budget < 0:
    raise ValueError(f'max_seq_len {max_seq_len} leaves no room for {F} field tokens and [SEP] behind {num_patches} patches')
  try:
    field_ids = [int(t) if isinstance(t, int) else vocab.id(t) for t in field_tokens]
    sep, unk = vocab.id('[SEP]'), vocab.id('[UNK]')
  except KeyError as e:
    raise ValueError(f'the vocabulary has no token {e.args[0]!r}') from None
  if any(i < 0 for i in field_ids):
    raise ValueError('field token ids must not be negative')
  dev = vocab.device
  if isinstance(fields, tuple):
    if len(fields) != 3:
      raise ValueError('packed fields are a (bytes, offsets, lengths) tuple')
    data, offsets, lengths = fields
    if data.dtype != torch.uint8 or data.dim() != 1:
      raise ValueError('bytes must be a 1-D uint8 tensor')
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < F or offsets.numel() % F:
      raise ValueError('offsets must be int64 [B*F], B >= 1')
    if lengths.dtype != torch.int32 or lengths.shape != offsets.shape:
      raise ValueError('lengths must be int32 [B*F]')
    if any(t.device != dev for t in (data, offsets, lengths)):
      raise ValueError('bytes, offsets and lengths must live on the vocabulary\'s device')
    B = offsets.numel() // F
    data, offsets, lengths = data.contiguous(), offsets.contiguous(), lengths.contiguous()
  else:
    if len(fields) != F:
      raise ValueError(f'{len(fields)} fields for {F} field tokens')
    (data, offsets, lengths), B = _pack_fields(list(fields), dev)
  if dev.type == 'cuda':
    from . import _lib
    L = _lib.lib()
    ids = torch.empty(B, T, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    start = torch.empty(B, T, dtype=torch.uint8, device=dev)
    need = L.mmt_text_tokens_workspace_bytes(B, F, budget)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    ftok = (ctypes.c_int32 * F)(*field_ids)
    _lib.check(L.mmt_text_tokens(B, F, data.data_ptr() if data.numel() else ws.data_ptr(), data.numel(), offsets.data_ptr(),
                                 lengths.data_ptr(), vocab.image.data_ptr(), vocab.image.numel(), vocab.codepoints.data_ptr(),
                                 vocab.codepoints.numel(), ftok, sep, unk, T, budget, ids.data_ptr(), count.data_ptr(),
                                 start.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream))
    start = start.bool()
  else:
    ids, count, start = _rows_cpu(vocab, data.numpy().tobytes(), offsets.tolist(), lengths.tolist(), B, F, field_ids,
                                  sep, unk, T, budget)
  return {'text_token_ids': ids, 'num_text_wordpieces': count, 'text_word_start': start}


def decode_text_features(data_config, vocab: WordpieceVocab, fields) -> Dict[str, torch.Tensor]:
  """The text half of `decode_fn` as the data config drives it: the fields and their special tokens come from
  `text_special_token_field_dict` (in its order), the row length from `max_seq_len`, `image_size` and `patch_size`.
  fields: a dict {field name: list of B str / bytes}, or what `texts_to_token_features` takes (in the dict's order)."""
  spec = json.loads(data_config.text_special_token_field_dict)
  if not isinstance(spec, dict) or not spec:
    raise ValueError('text_special_token_field_dict must name at least one field')
  if isinstance(fields, dict):
    missing = [k for k in spec if k not in fields]
    if missing:
      raise ValueError(f'fields lacks {missing}')
    fields = [list(fields[k]) for k in spec]
  num_patches = (int(data_config.image_size) // int(data_config.patch_size)) ** 2
  return texts_to_token_features(vocab, fields, list(spec.values()), int(data_config.max_seq_len), num_patches)
