"""Cases of `feature_pipeline.random_item_masking` for the one-launch route (`mmt_item_masking`): inputs as numpy arrays,
shared by tests/test_item_masking_host.py (the host variant on CPU tensors) and tests/test_gpu_item_masking.py (the
kernel).  The yardstick is always `kernel=False`, the torch ops of the same call on the same device; every output must be
equal bit for bit, dtype included."""
import numpy as np
import torch

UNSEL = [101, 102, 103, 1]                  # [CLS] [SEP] [PATCH]-like ids
MASK = 104
VOCAB = 3000
SIZES = (1, 2, 63, 64, 65, 257, 1000)
WORD_MODES = ('every-token', 'whole-word', 'no-start-at-0')
NAMES = ('OUT masked', 'positions', 'n_masked', 'labels')


def base_case(T, mode, seed, B=5, unsel_rate=0.05, lengths=None):
  """B rows: n_tokens 0, T, and ragged lengths between (or `lengths`); behind n_tokens the row holds word starts and
  unselectable ids that must not count."""
  rng = np.random.default_rng(seed)
  n = np.array(([0, T] + [int(rng.integers(1, T + 1)) for _ in range(B)])[:B], np.int64)
  if lengths is not None:
    n = np.array(lengths, np.int64)
    B = len(n)
  tok = rng.integers(1000, VOCAB, (B, T)).astype(np.int32)
  tok[rng.random((B, T)) < unsel_rate] = UNSEL[1]
  ws = rng.random((B, T)) < 0.6
  ws[:, 0] = mode != 'no-start-at-0'
  for b in range(B):
    tok[b, n[b]:] = UNSEL[int(rng.integers(0, len(UNSEL)))]      # garbage in the padding
    ws[b, n[b]:] = True
  ins = dict(token_ids=tok, n_tokens=n, item_keys=rng.random((B, T), dtype=np.float32), value_u=rng.random((B, T), dtype=np.float32),
             random_ids=rng.integers(0, VOCAB, (B, T)).astype(np.int32), word_start=None if mode == 'every-token' else ws)
  kw = dict(selection_rate=0.15, max_selections=max(1, T // 4), unselectable_ids=list(UNSEL), mask_token_id=MASK)
  return ins, kw


def _thresholds():
  f = np.float32
  m, r = f(0.8), f(0.8 + 0.1)                # what torch compares with: the Python numbers rounded once
  vals = [m, np.nextafter(m, f(0)), np.nextafter(m, f(1)), r, np.nextafter(r, f(0)), np.nextafter(r, f(1)), f(0.8) + f(0.1), f(0), f(1),
          f(0.9), f('nan')]
  return np.array(vals, np.float32)


def variants(T, mode, seed):
  """(name, inputs, keyword arguments) for every corner of the list at this size."""
  out = []
  ins, kw = base_case(T, mode, seed)
  out.append(('plain', ins, kw))
  ins, kw = base_case(T, mode, seed + 1)
  ins['item_keys'] = (np.random.default_rng(seed).integers(0, 4, ins['item_keys'].shape) / 4).astype(np.float32)
  out.append(('ties', ins, dict(kw, selection_rate=0.5, max_selections=T)))
  ins, kw = base_case(T, mode, seed + 2)
  k = ins['item_keys']
  rng = np.random.default_rng(seed + 2)
  special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 0.25], np.float32)
  pick = rng.random(k.shape) < 0.7
  k[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
  out.append(('inf-nan-zero', ins, dict(kw, selection_rate=0.6, max_selections=T)))
  out.append(('inf-nan-zero-all', ins, dict(kw, selection_rate=1.0, max_selections=T + 5)))
  ins, kw = base_case(T, mode, seed + 3)
  ins['token_ids'][:] = UNSEL[0]
  out.append(('all-unselectable', ins, dict(kw, selection_rate=1.0)))
  ins, kw = base_case(T, mode, seed + 4, unsel_rate=0.0)
  th = _thresholds()
  ins['value_u'] = th[np.random.default_rng(seed).integers(0, len(th), ins['value_u'].shape)]
  out.append(('thresholds', ins, dict(kw, selection_rate=1.0, max_selections=T)))
  for rate in (0.0, 1.0):
    ins, kw = base_case(T, mode, seed + 5)
    out.append((f'rate-{rate}', ins, dict(kw, selection_rate=rate, max_selections=T)))
    out.append((f'value-rates-{rate}', ins, dict(kw, selection_rate=0.5, max_selections=T, mask_token_rate=rate, random_token_rate=1.0 - rate)))
  ins, kw = base_case(T, mode, seed + 6)
  out.append(('max-below', ins, dict(kw, selection_rate=0.5, max_selections=max(0, T // 8))))
  out.append(('max-above', ins, dict(kw, selection_rate=0.5, max_selections=T + 3)))
  out.append(('max-zero', ins, dict(kw, selection_rate=0.5, max_selections=0)))
  return out


def rounding_case():
  """selection_rate 0.15 at 20 selectable items: the float32 product decides between 3 and 4; beside it the counts around it."""
  T = 24
  rng = np.random.default_rng(11)
  n = np.array([20, 19, 21, 7, 24], np.int64)
  tok = rng.integers(1000, VOCAB, (5, T)).astype(np.int32)
  ins = dict(token_ids=tok, n_tokens=n, item_keys=rng.random((5, T), dtype=np.float32), value_u=rng.random((5, T), dtype=np.float32),
             random_ids=rng.integers(0, VOCAB, (5, T)).astype(np.int32), word_start=None)
  return ins, dict(selection_rate=0.15, max_selections=T, unselectable_ids=list(UNSEL), mask_token_id=MASK)


def run(ins, kw, device, kernel):
  from mmt_amd import feature_pipeline as fp
  t = {k: None if v is None else torch.from_numpy(v).to(device) for k, v in ins.items()}
  return fp.random_item_masking(t.pop('token_ids'), t.pop('n_tokens'), kernel=kernel, **t, **kw)


def assert_same(ins, kw, device, what=''):
  """kernel=True against kernel=False, every output, bit for bit; returns the kernel's outputs."""
  want = run(ins, kw, device, False)
  got = run(ins, kw, device, True)
  for name, w, g in zip(NAMES, want, got):
    assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (what, name, g.dtype, w.dtype)
    if not torch.equal(g, w):
      bad = (g != w).nonzero()[:4].tolist()
      raise AssertionError(f'{what}: {name} differs at {bad}')
  return got


# ---- make_mlm_and_mpp_features with the switch either way ----------------------------------------------------------------
CLS, SEP, PATCH, ATT, MASKID, FVOCAB = 101, 102, 5, 6, 103, 2000


def _feature_case(rng, B, P, T, S, whole_word, rates):
  """The kind of batch tests/test_feature_pipeline.py builds: [CLS] [PATCH] patch tokens, ragged text with unselectable
  ids at both ends and in the middle, a tie among the keys."""
  n_patch, E = P * P, 12
  n_text = rng.integers(3, T + 1, B)
  feats = {'patch_token_ids': np.tile(np.concatenate([[CLS, PATCH], 104 + np.arange(n_patch)]).astype(np.int32), (B, 1)),
           'text_token_ids': np.zeros((B, T), np.int32), 'num_text_wordpieces': n_text.astype(np.int32),
           'patch_embeddings': rng.standard_normal((B, n_patch, E)).astype(np.float32),
           'unnormalized_patch_embeddings': rng.random((B, n_patch, E), dtype=np.float32)}
  ws = np.zeros((B, T), bool)
  for b in range(B):
    t = rng.integers(1000, FVOCAB, n_text[b]).astype(np.int32)
    t[0], t[-1] = ATT, SEP
    if n_text[b] > 6:
      t[4] = SEP
    feats['text_token_ids'][b, :n_text[b]] = t
    ws[b, :n_text[b]] = rng.random(n_text[b]) < 0.6
    ws[b, 0] = True
  if whole_word:
    feats['text_word_start'] = ws
  rnd = {'mlm_item_keys': rng.random((B, T), dtype=np.float32), 'mlm_value_u': rng.random((B, T), dtype=np.float32),
         'mlm_random_ids': rng.integers(0, FVOCAB, (B, T)).astype(np.int32),
         'mpp_item_keys': rng.random((B, 2 + n_patch), dtype=np.float32), 'mpp_value_u': rng.random((B, 2 + n_patch), dtype=np.float32),
         'mpp_random_ids': rng.integers(0, FVOCAB, (B, 2 + n_patch)).astype(np.int32)}
  rnd['mlm_item_keys'][:, 3] = rnd['mlm_item_keys'][:, 1]
  kw = dict(max_seq_len=S, num_patches=n_patch, patch_size=2, vocab_size=FVOCAB, mask_token_id=MASKID,
            unselectable_ids=[CLS, SEP, PATCH, ATT], mlm_fraction_to_mask=rates[0], mpp_fraction_to_mask=rates[1],
            mlm_max_selections_per_seq=rates[2], mpp_max_selections_per_seq=rates[3])
  return feats, rnd, kw


FEATURE_CASES = [dict(B=5, P=4, T=20, S=2 + 16 + 24, whole_word=False, rates=(0.15, 0.5, 20, 6)),
                 dict(B=4, P=3, T=30, S=2 + 9 + 30, whole_word=True, rates=(0.3, 0.5, 41, 5)),
                 dict(B=3, P=3, T=12, S=2 + 9 + 12, whole_word=False, rates=(1.0, 1.0, 3, 2))]


def feature_outputs(device, switch):
  from mmt_amd import feature_pipeline as fp
  rng = np.random.default_rng(3)
  outs = []
  for c in FEATURE_CASES:
    feats, rnd, kw = _feature_case(rng, **c)
    outs.append(fp.make_mlm_and_mpp_features({k: torch.from_numpy(v).to(device) for k, v in feats.items()},
                                             {k: torch.from_numpy(v).to(device) for k, v in rnd.items()}, masking_kernel=switch, **kw))
  return outs


def assert_feature_outputs_equal(a, b):
  for x, y in zip(a, b):
    assert x.keys() == y.keys()
    for k in x:
      assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k
