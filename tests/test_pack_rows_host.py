"""Row packing on the host (`mmt_pack_rows_host`, include/mmt_layer.h): the functions the kernels run, as loops, against
the ten-line next-fit of tests/_pack_cases.py plus `packed_example_layout`, bit for bit, inside guarded buffers; every
refusal with its message; `fused.pack_rows` and `input_utils.pack_batch` on CPU tensors; the sanitizer program."""
import ctypes
import os

import pytest
import torch

from tests import _pack_cases as PC


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  return _lib.lib()


@pytest.mark.parametrize('tables', [True, False], ids=['tables', 'no-tables'])
@pytest.mark.parametrize('name', list(PC.CASES))
def test_host_variant_equals_next_fit_and_layout_bitwise(lib, name, tables):
  consumed = PC.check_case(name, tables, 'cpu')
  E = len(PC.CASES[name]['lengths'])
  if name in ('stop-at-row-R', 'stop-at-E-max', 'row-filled-exactly'):
    assert consumed < E
  if name in ('all-fit-absent-slots', 'one-example', 'length-equals-S-row'):
    assert consumed == E


def test_the_cases_are_the_edges_they_claim():
  """A check of the ORACLE alone, not of the library: `next_fit` of tests/_pack_cases.py gives the rows each case is named
  for, so that a case cannot drift away from its name.  It runs no product code and passes without the feature."""
  nf = lambda n: PC.next_fit(PC.CASES[n]['lengths'], PC.CASES[n]['S'], PC.CASES[n]['R'], PC.CASES[n]['S_row'], PC.CASES[n]['E_max'])
  assert nf('row-filled-exactly') == ([[8, 8], [4, 6, 6], []], 5)
  assert nf('one-over-opens-a-row') == ([[8, 7], [2, 8], [8, 1]], 6)
  assert nf('stop-at-row-R') == ([[8, 7], [2, 8]], 4)
  assert nf('stop-at-E-max') == ([[5, 6, 7], []], 3)
  assert nf('one-row') == ([[4, 8, 7]], 3)
  assert nf('length-equals-S-row') == ([[12], [3], [12], [9, 3]], 5)
  assert nf('lengths-clamped') == ([[1, 1, 8, 3], [8, 1], [8], []], 7)
  rows, consumed = nf('limit-4096')
  assert consumed == 4096 and len(PC.CASES['limit-4096']['lengths']) == 4096


def test_wild_positions_stay_inside_the_rows(lib):
  """Position tables are data: entries below 0 and at or above S are clamped into the example's S positions and the
  flat index into [0, R * S_row)."""
  c, ins, want, consumed = PC.case_data('length-equals-S-row', True)
  ins = dict(ins)
  ins['mlm_positions'] = torch.tensor([[-1, 2 ** 31 - 1, 5]] * 5, dtype=torch.int32)
  ins['mpp_positions'] = torch.tensor([[-2 ** 31, 12]] * 5, dtype=torch.int32)
  rc, out, whole = PC.call(ins, c['S'], c['S_row'], c['R'], c['E_max'], 'cpu')
  assert rc == 0
  PC.check_guards(out, whole)
  first = want['first_positions']
  base = first[:, 0] * c['S_row'] + first[:, 1]
  last = c['R'] * c['S_row'] - 1
  assert out['mlm_positions'].tolist() == [[int(b), min(int(b) + 11, last), min(int(b) + 5, last)] for b in base]
  assert out['mlm_positions'][4].tolist() == [45, 47, 47]                # the last example sits at the end of the last row
  assert out['mpp_positions'].tolist() == [[int(b), min(int(b) + 11, last)] for b in base]


def _refusal_args(**change):
  """A valid call's arguments by name, with `change` applied: (desc fields, pointers)."""
  from mmt_amd import _lib
  E, S, R, S_row, E_max = 3, 8, 2, 16, 4
  t = dict(word_ids=torch.ones(E, S, dtype=torch.int32), segment_ids=torch.ones(E, S, dtype=torch.int32),
           lengths=torch.full((E,), 5, dtype=torch.int32), mlm=torch.zeros(E, 2, dtype=torch.int32), mpp=None,
           out_word=torch.full((R, S_row), 77, dtype=torch.int32), out_seg=torch.full((R, S_row), 77, dtype=torch.int32),
           ids=torch.full((R, S_row), 77, dtype=torch.int32), starts=torch.full((R, S_row), 77, dtype=torch.int32),
           slots=torch.full((R, S_row), 77, dtype=torch.int32), first=torch.full((E_max, 2), 77, dtype=torch.int64),
           weight=torch.full((E_max,), 77.), out_mlm=torch.full((E_max, 2), 77, dtype=torch.int32), out_mpp=None,
           consumed=torch.full((1,), 77, dtype=torch.int32), ws=torch.full((64,), 77, dtype=torch.int32))
  d = _lib.PackDesc()
  d.E, d.S, d.R, d.S_row, d.E_max, d.n_mlm, d.n_mpp = E, S, R, S_row, E_max, 2, 0
  ws_bytes = 64 * 4
  for k, v in change.items():
    if k == 'ws_bytes':
      ws_bytes = v
    elif hasattr(d, k):
      setattr(d, k, v)
    else:
      t[k] = v
  p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
  order = ('word_ids', 'segment_ids', 'lengths', 'mlm', 'mpp', 'out_word', 'out_seg', 'ids', 'starts', 'slots', 'first', 'weight',
           'out_mlm', 'out_mpp', 'consumed', 'ws')
  return d, [p(t[k]) for k in order] + [ws_bytes], t


REFUSALS = [
    (dict(word_ids=None), -1, 'NULL argument'), (dict(segment_ids=None), -1, 'NULL argument'), (dict(lengths=None), -1, 'NULL argument'),
    (dict(out_word=None), -1, 'NULL argument'), (dict(ids=None), -1, 'NULL argument'), (dict(starts=None), -1, 'NULL argument'),
    (dict(slots=None), -1, 'NULL argument'), (dict(first=None), -1, 'NULL argument'), (dict(weight=None), -1, 'NULL argument'),
    (dict(consumed=None), -1, 'NULL argument'),
    (dict(E=0), -1, 'must be at least 1'), (dict(R=0), -1, 'must be at least 1'), (dict(E_max=-3), -1, 'must be at least 1'),
    (dict(S_row=7), -1, 'S_row 7 at least S'), (dict(S=0), -1, 'S 0 must be at least 1'),
    (dict(E=4097), -1, 'MMT_PACK_MAX_EXAMPLES'), (dict(E_max=4097), -1, 'MMT_PACK_MAX_EXAMPLES'),
    (dict(R=1 << 20, S_row=1 << 12), -1, 'below 2^31'), (dict(E=4096, S=1 << 20, S_row=1 << 20), -1, 'below 2^31'),
    (dict(n_mlm=0), -1, 'a position table needs'), (dict(out_mlm=None), -1, 'a position table needs'),
    (dict(ws=None), -3, 'workspace of 48 bytes needed, 0 given'), (dict(ws_bytes=47), -3, 'workspace of 48 bytes needed, 47 given'),
]


@pytest.mark.parametrize('change,code,text', REFUSALS, ids=[f'{i}-{"-".join(r[0])}' for i, r in enumerate(REFUSALS)])
def test_every_refusal_returns_its_code_and_message_and_writes_nothing(lib, change, code, text):
  d, args, t = _refusal_args(**change)
  assert lib.mmt_pack_rows_host(d, *args) == code
  msg = lib.mmt_last_error().decode()
  assert msg.startswith('mmt_pack_rows_host: ') and text in msg, msg
  for k in ('out_word', 'out_seg', 'ids', 'starts', 'slots', 'first', 'weight', 'out_mlm', 'consumed', 'ws'):
    if t[k] is not None:
      assert bool((t[k] == 77).all()), k
  bad = type(d)()
  assert lib.mmt_pack_rows_workspace_bytes(bad) == 0
  assert lib.mmt_pack_rows_host(None, *args) == -1


def test_a_valid_call_is_accepted_after_the_refusals(lib):
  d, args, t = _refusal_args()
  assert lib.mmt_pack_rows_workspace_bytes(d) == 48
  assert lib.mmt_pack_rows_host(d, *args) == 0
  assert int(t['consumed']) == 3 and t['weight'].tolist() == [1, 1, 1, 0]


def test_fused_pack_rows_on_cpu_tensors_takes_the_host_variant():
  from mmt_amd import fused
  c, ins, want, _ = PC.case_data('one-over-opens-a-row', True)
  out = fused.pack_rows(ins['word_ids'], ins['segment_ids'], ins['lengths'], c['R'], c['S_row'], c['E_max'],
                        mlm_positions=ins['mlm_positions'], mpp_positions=ins['mpp_positions'])
  assert out.keys() == want.keys()
  for k, w in want.items():
    assert out[k].device.type == 'cpu' and out[k].dtype == w.dtype and torch.equal(out[k], w), k
  from mmt_amd import _lib
  with pytest.raises(_lib.MmtError, match='S_row 4 at least S'):
    fused.pack_rows(ins['word_ids'], ins['segment_ids'], ins['lengths'], 2, 4, 3)


def test_pack_batch_keeps_per_example_tensors_and_weights_absent_slots():
  """`input_utils.pack_batch` on a CPU batch of the synthetic contract: per-example tensors are the pool's first
  max_examples entries untouched, every `*_weights` label is multiplied by example_weight, the packed inputs carry the
  layout, the flat positions and the pattern."""
  from mmt_amd import input_utils
  from mmt_amd.ops import AttentionPattern
  E, S, F = 5, 8, 6
  g = torch.Generator().manual_seed(0)
  pat = AttentionPattern(id_mode=0)
  inputs = {'word_ids': torch.randint(1, 99, (E, S), generator=g, dtype=torch.int32), 'segment_ids': torch.ones(E, S, dtype=torch.int32),
            'valid_len': torch.tensor([5, 6, 7, 6, 8], dtype=torch.int32), 'patch_embeddings': torch.randn(E, 2, F, generator=g),
            'mlm_positions': torch.tensor([[4, 0], [5, 1], [6, 2], [2, 0], [7, 3]], dtype=torch.int32),
            'mpp_positions': torch.tensor([[2], [3], [2], [0], [3]], dtype=torch.int32), 'attention_pattern': pat}
  labels = {'mlm_label_ids': torch.randint(0, 9, (E, 2), generator=g, dtype=torch.int32), 'mlm_label_weights': torch.ones(E, 2),
            'itm_label_ids': torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32), 'itm_label_weights': torch.ones(E)}
  pin, plab, consumed = input_utils.pack_batch(inputs, labels, rows=2, row_len=12, max_examples=4)
  assert int(consumed) == 3 and consumed.shape == (1,)              # [5, 6] | [7]; example 3 would open row 2
  assert set(pin) == {'word_ids', 'segment_ids', 'patch_embeddings', 'mlm_positions', 'mpp_positions', 'attention_pattern',
                      'example_ids', 'example_starts', 'patch_slots', 'first_positions'}
  assert pin['attention_pattern'] is pat and tuple(pin['word_ids'].shape) == (2, 12)
  assert torch.equal(pin['patch_embeddings'], inputs['patch_embeddings'][:4])
  assert pin['first_positions'].tolist() == [[0, 0], [0, 5], [1, 0], [0, 0]]
  assert pin['mlm_positions'].tolist() == [[4, 0], [10, 6], [18, 14], [0, 0]]
  assert pin['mpp_positions'].tolist() == [[2], [8], [14], [0]]
  assert torch.equal(plab['mlm_label_ids'], labels['mlm_label_ids'][:4]) and torch.equal(plab['itm_label_ids'], labels['itm_label_ids'][:4])
  assert plab['mlm_label_weights'].tolist() == [[1, 1], [1, 1], [1, 1], [0, 0]] and plab['itm_label_weights'].tolist() == [1, 1, 1, 0]
  # more slots than pool examples: the per-example tensors are padded with zeros behind the pool
  pin, plab, consumed = input_utils.pack_batch(inputs, labels, rows=4, row_len=12, max_examples=7)
  assert int(consumed) == 5 and tuple(pin['patch_embeddings'].shape) == (7, 2, F) and not pin['patch_embeddings'][5:].any()
  assert plab['itm_label_weights'].tolist() == [1, 1, 1, 1, 1, 0, 0] and tuple(plab['mlm_label_ids'].shape) == (7, 2)


def test_sanitizer_program_of_the_pack_host_stage():
  """`make asan-pack` (csrc/Makefile): the argument checks and mmt_pack_rows_host under AddressSanitizer + UBSan, driven by
  a C program with its own main in exact-size heap blocks.  CPU only; nothing is loaded into Python."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  csrc = os.path.join(root, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-pack'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'pack asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr


# ---- the loader's packing stage on shards written from the committed JPEG fixtures and the text corpus, on the CPU ------
IMAGE, PATCH, SEQ, BATCH = 32, 16, 32, 4
PER_EXAMPLE_LABELS = ('mlm_label_ids', 'mlm_label_weights', 'mpp_label_ids', 'mpp_label_weights')


@pytest.fixture(scope='module')
def loader_streams(tmp_path_factory):
  """The unpacked stream and the packed one of the same 24 records, seed and config: lists of (inputs, labels)."""
  import json
  from tests import _record_cases as R
  from mmt_amd import configs, pretrain_dataloader as pd
  d = tmp_path_factory.mktemp('pack')
  vocab = R.write_vocab(d / 'vocab.txt')
  R.write_shards(d, R.loader_records(24), 2)
  base = dict(input_path=str(d / '*.tfrecord'), vocab_filename=vocab, is_training=False, global_batch_size=BATCH, image_size=IMAGE,
              patch_size=PATCH, max_seq_len=SEQ, tasks='mlm', text_special_token_field_dict=json.dumps(R.FIELD_DICT),
              mlm_max_selections_per_seq=SEQ - 6, mpp_max_selections_per_seq=4, seed=11)
  plain = list(pd.MmtPretrainDataLoader(configs.MmtPretrainDataConfig(**base), device='cpu').load())
  loader = pd.MmtPretrainDataLoader(configs.MmtPretrainDataConfig(**base, pack_rows=2, pack_row_len=80), device='cpu')
  return plain, list(loader.load()), loader


def _consumed(inputs):
  return int(inputs['example_ids'].max(1).values.sum())          # ids fall from the row's example count


def test_config_keys_default_to_off():
  from mmt_amd import configs
  assert configs.MmtDataConfig().pack_rows == 0 and configs.MmtDataConfig().pack_row_len == 0
  cfg = configs.parse_configuration('mmt/pretraining', params_override='task.train_data.pack_rows=8,task.train_data.pack_row_len=2048')
  assert cfg.task.train_data.pack_rows == 8 and cfg.task.train_data.pack_row_len == 2048


def test_packed_loader_stream_equals_the_unpacked_stream(loader_streams):
  """The concatenation of the batches' consumed examples is the unpacked loader's stream: labels and patch features
  bitwise, the word and segment ids of every example read back from its place in the rows, the positions as flat
  indices of the same tokens; every example exactly once, across carry-overs (a batch takes 4 or 5 of the pool)."""
  plain, packed, loader = loader_streams
  cat = lambda k, side: torch.cat([b[side][k] for b in plain])
  want_in = {k: cat(k, 0) for k in ('word_ids', 'segment_ids', 'valid_len', 'patch_embeddings', 'mlm_positions', 'mpp_positions')}
  want_lab = {k: cat(k, 1) for k in PER_EXAMPLE_LABELS}
  N = want_in['word_ids'].shape[0]
  assert N == 24
  at, takes = 0, []
  for inputs, labels in packed:
    R_, L = inputs['word_ids'].shape
    M = inputs['first_positions'].shape[0]
    assert (R_, L) == (2, 80) and M == 4 * (80 // 8) and 'valid_len' not in inputs
    n = _consumed(inputs)
    takes.append(n)
    assert torch.equal(inputs['patch_embeddings'][:n], want_in['patch_embeddings'][at:at + n])
    for k in PER_EXAMPLE_LABELS:
      assert torch.equal(labels[k][:n], want_lab[k][at:at + n].to(labels[k].dtype)), k
      assert tuple(labels[k].shape) == (M,) + tuple(want_lab[k].shape[1:])
    assert not labels['mlm_label_weights'][n:].any() and not labels['mpp_label_weights'][n:].any()
    flat_w, flat_s = inputs['word_ids'].reshape(-1), inputs['segment_ids'].reshape(-1)
    covered = torch.zeros(R_ * L, dtype=torch.bool)
    for e in range(n):
      r, f = inputs['first_positions'][e].tolist()
      ln = int(want_in['valid_len'][at + e])
      sl = slice(r * L + f, r * L + f + ln)
      assert torch.equal(flat_w[sl], want_in['word_ids'][at + e, :ln]) and torch.equal(flat_s[sl], want_in['segment_ids'][at + e, :ln])
      assert bool((inputs['patch_slots'].reshape(-1)[sl] == e).all()) and bool((inputs['example_starts'].reshape(-1)[sl] == f).all())
      covered[sl] = True
      for k in ('mlm_positions', 'mpp_positions'):
        assert torch.equal(inputs[k][e], want_in[k][at + e] + (r * L + f)), k
    assert not flat_w[~covered].any() and bool((inputs['patch_slots'].reshape(-1)[~covered] == -1).all())
    at += n
  assert at == N and len(packed) >= 3 and all(1 <= t <= 5 for t in takes), takes
  assert loader.pack_batches == len(packed) and loader.pack_wait_seconds >= 0


def _check_packed_stream(plain, packed, rows, row_len, per_example_inputs, label_keys, index_keys=()):
  """The packed batches' consumed examples, concatenated, are the unpacked stream: per-example inputs and labels
  bitwise, word and segment ids read back from the rows; absent slots carry weight 0 and index -1.  Returns the takes."""
  cat = lambda k, side: torch.cat([b[side][k] for b in plain])
  want_in = {k: cat(k, 0) for k in ('word_ids', 'segment_ids', 'valid_len') + tuple(per_example_inputs) + tuple(index_keys)}
  want_lab = {k: cat(k, 1) for k in label_keys}
  N = want_in['word_ids'].shape[0]
  at, takes = 0, []
  for inputs, labels in packed:
    assert tuple(inputs['word_ids'].shape) == (rows, row_len) and 'valid_len' not in inputs
    M = inputs['first_positions'].shape[0]
    n = _consumed(inputs)
    takes.append(n)
    for k in per_example_inputs:
      assert torch.equal(inputs[k][:n], want_in[k][at:at + n]), k
    for k in index_keys:
      assert torch.equal(inputs[k][:n], want_in[k][at:at + n]) and tuple(inputs[k].shape) == (M,), k
      assert bool((inputs[k][n:] == -1).all()), k                # also where the pool holds real examples behind the prefix
    for k in label_keys:
      assert torch.equal(labels[k][:n], want_lab[k][at:at + n].to(labels[k].dtype)) and labels[k].shape[0] == M, k
      if k.endswith('_weights'):
        assert not labels[k][n:].any(), k
    flat_w, flat_s = inputs['word_ids'].reshape(-1), inputs['segment_ids'].reshape(-1)
    covered = torch.zeros(rows * row_len, dtype=torch.bool)
    for e in range(n):
      r, f = inputs['first_positions'][e].tolist()
      ln = int(want_in['valid_len'][at + e])
      sl = slice(r * row_len + f, r * row_len + f + ln)
      assert torch.equal(flat_w[sl], want_in['word_ids'][at + e, :ln]) and torch.equal(flat_s[sl], want_in['segment_ids'][at + e, :ln])
      assert bool((inputs['patch_slots'].reshape(-1)[sl] == e).all())
      covered[sl] = True
    assert not flat_w[~covered].any()
    at += n
  assert at == N, (at, N)
  return takes


def test_packed_classification_loader_stream_equals_the_unpacked_stream(tmp_path):
  """`MmtClassificationDataLoader` on CPU with `pack_rows`: 32 records, per-replica batch 8 (the matching step works on
  16), 2 rows of 80 positions -- every matched example once, in the unpacked order, across carry-overs."""
  import json
  from tests import _finetune_record_cases as F
  from tests import _record_cases as R
  from mmt_amd import configs, classification_dataloader as cd
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  R.write_shards(tmp_path, R.loader_records(32), 2)
  base = dict(input_path=str(tmp_path / '*.tfrecord'), vocab_filename=vocab, is_training=False, global_batch_size=F.BATCH,
              image_size=F.IMAGE, patch_size=F.PATCH, max_seq_len=F.SEQ, text_special_token_field_dict=json.dumps(R.FIELD_DICT),
              min_shift=5, seed=11)
  plain = list(cd.MmtClassificationDataLoader(configs.MmtClassificationDataConfig(**base), device='cpu').load())
  packed = list(cd.MmtClassificationDataLoader(configs.MmtClassificationDataConfig(**base, pack_rows=2, pack_row_len=80), device='cpu').load())
  takes = _check_packed_stream(plain, packed, 2, 80, ('patch_embeddings',), cd.LABEL_KEYS)
  assert sum(takes) == sum(b[0]['word_ids'].shape[0] for b in plain) >= 32 and len(packed) >= 6


def test_packed_retrieval_loader_marks_absent_slots_and_predict_drops_them(tmp_path):
  """`MmtRetrievalDataLoader` on CPU with `pack_rows`: all 35 pairs of 5 images and 7 texts once, in the unpacked order;
  the three index tensors are -1 in every slot at or behind `consumed` (the pool holds later pairs there), and the
  filter `predict.predict` applies to a packed batch keeps exactly the consumed pairs."""
  import json
  from tests import _finetune_record_cases as F
  from tests import _record_cases as R
  from mmt_amd import configs, retrieval_dataloader as rd
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  image_pattern, text_pattern = F.write_separate_sets(tmp_path)[:2]
  base = dict(vocab_filename=vocab, is_training=False, global_batch_size=F.BATCH, image_size=F.IMAGE, patch_size=F.PATCH,
              max_seq_len=F.SEQ, text_special_token_field_dict=json.dumps(R.FIELD_DICT), image_input_path=image_pattern,
              text_input_path=text_pattern)
  plain = list(rd.MmtRetrievalDataLoader(configs.MmtRetrievalDataConfig(**base), device='cpu').load())
  packed = list(rd.MmtRetrievalDataLoader(configs.MmtRetrievalDataConfig(**base, pack_rows=2, pack_row_len=80), device='cpu').load())
  keys = ('image_index', 'text_index', 'gt_image_index')
  takes = _check_packed_stream(plain, packed, 2, 80, ('patch_embeddings',), ('label_ids', 'label_weights'), keys)
  assert sum(takes) == 35 and len(packed) >= 7
  pairs = []
  for inputs, _ in packed:
    here = (inputs['image_index'] >= 0) & (inputs['text_index'] >= 0)
    assert int(here.sum()) == _consumed(inputs)
    pairs += list(zip(inputs['image_index'][here].tolist(), inputs['text_index'][here].tolist()))
  assert len(set(pairs)) == len(pairs) == 35
