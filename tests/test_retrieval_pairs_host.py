"""All pairs from separate sets, host side (mmt_amd/retrieval.py, MmtEncoder.embed_pairs' torch branch, the argument
checks of mmt_embed_fwd_pairs): no GPU."""
import json

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401

H, S, P, I, T = 64, 40, 3, 3, 4
N_IMG, LT = 2 + P * P, S - 2 - P * P            # 11, 29
TEXT_LEN = (0, 2, 17, 29)


def data_cfg():
  from mmt_amd import configs
  return configs.MmtRetrievalDataConfig(max_seq_len=S, image_size=16 * P, patch_size=16, relative_pos_max_distance=12,
                                        pos_weight=3.0)


@pytest.fixture(scope='module')
def sets():
  from mmt_amd import input_utils
  g = torch.Generator().manual_seed(5)
  s = input_utils.synthetic_retrieval_sets(data_cfg(), I, T, 'cpu', g, vocab_size=2000)
  n = torch.tensor(TEXT_LEN, dtype=torch.int32)
  s.num_text_wordpieces.copy_(n)
  s.text_token_ids.mul_((torch.arange(LT)[None] < n[:, None]).to(torch.int32))      # zero-padded as decode_fn pads
  s.image_index.copy_(torch.tensor([40, 7, 19]))
  s.gt_image_index.copy_(torch.tensor([19, 7, 40, 7]))
  return s


def encoder(position_table: bool):
  from mmt_amd import MmtEncoder
  torch.manual_seed(3)
  enc = MmtEncoder(vocab_size=2000, hidden_size=H, num_hidden_layers=0, num_attention_heads=1, intermediate_size=H,
                   max_absolute_position_embeddings=S + 3 if position_table else None, patch_embedding_size=768)
  with torch.no_grad():                            # the initial LayerNorm / bias values would hide a dropped term
    enc._embedding_norm_layer.weight.uniform_(0.5, 1.5)
    enc._embedding_norm_layer.bias.uniform_(-0.5, 0.5)
    enc._patch_projection_bias.uniform_(-0.5, 0.5)
  return enc.eval()


ENTRIES = (torch.tensor([0, 2, 2, 1, 0, 1, 2], dtype=torch.int32), torch.tensor([3, 0, 1, 2, 3, 3, 0], dtype=torch.int32))


@pytest.mark.parametrize('position_table', [True, False])
def test_embed_pairs_torch_branch_equals_embed_on_the_materialised_batch(sets, position_table):
  enc = encoder(position_table)
  ie, te = ENTRIES
  inputs, _ = sets.materialize(ie, te)
  with torch.no_grad():
    want = enc.embed(inputs['word_ids'], inputs['segment_ids'], inputs['patch_embeddings'])
    got, valid_len = enc.embed_pairs(sets, ie, te)
  assert got.dtype == torch.float32 and got.shape == (7, S, H)
  assert torch.equal(got, want)
  assert valid_len.dtype == torch.int32 and torch.equal(valid_len, inputs['valid_len'])
  # a write to the projection that torch's version counter does not see (what the fused optimizer's kernels do) is
  # seen by the next call: nothing about the image table is cached behind the caller's back
  proj = enc.project_image_table(sets)
  w = enc._patch_projection_weight
  version = w._version
  w.data.mul_(-2.0)
  assert w._version == version
  with torch.no_grad():
    want2 = enc.embed(inputs['word_ids'], inputs['segment_ids'], inputs['patch_embeddings'])
    got2, _ = enc.embed_pairs(sets, ie, te)
    assert torch.equal(got2, want2) and not torch.equal(got2, got)
    # a caller that keeps the projected table passes it in, and refreshes it in place
    assert torch.equal(enc.embed_pairs(sets, ie, te, patch_proj=proj)[0], got)
    assert enc.project_image_table(sets, out=proj) is proj
    assert torch.equal(enc.embed_pairs(sets, ie, te, patch_proj=proj)[0], want2)


def test_encoder_and_model_refuse_pairs_beside_explicit_inputs(sets):
  from mmt_amd import MmtClassificationModel, layers
  enc = encoder(False)
  ie, te = ENTRIES
  w = torch.zeros(7, S, dtype=torch.int32)
  for kw in ({'word_ids': w}, {'segment_ids': w}, {'patch_embeddings': sets.patch_embeddings[:1]},
             {'valid_len': torch.full((7,), S, dtype=torch.int32)}):
    with pytest.raises(ValueError, match='must be None'):
      enc(pairs=(sets, ie, te), **kw)
  model = MmtClassificationModel(enc, [layers.ClassificationHead(H, 2, name='itm')])
  with pytest.raises(ValueError, match='must be None'):
    model(word_ids=w, pairs=(sets, ie, te))


def test_materialize_is_the_loaders_batch(sets):
  from mmt_amd import feature_pipeline, input_utils
  from oracle import side_inputs as si
  ie, te = ENTRIES
  inputs, labels = sets.materialize(ie, te)
  assert set(inputs) == {'word_ids', 'segment_ids', 'patch_embeddings', 'attention_pattern', 'valid_len', 'image_index',
                         'text_index', 'gt_image_index'}
  assert inputs['attention_pattern'] == input_utils.attention_pattern_from_config(sets.data_cfg)
  for b, (i, t) in enumerate(zip(ie.tolist(), te.tolist())):
    n = TEXT_LEN[t]
    assert np.array_equal(inputs['segment_ids'][b].numpy(), si.make_segment_ids(N_IMG, n, S))
    assert int(inputs['valid_len'][b]) == N_IMG + n
    assert torch.equal(inputs['word_ids'][b, :N_IMG], sets.prefix_ids)
    assert torch.equal(inputs['word_ids'][b, N_IMG:], sets.text_token_ids[t])
    assert int((inputs['word_ids'][b, N_IMG + n:] != 0).sum()) == 0
    assert torch.equal(inputs['patch_embeddings'][b], sets.patch_embeddings[i])
    assert (int(inputs['image_index'][b]), int(inputs['text_index'][b]), int(inputs['gt_image_index'][b])) == \
        (int(sets.image_index[i]), int(sets.text_index[t]), int(sets.gt_image_index[t]))
  assert inputs['word_ids'].dtype == inputs['segment_ids'].dtype == inputs['valid_len'].dtype == torch.int32
  assert inputs['word_ids'][0, :3].tolist() == [input_utils.CLS_ID, input_utils.PATCH_ID, input_utils.PATCH_START_UNUSED_INDEX]
  want = feature_pipeline.make_retrieval_labels({'image_index': inputs['image_index'],
                                                 'gt_image_index': inputs['gt_image_index']}, pos_weight=3.0)
  assert set(labels) == {'label_ids', 'label_weights'}
  assert torch.equal(labels['label_ids'], want['label_ids']) and torch.equal(labels['label_weights'], want['label_weights'])
  assert labels['label_ids'].tolist() == [0, 1, 0, 0, 0, 1, 1] and float(labels['label_weights'][5]) == 3.0
  # the padding entry of pair_entries: no image, empty text, index -1
  pad, _ = sets.materialize([-1, 1], [2, -1])
  assert pad['valid_len'].tolist() == [N_IMG + 17, N_IMG] and int(pad['patch_embeddings'][0].abs().sum()) == 0
  assert pad['image_index'].tolist() == [-1, 7] and pad['text_index'].tolist()[1] == -1


def test_synthetic_sets_follow_the_layout_of_synthetic_batch():
  from mmt_amd import input_utils
  g = torch.Generator().manual_seed(11)
  s = input_utils.synthetic_retrieval_sets(data_cfg(), 5, 64, 'cpu', g, vocab_size=2000)
  n = s.num_text_wordpieces
  assert s.patch_embeddings.shape == (5, P * P, 768) and s.text_token_ids.shape == (64, LT)
  assert int(n.min()) >= 2 and int(n.max()) <= LT and len(set(n.tolist())) > 4                  # ragged
  assert (s.text_token_ids[:, 0] == input_utils.ATT_ID).all()
  last = s.text_token_ids[torch.arange(64), (n - 1).long()]
  assert (last == input_utils.SEP_ID).all()
  pad = torch.arange(LT)[None] >= n[:, None]
  assert (s.text_token_ids[pad] == 0).all() and (s.text_token_ids[~pad] > 0).all()
  assert set(s.gt_image_index.tolist()) <= set(s.image_index.tolist())


def test_pair_entries_order_shards_and_padding():
  from mmt_amd.retrieval import num_shard_pairs, pair_entries
  ni, nt, batch = 5, 7, 8                                      # 35 pairs: four full batches and a tail of three
  ie, te = pair_entries(ni, nt, 0, 40)
  assert ie.dtype == te.dtype == torch.int32
  assert ie[:35].tolist() == [p // nt for p in range(35)] and te[:35].tolist() == [p % nt for p in range(35)]   # image-major
  assert ie[35:].tolist() == [-1] * 5 and te[35:].tolist() == [-1] * 5
  tail = pair_entries(ni, nt, 4 * batch, batch)
  assert tail[0].tolist() == [4, 4, 4, -1, -1, -1, -1, -1] and tail[1].tolist() == [4, 5, 6, -1, -1, -1, -1, -1]
  seen = []
  for sid in (0, 1):
    n = num_shard_pairs(ni, nt, (sid, 2))
    assert n == (18 if sid == 0 else 17)
    a, b = pair_entries(ni, nt, 0, 24, (sid, 2))
    pairs = [(i, t) for i, t in zip(a.tolist(), b.tolist()) if i >= 0]
    assert len(pairs) == n and a[n:].tolist() == [-1] * (24 - n)
    assert all((i * nt + t) % 2 == sid for i, t in pairs)      # dataset.shard(2, sid)
    seen += pairs
  assert len(seen) == len(set(seen)) == 35 and set(seen) == {(i, t) for i in range(ni) for t in range(nt)}
  with pytest.raises(ValueError):
    pair_entries(ni, nt, 0, 8, (2, 2))


def _recall_case(case):
  rng = np.random.default_rng(7)
  ni, nt = 6, 9
  if case == 'distinct':
    scores = rng.permutation(ni * nt).reshape(ni, nt) / (ni * nt)
  else:
    scores = rng.choice([0.25, 0.5, 0.75], size=(ni, nt))       # heavy ties
  scores = scores.astype(np.float32)
  scored = np.ones((ni, nt), bool)
  image_index, text_index = np.arange(ni) + 10, np.arange(nt) + 100
  if case == 'shuffled':
    scores = (rng.permutation(ni * nt).reshape(ni, nt) / (ni * nt)).astype(np.float32)
    image_index = rng.permutation(np.arange(ni) * 13 + 5)        # unsorted, non-contiguous
    text_index = rng.permutation(np.arange(nt) * 7 + 1000)
    scored = rng.random((ni, nt)) > 0.3
    scored[2, :] = False                                         # an image no pair of which was scored
  gt_image_index = image_index[rng.integers(0, ni, nt)]
  return scores, scored, image_index, text_index, gt_image_index


@pytest.mark.parametrize('case', ['distinct', 'tied', 'shuffled'])
def test_recall_from_the_matrix_equals_the_raw_result_route(case, tmp_path):
  from mmt_amd import predict, retrieval
  scores, scored, img, txt, gt = _recall_case(case)
  if case == 'shuffled':
    scores[0, 0], scored[0, 0] = 1.5, True                       # clipped in the files
  args = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (scores, scored, img, txt, gt))
  results = retrieval.results_from_scores(*args)
  assert len(results) == int(scored.sum())
  topks = (1, 3, 5, 10)
  want = predict.get_recall_at_k(results, topks)
  got = retrieval.recall_at_k_from_scores(*args, topks=topks)
  assert list(got.items()) == list(want.items())
  assert len({v for v in got.values()}) > 1                      # not a case every rule answers alike
  a, b = tmp_path / 'raw', tmp_path / 'matrix'
  want_files = predict.write_results(results, str(a), topks)
  got_files = retrieval.write_results_from_scores(*args, str(b), topks)
  assert dict(got_files) == dict(want_files)
  for name in ('results.csv', 'recall.json'):
    assert open(a / name, 'rb').read() == open(b / name, 'rb').read(), name
  assert json.load(open(b / 'recall.json')) == dict(got_files)


def test_sets_refuse_bad_tables(sets):
  import dataclasses
  from mmt_amd.retrieval import RetrievalSets
  fields = {f.name: getattr(sets, f.name) for f in dataclasses.fields(sets)}
  RetrievalSets(**fields)
  with pytest.raises(ValueError, match='image_index holds duplicate'):
    RetrievalSets(**dict(fields, image_index=torch.tensor([4, 9, 4])))
  with pytest.raises(ValueError, match='text_index holds duplicate'):
    RetrievalSets(**dict(fields, text_index=torch.tensor([1, 2, 3, 1])))
  with pytest.raises(ValueError, match=r'num_text_wordpieces must lie in \[0, 29\]'):
    RetrievalSets(**dict(fields, num_text_wordpieces=torch.tensor([0, 2, 17, 30], dtype=torch.int32)))
  with pytest.raises(ValueError, match='patch_embeddings must be'):
    RetrievalSets(**dict(fields, patch_embeddings=torch.zeros(I, P * P + 1, 768)))
  with pytest.raises(ValueError, match='text_token_ids must be'):
    RetrievalSets(**dict(fields, text_token_ids=torch.zeros(T, LT - 1, dtype=torch.int32)))


def test_pair_entry_point_argument_errors_without_gpu():
  """mmt_embed_fwd_pairs refuses before any launch: NULL arguments and an image part that fills the row are
  MMT_E_INVALID (-1), dropout is MMT_E_UNSUPPORTED (-2), each with its message."""
  from mmt_amd import _lib
  L = _lib.lib()
  assert 'mmt_embed_fwd_pairs' in _lib.EXPORTS and hasattr(L, 'mmt_embed_fwd_pairs')
  d = _lib.EmbedDesc()
  d.rows, d.S, d.H, d.dtype = 2 * S, S, H, _lib.MMT_F32
  d.vocab, d.seg_vocab, d.patch_start, d.n_patch, d.eps = 2000, 16, 2, P * P, 1e-12
  call = lambda *ptrs: L.mmt_embed_fwd_pairs(d, *ptrs[:5], I, T, *ptrs[5:], None)
  ok = [1] * 5 + [1, 1, None, 1, 1, 1, None, 1, 1]     # entries, ids, lengths | tables (pos, bias nullable), proj, out, valid_len
  for k in (0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 13):
    ptrs = list(ok)
    ptrs[k] = None
    assert call(*ptrs) == -1, k
    assert b'mmt_embed_fwd_pairs: NULL argument' in L.mmt_last_error()
  ptrs = list(ok)
  ptrs[10] = None
  assert call(*ptrs) == -1 and b'n_patch > 0 but patch_proj is NULL' in L.mmt_last_error()
  d.dropout_p = 0.1
  assert call(*ok) == -2 and b'prediction only' in L.mmt_last_error()
  d.dropout_p = 0.0
  d.S, d.rows = N_IMG, 2 * N_IMG                          # n_img == S
  assert call(*ok) == -1 and b'leaves no room for text' in L.mmt_last_error()
  assert L.mmt_embed_fwd_pairs(None, *ok[:5], I, T, *ok[5:], None) == -1
