"""All pairs from separate sets on the device: the pair instantiation of the embedding kernel against the existing kernel
on the materialised batch, the model on `pairs=` against the model on the materialised batch, and the scorer (eager,
graphed, fallen back) against `predict.predict`."""
import warnings

import pytest
import torch

import __graft_entry__  # noqa: F401
from tests._cases import ENC_TOL

pytestmark = pytest.mark.gpu

N_I, N_T, B = 3, 4, 7


def _kernel_case(H, S, n_patch, position_table, dtype):
  """Tables and entries for one shape, and the batch materialised by the rule of include/mmt_layer.h -- written out
  here, independent of the package's own materialize."""
  g = torch.Generator(device='cuda').manual_seed(H + S)
  vocab, n_img = 300, 2 + n_patch
  lt = S - n_img
  rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=g)
  tables = dict(word_table=rnd(vocab, H), seg_table=rnd(16, H), gamma=rnd(H) * 0.2 + 1.0, beta=rnd(H) * 0.2,
                pos_table=rnd(S + 5, H) if position_table else None)
  proj = rnd(N_I, n_patch, H).to(dtype)
  prefix = torch.randint(0, vocab, (n_img,), device='cuda', generator=g, dtype=torch.int32)
  text_ids = torch.randint(0, vocab, (N_T, lt), device='cuda', generator=g, dtype=torch.int32)
  text_ids[1, min(3, lt - 1)] = vocab + 7                                  # an id outside the vocabulary: a zero row
  text_len = torch.tensor([0, lt, lt + 9, -3], device='cuda', dtype=torch.int32)
  image_entry = torch.tensor([0, 2, 2, -1, N_I, 1, 0], device='cuda', dtype=torch.int32)
  text_entry = torch.tensor([1, 3, 1, 0, 2, N_T + 5, -1], device='cuda', dtype=torch.int32)
  # the rule
  i_ok = (image_entry >= 0) & (image_entry < N_I)
  t_ok = (text_entry >= 0) & (text_entry < N_T)
  tc = text_entry.long().clamp(0, N_T - 1)
  text = torch.where(t_ok[:, None], text_ids[tc], torch.zeros_like(text_ids[:1]))
  n_text = torch.where(t_ok, text_len[tc].clamp(0, lt), torch.zeros_like(text_entry))
  word_ids = torch.cat([prefix[None].expand(B, n_img), text], 1).contiguous()
  pos = torch.arange(S, device='cuda')[None]
  seg_ids = ((pos < n_img).to(torch.int32) + 2 * ((pos > n_img) & (pos < n_img + n_text[:, None])).to(torch.int32))
  patches = proj[image_entry.long().clamp(0, N_I - 1)]
  patches = torch.where(i_ok[:, None, None], patches, torch.zeros_like(patches[:1, :1])).contiguous()
  return tables, proj, prefix, text_ids, text_len, image_entry, text_entry, word_ids, seg_ids, patches, (n_img + n_text).to(torch.int32)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('H,S,n_patch,position_table', [(64, 40, 9, False), (768, 70, 25, True), (1032, 33, 4, False)],
                         ids=['H64', 'H768-pos', 'H1032'])
def test_pair_kernel_equals_the_kernel_on_the_materialised_batch(H, S, n_patch, position_table, dtype):
  from mmt_amd import fused
  (tables, proj, prefix, text_ids, text_len, image_entry, text_entry, word_ids, seg_ids, patches,
   want_len) = _kernel_case(H, S, n_patch, position_table, dtype)
  with torch.no_grad():
    want = fused.embed_assemble(word_ids, seg_ids, tables['word_table'], tables['seg_table'], tables['gamma'], tables['beta'],
                                pos_table=tables['pos_table'], patch_proj=patches, p=0.0, out_dtype=dtype)
    out = torch.full((B, S, H), float('nan'), dtype=dtype, device='cuda')
    valid_len = torch.full((B,), -77, dtype=torch.int32, device='cuda')
    got, got_len = fused.embed_assemble_pairs(image_entry, text_entry, prefix, text_ids, text_len, patch_proj=proj,
                                              seq_len=S, out_dtype=dtype, out=out, valid_len=valid_len, **tables)
  torch.cuda.synchronize()
  assert got is out and got_len is valid_len
  assert torch.isfinite(got.float()).all()
  assert torch.equal(got, want)
  assert got_len.dtype == torch.int32 and torch.equal(got_len, want_len)
  assert want_len.tolist() == [2 + n_patch + n for n in (S - 2 - n_patch, 0, S - 2 - n_patch, 0, S - 2 - n_patch, 0, 0)]


def test_pair_binding_is_forward_only_and_checks_shapes():
  from mmt_amd import fused
  tables, proj, prefix, text_ids, text_len, image_entry, text_entry, *_ = _kernel_case(64, 40, 9, False, torch.float32)
  args = (image_entry, text_entry, prefix, text_ids, text_len)
  kw = dict(patch_proj=proj, out_dtype=torch.float32, **tables)
  with pytest.raises(RuntimeError, match='forward only'):
    fused.embed_assemble_pairs(*args, **dict(kw, word_table=tables['word_table'].clone().requires_grad_(True)))
  with torch.no_grad():
    with pytest.raises(ValueError, match='text_entry'):
      fused.embed_assemble_pairs(image_entry, text_entry[:-1].contiguous(), prefix, text_ids, text_len, **kw)
    with pytest.raises(ValueError, match='image_entry'):
      fused.embed_assemble_pairs(image_entry.long(), text_entry, prefix, text_ids, text_len, **kw)
    with pytest.raises(ValueError, match='prefix_ids'):
      fused.embed_assemble_pairs(image_entry, text_entry, prefix[:-1].contiguous(), text_ids, text_len, **kw)
    with pytest.raises(ValueError, match='text_len'):
      fused.embed_assemble_pairs(image_entry, text_entry, prefix, text_ids, text_len[:-1].contiguous(), **kw)
    with pytest.raises(ValueError, match='sequence length'):
      fused.embed_assemble_pairs(*args, seq_len=41, **kw)
    with pytest.raises(ValueError, match='patch_proj'):
      fused.embed_assemble_pairs(*args, **dict(kw, patch_proj=proj.to(torch.bfloat16)))


# ---- model and scorer ------------------------------------------------------------------------------------------------
SET_I, SET_T, BATCH = 5, 7, 8            # 35 pairs: four full batches and a tail of three


def _retrieval(dtype):
  import mmt_amd
  from mmt_amd import configs, input_utils
  from tests._parity import tiny_experiment
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp = configs.get_exp_config('mmt/retrieval')
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(),
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': exp.task.train_data.as_dict()}}, strict=False)
  task = mmt_amd.tasks.get_task(cexp.task, compute_dtype=dtype)
  torch.manual_seed(0)
  model = task.build_model().cuda().eval()
  g = torch.Generator(device='cuda').manual_seed(1)
  sets = input_utils.synthetic_retrieval_sets(cexp.task.train_data, SET_I, SET_T, 'cuda', g, vocab_size=2000)
  return task, model, sets


@pytest.fixture(scope='module')
def fp32_setup():
  """The fp32 model and sets, and the eager scorer's matrix every scorer test compares with (computed once)."""
  from mmt_amd.retrieval import PairScorer
  task, model, sets = _retrieval(torch.float32)
  scorer = PairScorer(task, model, sets, BATCH, graph=False)
  scores, scored = scorer.score_all()
  torch.cuda.synchronize()
  return task, model, sets, scorer, scores.clone(), scored.clone()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_model_on_pairs_equals_model_on_the_materialised_batch(dtype, fp32_setup):
  task, model, sets = fp32_setup[:3] if dtype == torch.float32 else _retrieval(dtype)
  ie = torch.arange(SET_I, device='cuda', dtype=torch.int32)
  te = torch.full((SET_I,), 3, device='cuda', dtype=torch.int32)
  inputs, _ = sets.materialize(ie, te)
  for k in ('image_index', 'text_index', 'gt_image_index'):
    inputs.pop(k)
  with torch.no_grad():
    want = model(**inputs, training=False)['itm_logits']
    got = model(pairs=(sets, ie, te), attention_pattern=inputs['attention_pattern'], training=False)['itm_logits']
  torch.cuda.synchronize()
  assert got.shape == (SET_I, 2) and torch.isfinite(got.float()).all()
  assert torch.equal(got, want), float((got.float() - want.float()).abs().max())


def _predict_results(task, model, sets):
  """The route that existed before: `predict.predict` over materialised batches of the same 8-pair windows."""
  from mmt_amd import predict
  from mmt_amd.retrieval import pair_entries
  batches = [sets.materialize(*pair_entries(SET_I, SET_T, first, BATCH, device='cuda'))
             for first in range(0, SET_I * SET_T, BATCH)]
  results = [r for r in predict.predict(task, batches, model) if r.image_index >= 0]
  assert len(results) == SET_I * SET_T
  return results


def _max_diff(scores, results):
  m = scores.cpu()
  return max(abs(float(m[r.image_index, r.text_index]) - r.output) for r in results)      # the sets' ids are 0 .. n - 1


def test_scorer_matches_predict_on_materialised_batches(fp32_setup):
  from mmt_amd import predict
  from mmt_amd.retrieval import recall_at_k_from_scores, results_from_scores
  task, model, sets, _, scores, scored = fp32_setup
  results = _predict_results(task, model, sets)
  assert bool(scored.all())
  m = scores.cpu()
  err = _max_diff(scores, results)
  print(f'scorer vs predict on materialised batches: max abs diff {err:.3e}')
  assert err <= ENC_TOL
  assert float(m.min()) > 0.0 and float(m.max()) < 1.0 and float(m.max() - m.min()) > 1e-4
  idx = (sets.image_index, sets.text_index, sets.gt_image_index)
  assert recall_at_k_from_scores(scores, scored, *idx) == predict.get_recall_at_k(results_from_scores(scores, scored, *idx))


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graphed'])
def test_weights_written_between_two_scoring_calls_are_seen(fp32_setup, graph):
  """The projected image table must follow the projection's weights.  Eager: a write through the raw storage, which
  torch's version counter does not see -- what the fused optimizer's kernels and a replayed train step do.  Graphed: an
  in-place `load_state_dict`, as a checkpoint sweep does, between two replayed runs.  Both against `predict.predict`
  on materialised batches with the new weights."""
  from mmt_amd.retrieval import PairScorer
  task, model, sets, _, scores, _ = fp32_setup
  w, b = model.encoder._patch_projection_weight, model.encoder._patch_projection_bias
  saved = {k: v.clone() for k, v in model.state_dict().items()}
  scorer = PairScorer(task, model, sets, BATCH, graph=graph)
  try:
    with warnings.catch_warnings():
      warnings.simplefilter('error')
      first, _ = scorer.score_all()
      assert torch.equal(first, scores)
      if graph:
        assert scorer.graph is not None
        state = {k: v.clone() for k, v in saved.items()}
        state['encoder._patch_projection_weight'] = -8.0 * w.detach()
        state['encoder._patch_projection_bias'] = b.detach() + 1.0
        model.load_state_dict(state)
      else:
        versions = (w._version, b._version)
        w.data.mul_(-8.0)
        b.data.add_(1.0)
        assert (w._version, b._version) == versions
      second, _ = scorer.score_all()
      shortlist = scorer.score_pairs([4, 0, 2], [6, 0, 3])
    torch.cuda.synchronize()
    results = _predict_results(task, model, sets)
    stale, err = _max_diff(first, results), _max_diff(second, results)
    print(f'after the write: stale scores off by {stale:.3e}, fresh scores by {err:.3e}')
    assert stale > 2 * ENC_TOL                     # the write moves the scores: stale ones could not pass the bar below
    assert err <= ENC_TOL
    assert torch.equal(shortlist, second[[4, 0, 2], [6, 0, 3]])
  finally:
    model.load_state_dict(saved)
    scorer.close()
  again, _ = PairScorer(task, model, sets, BATCH, graph=False).score_all()
  assert torch.equal(again, scores)                # the shared model is as the other tests expect it


def test_scorer_refuses_a_logits_key_the_model_does_not_have(fp32_setup):
  from mmt_amd.retrieval import PairScorer
  task, model, sets = fp32_setup[:3]
  with pytest.raises(KeyError, match='itn_logits'):
    PairScorer(task, model, sets, BATCH, logits_key='itn_logits', graph=False).score_all()


def test_graphed_scorer_gives_the_eager_bits(fp32_setup):
  from mmt_amd.retrieval import PairScorer
  task, model, sets, _, scores, scored = fp32_setup
  graphed = PairScorer(task, model, sets, BATCH, graph=True)
  with warnings.catch_warnings():
    warnings.simplefilter('error')                       # a fallback would pass the comparison eagerly
    got, got_scored = graphed.score_all()
    again, _ = graphed.score_all()
  torch.cuda.synchronize()
  assert graphed.graph is not None
  assert torch.equal(got, scores) and torch.equal(again, scores) and torch.equal(got_scored, scored)
  graphed.close()
  assert graphed.graph is None


def test_sharded_scoring_fills_its_own_pairs(fp32_setup):
  from mmt_amd.retrieval import PairScorer
  task, model, sets, scorer, scores, _ = fp32_setup
  got, got_scored = scorer.score_all(shard=(1, 2))
  want = (torch.arange(SET_I * SET_T, device='cuda') % 2 == 1).view(SET_I, SET_T)
  assert torch.equal(got_scored, want)
  assert bool((got[~want] == -1).all())
  # the same pairs in other batches, other rows: same kernels, same shapes
  assert float((got[want] - scores[want]).abs().max()) <= ENC_TOL


def test_score_pairs_equals_the_matrix_entries(fp32_setup):
  _, _, _, scorer, scores, _ = fp32_setup
  ie, te = [4, 0, 2, 2, 1, 3], [6, 0, 3, 5, 1, 2]
  got = scorer.score_pairs(ie, te)
  torch.cuda.synchronize()
  assert got.shape == (6,) and torch.equal(got, scores[ie, te])


class _RaisesWhileCapturing(torch.nn.Module):
  def __init__(self, model):
    super().__init__()
    self.model = model

  def forward(self, **kw):
    if torch.cuda.is_current_stream_capturing():
      raise RuntimeError('this module cannot be captured')
    return self.model(**kw)


def test_capture_that_raises_falls_back_to_eager_with_one_warning(fp32_setup):
  from mmt_amd.retrieval import PairScorer
  task, model, sets, _, scores, scored = fp32_setup
  scorer = PairScorer(task, _RaisesWhileCapturing(model), sets, BATCH, graph=True)
  with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter('always')
    got, got_scored = scorer.score_all()
  torch.cuda.synchronize()
  ours = [w for w in caught if 'not recorded as a HIP graph' in str(w.message)]
  assert len(ours) == 1 and 'cannot be captured' in str(ours[0].message)
  assert scorer.graph is None and scorer.use_graph is False
  assert torch.equal(got, scores) and torch.equal(got_scored, scored)
