"""Packed batches on the GPU: the device call of `mmt_pack_rows` against its host variant, and what the packed rows mean
to the train step -- the same examples through the task unpacked and packed, absent example slots, and the packed step
recorded as a HIP graph.

Shapes: the tiny model of tests/test_gpu_packed_origin.py (L = 2, H = 128, 2-D ids, P = 14, S = 256); rows of 512
positions hold examples of 200..256.  The kernel-only cases are the host cases of tests/_pack_cases.py."""
import pytest
import torch

from tests import _pack_cases as PC
from tests._cases import ENC_GRAD_TOL, ENC_TOL
from tests._parity import tiny_experiment

pytestmark = pytest.mark.gpu


# ---- the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tables', [True, False], ids=['tables', 'no-tables'])
@pytest.mark.parametrize('name', list(PC.CASES))
def test_device_call_equals_the_host_variant_bitwise(name, tables):
  """Same guarded buffers, same sentinel check, every output equal to the oracle's (which the host variant equals bit
  for bit in tests/test_pack_rows_host.py) and to the host variant's own outputs."""
  PC.check_case(name, tables, 'cuda')
  c, ins, _, _ = PC.case_data(name, tables)
  _, host, _ = PC.call(ins, c['S'], c['S_row'], c['R'], c['E_max'], 'cpu')
  rc, dev, whole = PC.call(ins, c['S'], c['S_row'], c['R'], c['E_max'], 'cuda')
  assert rc == 0 and dev.keys() == host.keys()
  PC.check_guards(dev, whole)
  for k in host:
    assert torch.equal(dev[k].cpu(), host[k]), k


def test_device_refusals_launch_nothing():
  from mmt_amd import _lib, fused
  c, ins, _, _ = PC.case_data('one-row', True)
  dev = {k: v.cuda() for k, v in ins.items()}
  with pytest.raises(_lib.MmtError, match='mmt_pack_rows: S 8 must be at least 1 and S_row 4 at least S'):
    fused.pack_rows(dev['word_ids'], dev['segment_ids'], dev['lengths'], 2, 4, 3)
  with pytest.raises(_lib.MmtError, match='MMT_PACK_MAX_EXAMPLES'):
    fused.pack_rows(dev['word_ids'], dev['segment_ids'], dev['lengths'], 2, 16, 4097)
  torch.cuda.synchronize()


# ---- the train step ------------------------------------------------------------------------------------------------------------
TEXT = [58, 2, 12, 48]                # examples of 256, 200, 210 and 246 positions: two rows of 512, each with a padding tail
ROWS, ROW_LEN = 2, 512


@pytest.fixture(scope='module')
def parity():
  """The tiny pretraining model in fp32 without dropout, one ragged unpacked batch of four examples with all three
  losses live, and the task's results on it: the reference of the packed runs, computed once."""
  import mmt_amd
  from mmt_amd import input_utils
  exp = tiny_experiment(S=256, core=2, R=49)
  exp.task.train_data.tasks = 'mlm,mpp,itm'
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  g = torch.Generator(device='cuda').manual_seed(5)
  inputs, labels = input_utils.synthetic_batch(exp.task.train_data, 4, 'cuda', g, vocab_size=2000, text_lengths=TEXT)
  assert inputs['valid_len'].tolist() == [256, 200, 210, 246]
  labels['itm_label_ids'] = torch.tensor([1, 0, 1, 1], dtype=torch.int32, device='cuda')     # a negative pair masks its MLM / MPP rows
  assert float(labels['mlm_label_weights'].sum()) > 0 and float(labels['mpp_label_weights'].sum()) > 0
  return dict(task=task, model=model, inputs=inputs, labels=labels, data=exp.task.train_data, want=run_step(task, model, (inputs, labels)))


def run_step(task, model, batch):
  """`task.train_step` with an optimizer that moves nothing: (total loss, {term: value}, {parameter: gradient})."""
  opt = torch.optim.SGD(model.parameters(), lr=0.0)
  terms = {}
  out = task.train_step(batch, model, opt, metrics=terms, step=1, micro_batch_size=batch[0]['word_ids'].shape[0])
  torch.cuda.synchronize()
  grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
  return float(out['loss']), {k: float(v[-1]) for k, v in terms.items()}, grads


def assert_same_step(got, want, what):
  loss, terms, grads = got
  w_loss, w_terms, w_grads = want
  print(f'{what}: loss {loss:.6f} against {w_loss:.6f}')
  assert abs(loss - w_loss) < ENC_TOL
  assert terms.keys() == w_terms.keys() == {'mlm_loss', 'mpp_loss', 'itm_loss'}
  for k in terms:
    print(f'  {k}: {terms[k]:.6f} against {w_terms[k]:.6f}')
    assert w_terms[k] > 0 and abs(terms[k] - w_terms[k]) < ENC_TOL, k
  assert grads.keys() == w_grads.keys() and len(grads) > 20
  worst = 0.0
  for n, g in grads.items():
    scale = float(w_grads[n].abs().max())
    assert scale > 0, n
    e = float((g - w_grads[n]).abs().max()) / max(1e-3, scale)
    worst = max(worst, e)
    assert e < ENC_GRAD_TOL, (n, e)
  print(f'  worst gradient error, relative to max |grad|: {worst:.3e}')


def test_packed_train_step_equals_the_unpacked_one(parity):
  """The same four examples through `train_step` as a ragged [4, 256] batch and packed into [2, 512]: total loss and
  each term within ENC_TOL, every parameter gradient within ENC_GRAD_TOL of its max |grad| -- the bounds of the
  packed-against-alone tests of tests/test_gpu_packed_origin.py."""
  from mmt_amd import input_utils
  pm = parity
  pin, plab, consumed = input_utils.pack_batch(pm['inputs'], pm['labels'], ROWS, ROW_LEN, 4)
  assert int(consumed) == 4 and pin['first_positions'].tolist() == [[0, 0], [0, 256], [1, 0], [1, 210]]
  assert tuple(pin['word_ids'].shape) == (ROWS, ROW_LEN) and tuple(pin['mlm_positions'].shape) == tuple(pm['inputs']['mlm_positions'].shape)
  assert_same_step(run_step(pm['task'], pm['model'], (pin, plab)), pm['want'], 'packed')


def test_absent_example_slots_change_nothing(parity):
  """E_max = 7 for the same four examples: three absent slots with weight 0 and positions 0.  The loss kernel's sums
  are not disturbed (lane t adds rows t, t + 256, .. in rising order and folds 256 lanes in a fixed tree; the absent
  rows come last and add exact zeros), but the logits in front of them come from GEMMs over more rows and the gradient
  of the gather from a scatter over more indices, whose tilings and orders may differ -- so the comparison keeps the
  tolerance of the packed run instead of asking for equal bits."""
  from mmt_amd import input_utils
  pm = parity
  pin, plab, consumed = input_utils.pack_batch(pm['inputs'], pm['labels'], ROWS, ROW_LEN, 7)
  assert int(consumed) == 4 and tuple(plab['mlm_label_ids'].shape)[0] == 7 and tuple(pin['patch_embeddings'].shape)[0] == 7
  assert plab['itm_label_weights'].tolist() == [1, 1, 1, 1, 0, 0, 0] and not pin['mlm_positions'][4:].any()
  assert_same_step(run_step(pm['task'], pm['model'], (pin, plab)), pm['want'], 'packed, three absent slots')


def test_validation_step_takes_a_packed_batch(parity):
  from mmt_amd import input_utils
  pm = parity
  pm['model'].eval()
  with torch.no_grad():
    want = float(pm['task'].validation_step((pm['inputs'], pm['labels']), pm['model'])['loss'])
    pin, plab, _ = input_utils.pack_batch(pm['inputs'], pm['labels'], ROWS, ROW_LEN, 5)
    got = float(pm['task'].validation_step((pin, plab), pm['model'])['loss'])
  pm['model'].train()
  print(f'validation loss packed {got:.6f} unpacked {want:.6f}')
  assert abs(got - want) < ENC_TOL


# ---- the recorded step -----------------------------------------------------------------------------------------------------------
def _twin(eager_only):
  import mmt_amd
  from mmt_amd import distribute, graphed, optimization, tasks
  exp = tiny_experiment(S=256, core=2, R=49)
  exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': 0.1, 'attention_probs_dropout_prob': 0.1}}},
                         'train_data': {'tasks': 'mlm,mpp,itm', 'pack_rows': ROWS, 'pack_row_len': ROW_LEN}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt_cfg = exp.trainer.optimizer_config
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()), reduce=tasks.gradient_reduce_mode(exp.task))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  step = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, clip_norm=opt_cfg.gradient_clip_norm, eager_steps=1)
  if eager_only:
    step.eager_left = 1 << 62
  data = task.build_inputs(exp.task.train_data, device='cuda', batch_size=2, ragged=True)
  return step, data, optimizer


def test_three_packed_steps_graphed_equal_three_eager_ones():
  """tests/test_gpu_graph.py's criterion on packed batches from `build_inputs` (a new batch every step, dropout 0.1,
  bf16): identical loss sequences and identical parameters.  The first call runs eagerly, the second records and
  replays, the third replays."""
  res = {}
  for eager_only in (True, False):
    step, data, optimizer = _twin(eager_only)
    losses = []
    for i in range(1, 4):
      batch = next(data)
      assert tuple(batch[0]['word_ids'].shape) == (ROWS, ROW_LEN) and batch[0]['first_positions'].shape[0] == 4
      losses.append(float(step(batch, i)['loss']))
    assert (step.graph is None) == eager_only
    res[eager_only] = (losses, torch.cat([s['param'] for s in optimizer.slabs]).clone())
    step.close()
  print('losses eager', res[True][0], 'graphed', res[False][0])
  assert res[True][0] == res[False][0]
  assert torch.equal(res[True][1], res[False][1])
  assert len(set(res[False][0])) == 3


# ---- the loader's packing stage on the device ------------------------------------------------------------------------------
def test_one_train_step_on_a_packed_loader_batch(tmp_path):
  """`build_inputs` on records with `pack_rows` set (shards written here from the committed JPEG fixtures): the batch has
  the packed layout with every slot's weight agreeing with the layout, and the task trains on it."""
  import json
  import numpy as np
  import mmt_amd
  from mmt_amd import optimization
  from tests import _record_cases as R
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  R.write_shards(tmp_path, R.loader_records(20), 2)
  exp = tiny_experiment()
  d = exp.task.train_data
  d.input_path, d.vocab_filename, d.text_special_token_field_dict = str(tmp_path / '*.tfrecord'), vocab, json.dumps(R.FIELD_DICT)
  d.mlm_max_selections_per_seq = 58                                      # every text position: whole words may exceed the tiny config's 8
  d.pack_rows, d.pack_row_len = 4, 512
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(3)
  model = task.build_model().cuda()
  opt = optimization.create_optimizer(model, exp.trainer.optimizer_config)
  it = task.build_inputs(d, device='cuda', batch_size=8, loader_args=dict(shuffle_buffer=8, example_shuffle_buffer=8))
  inputs, labels = next(it)
  assert task.input_source == 'records' and tuple(inputs['word_ids'].shape) == (4, 512) and 'valid_len' not in inputs
  M = 8 * (512 // (2 + 196 + 2))
  n = int(inputs['example_ids'].max(1).values.sum())
  assert inputs['first_positions'].shape[0] == M == labels['itm_label_ids'].shape[0] and 4 <= n <= 8
  assert labels['itm_label_weights'].tolist() == [1.0] * n + [0.0] * (M - n)
  out = task.train_step((inputs, labels), model, opt, clip_norm=1.0, step=1)
  assert np.isfinite(float(out['loss'])) and float(out['loss']) > 0


def test_predict_over_a_packed_retrieval_loader_scores_every_pair_once(tmp_path):
  """`predict.predict` over `MmtRetrievalDataLoader` with `pack_rows` (5 images x 7 texts, 4 rows of 512): the slots at
  or behind `consumed` carry index -1 and are dropped, so the results are the 35 pairs once each, in the unpacked order,
  with the unpacked scores within the encoder tolerance -- and the same recall@k."""
  import dataclasses
  import json
  import mmt_amd
  from mmt_amd import configs, predict
  from mmt_amd import retrieval_dataloader as rd
  from tests import _finetune_record_cases as F
  from tests import _record_cases as R
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  image_pattern, text_pattern = F.write_separate_sets(tmp_path)[:2]
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  cexp = configs.get_exp_config('mmt/retrieval')
  keep = {k: v for k, v in exp.task.train_data.as_dict().items() if hasattr(cexp.task.train_data, k)}
  cexp.override({'task': {'model': {'encoder': exp.task.model.encoder.as_dict(),
                                    'cls_heads': [{'inner_dim': 64, 'num_classes': 2, 'name': 'itm'}]},
                          'train_data': dict(keep, vocab_filename=vocab, is_training=False, drop_remainder=False,
                                             image_input_path=image_pattern, text_input_path=text_pattern,
                                             text_special_token_field_dict=json.dumps(R.FIELD_DICT))}})
  task = mmt_amd.tasks.get_task(cexp.task)
  torch.manual_seed(0)
  model = task.build_model().cuda().eval()
  cfg = cexp.task.train_data
  want = predict.predict(task, rd.MmtRetrievalDataLoader(cfg, device='cuda', chunk=4).load(batch_size=8), model)
  packed_cfg = dataclasses.replace(cfg, pack_rows=4, pack_row_len=512)
  batches = list(rd.MmtRetrievalDataLoader(packed_cfg, device='cuda', chunk=4).load(batch_size=8))
  assert any(bool((b[0]['image_index'] == -1).any()) for b in batches) and len(batches) >= 5
  got = predict.predict(task, batches, model)
  assert len(want) == 35 and [(r.image_index, r.text_index, r.gt_image_index) for r in got] == [(r.image_index, r.text_index, r.gt_image_index) for r in want]
  err = max(abs(a.output - b.output) for a, b in zip(got, want))
  print(f'max |packed - unpacked| score over 35 pairs: {err:.3e}')
  assert err < ENC_TOL
  assert max(r.output for r in want) - min(r.output for r in want) > 1e-4
  assert predict.get_recall_at_k(got) == predict.get_recall_at_k(want)
