"""The dense encoder oracle's keep masks and storage mode (host only): the GPU train-step tests
(tests/test_gpu_train_step_oracle.py) compare against it, so it is checked here against its own earlier body, against
the op-level restatement of the residual block, and for the size of the storage model's error on the very weights,
inputs and keep masks of the bf16 GPU cases (`tests._parity.step_case`: hand-made, since the synthetic batch has no CPU
path -- word_ids [2,256], patch_embeddings [2,196,768], 8 MLM and 6 MPP positions, band 32 + 8 global tokens at 198,
valid lengths [256, 231])."""
import numpy as np
import pytest
import torch

from oracle import encoder as oenc
from oracle import layer_ops as lo
from tests import _encoder_oracle_frozen as frozen
from tests._cases import BF16_GRAD_TOL
from tests._parity import (STEP_CASES, STEP_NUMBER, STEP_P_DROP, dense_inputs_cpu, keep_masks_from_seeds,
                           oracle_micro_steps, restated_dropout_seeds, step_case, storage_model_bars)

S = 256
_CASES = {}


def _case(case='band-global', pre=True):
  """(model, encoder config, dense CPU inputs, labels) of a hand-made case, made once."""
  if (case, pre) not in _CASES:
    _, model, (inputs, labels), data_cfg = step_case(case, pre=pre)
    _CASES[case, pre] = (model, model.encoder.get_config(), dense_inputs_cpu(inputs, data_cfg), labels)
  return _CASES[case, pre]


def _masks(cfg, B, micro_step=0):
  """The keep masks micro-step `micro_step` of train step STEP_NUMBER draws on rank 0."""
  seeds = restated_dropout_seeds(STEP_NUMBER, micro_step, 0, cfg['num_hidden_layers'])
  return keep_masks_from_seeds(seeds, B, S, cfg['hidden_size'], cfg['num_attention_heads'], STEP_P_DROP, STEP_P_DROP)


def _leaves(model):
  return {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}


def _run(fn, case='band-global', pre=True, **kw):
  """(loss, gradients by name) of `fn` (a pretraining_loss) on fresh float64 leaves."""
  model, cfg, inputs, labels = _case(case, pre)
  sd = _leaves(model)
  loss = fn(sd, cfg, inputs, labels, **kw)
  loss.backward()
  return float(loss.detach()), {k: v.grad for k, v in sd.items()}


def _assert_same(a, b):
  assert a[0] == b[0], (a[0], b[0])
  assert a[1].keys() == b[1].keys()
  for name in a[1]:
    if a[1][name] is None or b[1][name] is None:
      assert a[1][name] is None and b[1][name] is None, name
    else:
      assert torch.equal(a[1][name], b[1][name]), name


@pytest.mark.parametrize('case,pre', [('band-global', True), ('2d', True), ('band-global', False)],
                         ids=['band-global', '2d', 'post-ln'])
def test_without_masks_and_store_the_oracle_is_bit_for_bit_what_it_was(case, pre):
  now = _run(oenc.pretraining_loss, case, pre)
  assert sum(g is not None for g in now[1].values()) > 30
  _assert_same(now, _run(frozen.pretraining_loss, case, pre))
  model, cfg, inputs, _ = _case(case, pre)
  args = (cfg, inputs['word_ids'], inputs['segment_ids'], inputs['att_mask'], inputs['relative_att_ids'],
          inputs['patch_embeddings'])
  sd = {k: v.detach().double() for k, v in model.named_parameters()}
  assert torch.equal(oenc.encoder_forward(sd, *args), frozen.encoder_forward(sd, *args))


def test_all_true_masks_and_float64_storage_change_nothing():
  _, cfg, inputs, _ = _case()
  B, H, N, L = len(inputs['word_ids']), cfg['hidden_size'], cfg['num_attention_heads'], cfg['num_hidden_layers']
  ones = lambda *shape: (torch.ones(shape, dtype=torch.bool), 1.0)
  masks = {'embed': ones(B, S, H), 'att': [ones(B, N, S, S) for _ in range(L)],
           'h1': [ones(B, S, H) for _ in range(L)], 'h2': [ones(B, S, H) for _ in range(L)]}
  plain = _run(oenc.pretraining_loss)
  _assert_same(plain, _run(oenc.pretraining_loss, masks=masks))
  _assert_same(plain, _run(oenc.pretraining_loss, store=torch.float64))
  dropped = _run(oenc.pretraining_loss, masks=_masks(cfg, B))
  assert abs(dropped[0] - plain[0]) > 1e-3               # real masks are not a no-op


def test_masks_need_the_pre_activation_order():
  model, cfg, inputs, labels = _case(pre=False)
  with pytest.raises(ValueError):
    oenc.pretraining_loss(_leaves(model), cfg, inputs, labels, masks=_masks(cfg, len(inputs['word_ids'])))


def test_restated_seeds_are_distinct_across_sites_micro_steps_and_steps():
  seen = [s for step in (7, 8) for micro in (0, 1) for s in restated_dropout_seeds(step, micro, 0, 2)]
  assert len(seen) == 4 * 7 and len(set(seen)) == len(seen)


def test_gradients_at_the_sites_vanish_where_dropped_and_match_the_block_restatement():
  model, cfg, inputs, labels = _case()
  B, L = len(inputs['word_ids']), cfg['num_hidden_layers']
  masks = _masks(cfg, B)
  sd = _leaves(model)
  seen = {}
  def hook(name, t):
    if t.requires_grad:
      t.retain_grad()
    seen[name] = t
  oenc.pretraining_loss(sd, cfg, inputs, labels, masks=masks, hook=hook).backward()
  sites = {'site:embed': masks['embed']}
  for l in range(L):
    sites.update({f'site:att.{l}': masks['att'][l], f'site:h1.{l}': masks['h1'][l], f'site:h2.{l}': masks['h2'][l]})
  assert sites.keys() == {k for k in seen if k.startswith('site:')}
  for name, (keep, _) in sites.items():
    grad = seen[name].grad
    assert grad.shape == keep.shape, name
    assert not grad[~keep].any(), name                   # exactly zero where the value was dropped
    assert grad[keep].abs().max() > 0, name
  # the attention-output site of the last layer against residual_block_bwd: x1 = x + Dropout(o + b), h = LN(x1),
  # x2 = x1 + ..., so x1's direct gradient is x2's and the LayerNorm's is h's
  l = L - 1
  keep, keep_prob = masks['h1'][l]
  lp = f'encoder._transformer_layers.layers.{l}.'
  two = lambda t: t.detach().numpy().reshape(B * S, -1)
  d_o, _, dbias, dgamma, dbeta = lo.residual_block_bwd(
      two(seen[f'x:x2.{l}'].grad), two(seen[f'x:ln2.{l}'].grad), two(seen[f'x:x1.{l}']),
      gamma=sd[lp + 'ffn_layer_norm.weight'].detach().numpy(), keep=keep.numpy().reshape(B * S, -1),
      inv_keep=1.0 / keep_prob)
  assert np.abs(d_o - two(seen[f'site:h1.{l}'].grad)).max() < 1e-12
  assert np.abs(dbias - sd[lp + 'attention.output_bias'].grad.numpy()).max() < 1e-12
  assert np.abs(dgamma - sd[lp + 'ffn_layer_norm.weight'].grad.numpy()).max() < 1e-12
  assert np.abs(dbeta - sd[lp + 'ffn_layer_norm.bias'].grad.numpy()).max() < 1e-12


def test_stored_tensors_are_representable_in_the_storage_dtype():
  model, cfg, inputs, labels = _case()
  stored = {}
  def hook(name, t):
    if name.startswith('store:'):
      stored[name] = t.detach()
  oenc.pretraining_loss(_leaves(model), cfg, inputs, labels, masks=_masks(cfg, len(inputs['word_ids'])),
                        store=torch.bfloat16, hook=hook)
  for l in range(cfg['num_hidden_layers']):              # the points the product keeps in its compute dtype, per block
    lp = f'store:_transformer_layers.layers.{l}.'
    for what in ('ln1', 'qkv', 'att_out', 'x1', 'ln2', 'ffn_u', 'ffn_gelu', 'ffn_out', 'x2', 'attention.qkv_weight',
                 'intermediate_weight', 'ffn_output_weight', 'attention.output_weight'):
      assert lp + what in stored, what
    assert f'store:att.{l}.p' in stored and f'store:att.{l}.out' in stored
  for what in ('embed', 'patch_proj', 'mlm_logits', 'mpp_logits', 'itm_logits', 'mlm_gelu', 'mlm_ln', 'mpp_ln'):
    assert 'store:' + what in stored, what
  for name, t in stored.items():
    assert t.dtype == torch.float64
    assert torch.equal(t.to(torch.bfloat16).to(torch.float64), t), name


def _bf16_references(case, dropout):
  """(float64 oracle, storage model) of a bf16 GPU case, as the GPU test computes them."""
  model, cfg, inputs, labels = _case(case)
  B = len(inputs['word_ids'])
  if case == 'micro-steps':                              # batch 4 as two micro-steps of 2, gradients of loss_i / 2 summed
    masks = [_masks(cfg, 2, i) for i in range(2)]
    return tuple(oracle_micro_steps(model, inputs, labels, masks, 2, 0.5, store=st) for st in (None, torch.bfloat16))
  masks = _masks(cfg, B) if dropout else None
  return tuple(_run(oenc.pretraining_loss, case, masks=masks, store=st) for st in (None, torch.bfloat16))


@pytest.mark.parametrize('case,dropout', [(c, d) for c in STEP_CASES for d in (False, True) if d or c != 'micro-steps'])
def test_storage_model_error_stays_under_the_bf16_ceiling(case, dropout):
  """The bf16 bars of the GPU cases are max(2 * e_ref, 2^-8) capped at BF16_GRAD_TOL: on each case's weights, inputs and
  masks the reference alone must stay under the cap, or the cap and not the model would be the bar."""
  ref64, ref_store = _bf16_references(case, dropout)
  e_ref, bars = storage_model_bars(ref64, ref_store)
  for name in sorted(e_ref, key=e_ref.get, reverse=True)[:5]:
    print(f'{case} {name}: e_ref {e_ref[name]:.3e} bar {bars[name]:.3e}')
  assert e_ref['loss'] > 0                               # the storage mode rounds something
  worst = max(e_ref, key=e_ref.get)
  assert 2 * e_ref[worst] < BF16_GRAD_TOL, (worst, e_ref[worst])
