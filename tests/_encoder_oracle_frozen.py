"""FROZEN COPY, for one comparison only (tests/test_oracle_encoder.py): the body of oracle/encoder.py as it stood
before it learnt keep masks and the storage mode.  With `masks=None, store=None` the oracle must still return these
values bit for bit.  Nothing else may import this file; it is not kept in step with the oracle on purpose.

The original docstring follows.

ORACLE (test infrastructure, not product code) -- the whole encoder / pretraining model on
the CPU, written out with dense torch-CPU ops (float64 by default) so that autograd provides
reference gradients for the train-step tests.

Follows `src/modeling/models/mmt_encoder.py:189-237` (embedding assembly),
App. A.3 (one transformer layer; etcmodel, un-vendored: PARITY UNPINNED, see
oracle/attention.py), `mmt_pretraining_model.py:129-151`, `masked_patch_prediction_layer.py:74-98`,
TFM MaskedLM / ClassificationHead, and the loss of
`modeling/losses/weighted_sparse_categorical_crossentropy_loss.py:17-43`.

Weights are read from a state dict with the parameter names of `mmt_amd` (the product) -- the
oracle shares NO code with it.  Only tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg may import this module.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _ln(x, w, b, eps=1e-12):
  mu = x.mean(-1, keepdim=True)
  var = ((x - mu) ** 2).mean(-1, keepdim=True)
  return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu_tanh(x):
  return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def dense_relative_attention(q, k, v, emb, bias, att_mask, rel_ids, mask_value=-10000.0):
  """[B,S,N,D] dense operator (App. A.3 inner_att core), one-hot lookup semantics."""
  B, S, N, D = q.shape
  content = torch.einsum('bqnd,bknd->bnqk', q, k)
  if emb is not None and rel_ids is not None:
    R = emb.shape[0]
    relall = torch.einsum('bqnd,rnd->bnqr', q, emb)
    if bias is not None:
      relall = relall + bias.t()[None, :, None, :]
    ok = (rel_ids >= 0) & (rel_ids < R)
    idx = torch.where(ok, rel_ids, torch.zeros_like(rel_ids)).long()
    rel = torch.gather(relall, 3, idx[:, None].expand(B, N, S, S))
    content = content + torch.where(ok[:, None], rel, torch.zeros_like(rel))
  s = content / math.sqrt(D)
  if att_mask is not None:
    s = s + (1 - att_mask)[:, None].to(s.dtype) * mask_value
  p = torch.softmax(s, dim=-1)
  return torch.einsum('bnqk,bknd->bqnd', p, v)


def encoder_forward(sd, cfg, word_ids, segment_ids, att_mask, rel_ids, patch_embeddings,
                    prefix='encoder.', dtype=torch.float64):
  """sequence_output [B,S,H] of MmtEncoder (dropout off)."""
  g = lambda name: sd[prefix + name].detach().to(dtype) if not sd[prefix + name].requires_grad else sd[prefix + name]
  H, N = cfg['hidden_size'], cfg['num_attention_heads']
  D = H // N
  if segment_ids is None:
    segment_ids = torch.ones_like(word_ids)
  we = g('_word_embedding_layer.embedding_table')[word_ids.long()]
  se = g('_segment_embedding_layer.embedding_table')[segment_ids.long()]
  we = _ln(we, g('_embedding_norm_layer.weight'), g('_embedding_norm_layer.bias'))
  x = we + se
  S = x.shape[1]
  if prefix + '_position_embeddings' in sd:
    x = x + g('_position_embeddings')[:S]
  if patch_embeddings is not None:
    pe = patch_embeddings.to(dtype) @ g('_patch_projection_weight').t() + g('_patch_projection_bias')
    x = x + F.pad(pe, (0, 0, 2, S - 2 - pe.shape[1]))
  B = x.shape[0]
  pre = cfg['use_pre_activation_order']
  for l in range(cfg['num_hidden_layers']):
    lp = f'_transformer_layers.layers.{l}.'
    def att(h):
      qkv = h @ g(lp + 'attention.qkv_weight').t() + g(lp + 'attention.qkv_bias')
      qkv = qkv.view(B, S, 3, N, D)
      emb = g(lp + 'attention.relative_emb_table') if (prefix + lp + 'attention.relative_emb_table') in sd else None
      bias = g(lp + 'attention.relative_bias_table') if (prefix + lp + 'attention.relative_bias_table') in sd else None
      o = dense_relative_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], emb, bias, att_mask, rel_ids)
      return o.reshape(B, S, H) @ g(lp + 'attention.output_weight').t() + g(lp + 'attention.output_bias')
    def ffn(h):
      y = _gelu_tanh(h @ g(lp + 'intermediate_weight').t() + g(lp + 'intermediate_bias'))
      return y @ g(lp + 'ffn_output_weight').t() + g(lp + 'ffn_output_bias')
    ln1 = lambda h: _ln(h, g(lp + 'attention_layer_norm.weight'), g(lp + 'attention_layer_norm.bias'))
    ln2 = lambda h: _ln(h, g(lp + 'ffn_layer_norm.weight'), g(lp + 'ffn_layer_norm.bias'))
    if pre:
      x = x + att(ln1(x))
      x = x + ffn(ln2(x))
    else:
      x = ln1(x + att(x))
      x = ln2(x + ffn(x))
  return x


def _gather(seq, pos):
  B, S, W = seq.shape
  flat = (pos.long() + (torch.arange(B) * S)[:, None]).reshape(-1)
  return seq.reshape(B * S, W)[flat]


def weighted_sparse_ce(logits, labels, weights):
  lp = torch.log_softmax(logits.reshape(-1, logits.shape[-1]), -1)
  nll = -lp[torch.arange(lp.shape[0]), labels.reshape(-1).long()].view(labels.shape)
  w = weights.to(nll.dtype)
  den = w.sum()
  return (w * nll).sum() / den if float(den) != 0 else (w * nll).sum() * 0


def pretraining_loss(sd, cfg, inputs, labels, dtype=torch.float64):
  """mlm + mpp + itm loss of MmtPretrainingModel + PretrainingTask.build_losses."""
  g = lambda name: sd[name].detach().to(dtype) if not sd[name].requires_grad else sd[name]
  seq = encoder_forward(sd, cfg, inputs['word_ids'], inputs.get('segment_ids'), inputs.get('att_mask'),
                        inputs.get('relative_att_ids'), inputs.get('patch_embeddings'), dtype=dtype)
  x = _gather(seq, inputs['mlm_positions'])
  x = _gelu_tanh(x @ g('masked_lm.dense_weight').t() + g('masked_lm.dense_bias'))
  x = _ln(x, g('masked_lm.layer_norm.weight'), g('masked_lm.layer_norm.bias'))
  table = g('encoder._word_embedding_layer.embedding_table')
  mlm_logits = (x @ table.t() + g('masked_lm.output_bias')).view(*inputs['mlm_positions'].shape, -1)
  y = _gather(seq, inputs['mpp_positions'])
  y = _ln(y, g('masked_pp.layer_norm.weight'), g('masked_pp.layer_norm.bias'))
  y = _gelu_tanh(y @ g('masked_pp.dense_weight').t() + g('masked_pp.dense_bias')) + g('masked_pp.bias')
  mpp_logits = y.view(*inputs['mpp_positions'].shape, -1)
  itm = labels['itm_label_ids'].unsqueeze(1).to(dtype)
  loss = weighted_sparse_ce(mlm_logits, labels['mlm_label_ids'], labels['mlm_label_weights'] * itm)
  loss = loss + weighted_sparse_ce(mpp_logits, labels['mpp_label_ids'], labels['mpp_label_weights'] * itm)
  c = seq[:, 0]
  c = torch.tanh(c @ g('classification_heads.0.dense_weight').t() + g('classification_heads.0.dense_bias'))
  itm_logits = c @ g('classification_heads.0.out_proj_weight').t() + g('classification_heads.0.out_proj_bias')
  loss = loss + weighted_sparse_ce(itm_logits, labels['itm_label_ids'], labels['itm_label_weights'])
  return loss
