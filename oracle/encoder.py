"""ORACLE (test infrastructure, not product code) -- the whole encoder / pretraining model on
the CPU, written out with dense torch-CPU ops (float64 by default) so that autograd provides
reference gradients for the train-step tests.

Follows `src/modeling/models/mmt_encoder.py:189-237` (embedding assembly),
App. A.3 (one transformer layer; etcmodel, un-vendored: PARITY UNPINNED, see
oracle/attention.py), `mmt_pretraining_model.py:129-151`, `masked_patch_prediction_layer.py:74-98`,
TFM MaskedLM / ClassificationHead, and the loss of
`modeling/losses/weighted_sparse_categorical_crossentropy_loss.py:17-43`.

Dropout is taken as explicit keep masks (`masks`), never drawn here: the caller restates the masks the product drew
(`oracle.layer_ops.dropout_keep_mask`, `oracle.attention.dropout_keep_mask`) and the oracle applies them where the
product does.  `store` models "bf16 storage, exact arithmetic": every tensor the product keeps in its compute dtype is
rounded to `store` and back, and autograd's cast rounds the gradients at the same points (plus the operands only the
backward kernels keep in that dtype: the gradient of the attention scores, the tanh result of the ITM head).  That mode sizes the bars of
the bf16 train-step tests; it is not a second product.

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


def _storer(store, hook):
  """st(x, name): x as the product keeps it -- rounded to `store` and back (identity without `store`); `hook(name, x)`
  sees every tensor that passes."""
  def st(x, name):
    if store is not None:
      x = x.to(store).to(x.dtype)
      if hook is not None:
        hook('store:' + name, x)
    return x
  def grad(x):
    """x unchanged, its GRADIENT rounded: an operand that only the backward kernels keep in the compute dtype."""
    if store is not None and x.requires_grad:
      x.register_hook(lambda g: g.to(store).to(g.dtype))
    return x
  st.grad = grad
  return st


class _TanhStored(torch.autograd.Function):
  """tanh whose result is kept in `store`, and whose backward reads that kept result: torch.tanh on a bf16 tensor saves
  its bf16 output and differentiates as g * (1 - y^2) with it (`layers.ClassificationHead.forward`, `self.activation(x)`)."""

  @staticmethod
  def forward(ctx, x, store):
    y = torch.tanh(x).to(store).to(x.dtype)
    ctx.save_for_backward(y)
    ctx.store = store
    return y

  @staticmethod
  def backward(ctx, g):
    y, = ctx.saved_tensors
    return torch.ops.aten.tanh_backward(g.to(ctx.store).to(g.dtype), y), None


def _drop(t, site, name, hook):
  """Dropout with the explicit keep mask `site = (keep, keep_prob)`: kept values divided by keep_prob, the others 0.
  `hook('site:' + name, t)` sees the tensor the mask is applied to."""
  if hook is not None:
    hook('site:' + name, t)
  if site is None:
    return t
  keep, keep_prob = site
  keep = torch.as_tensor(keep).reshape(t.shape)
  return torch.where(keep, t / keep_prob, torch.zeros_like(t))


def dense_relative_attention(q, k, v, emb, bias, att_mask, rel_ids, mask_value=-10000.0, keep=None, st=None,
                             hook=None, name='att'):
  """[B,S,N,D] dense operator (App. A.3 inner_att core), one-hot lookup semantics.  keep = (mask [B,N,S,S], keep_prob)
  on the softmax probabilities, as `oracle.attention.relative_attention_fwd(keep_mask=, keep_prob=)`.  `st` rounds what
  the kernels keep in the compute dtype: P as the operand of the PV product BEFORE the keep scaling (the forward kernels
  feed the MFMA the bare probabilities and apply 1 / keep_prob to the accumulators, csrc/attn_fwd_band.hip:391; the
  backward hands P over the same way, csrc/attn_bwd_band.hip:58-61, :1291), the gradient of the scores, which is the
  bf16 operand of the dQ and dK products (csrc/attn_bwd_band.hip:358, :910), and the output."""
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
  if st is not None:
    s = st.grad(s)
  p = torch.softmax(s, dim=-1)
  if st is not None:
    p = st(p, name + '.p')
  if keep is not None or hook is not None:
    p = _drop(p, keep, name, hook)
  o = torch.einsum('bnqk,bknd->bqnd', p, v)
  return o if st is None else st(o, name + '.out')


def encoder_forward(sd, cfg, word_ids, segment_ids, att_mask, rel_ids, patch_embeddings,
                    prefix='encoder.', dtype=torch.float64, masks=None, store=None, hook=None):
  """sequence_output [B,S,H] of MmtEncoder.

  masks: None (dropout off) or {'embed': site, 'att': [site per layer], 'h1': [...], 'h2': [...]} with
  site = (bool keep mask, keep probability): [B,S,H] on the LayerNorm output of the word embeddings, [B,N,S,S] on the
  softmax probabilities, [B,S,H] on `attention output + output_bias` and on `ffn output + ffn_output_bias` before each
  residual add (pre-activation order only: the product's other order draws from torch's generator).
  store: None or a torch dtype, the storage model of the module docstring.
  hook(name, tensor): debug hook -- 'store:<name>' for every rounded tensor, 'site:<name>' for the tensor each mask
  applies to, 'x:<name>' for the residual stream and LayerNorm outputs of the blocks."""
  g = lambda name: sd[prefix + name].detach().to(dtype) if not sd[prefix + name].requires_grad else sd[prefix + name]
  st = _storer(store, hook)
  gw = lambda name: st(g(name), name)                 # a weight as a GEMM operand (and a bias a library GEMM adds)
  see = (lambda name, t: hook('x:' + name, t)) if hook is not None else (lambda name, t: None)
  pre = cfg['use_pre_activation_order']
  if masks is not None and not pre:
    raise ValueError('masks need use_pre_activation_order=True (the other order draws from torch\'s generator)')
  site = lambda kind, l=None: None if masks is None else (masks[kind] if l is None else masks[kind][l])
  H, N = cfg['hidden_size'], cfg['num_attention_heads']
  D = H // N
  if segment_ids is None:
    segment_ids = torch.ones_like(word_ids)
  we = g('_word_embedding_layer.embedding_table')[word_ids.long()]
  se = g('_segment_embedding_layer.embedding_table')[segment_ids.long()]
  we = _ln(we, g('_embedding_norm_layer.weight'), g('_embedding_norm_layer.bias'))
  if masks is not None or hook is not None:
    we = _drop(we, site('embed'), 'embed', hook)
  x = we + se
  S = x.shape[1]
  if prefix + '_position_embeddings' in sd:
    x = x + g('_position_embeddings')[:S]
  if patch_embeddings is not None:
    # the projection is a Dense layer of the stack: operands and result in the compute dtype (encoder.py `embed`)
    pe = st(patch_embeddings.to(dtype), 'patch_embeddings') @ gw('_patch_projection_weight').t() + gw('_patch_projection_bias')
    x = x + F.pad(st(pe, 'patch_proj'), (0, 0, 2, S - 2 - pe.shape[1]))
  x = st(x, 'embed')                                  # the embedding kernel reads fp32 tables and rounds its sum once
  B = x.shape[0]
  for l in range(cfg['num_hidden_layers']):
    lp = f'_transformer_layers.layers.{l}.'
    def att(h):
      qkv = st(h @ gw(lp + 'attention.qkv_weight').t() + gw(lp + 'attention.qkv_bias'), lp + 'qkv')
      qkv = qkv.view(B, S, 3, N, D)
      emb = gw(lp + 'attention.relative_emb_table') if (prefix + lp + 'attention.relative_emb_table') in sd else None
      bias = gw(lp + 'attention.relative_bias_table') if (prefix + lp + 'attention.relative_bias_table') in sd else None
      o = dense_relative_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], emb, bias, att_mask, rel_ids,
                                   keep=site('att', l), st=st if store is not None else None, hook=hook, name=f'att.{l}')
      # the output bias is added in fp32 by the residual kernel, after the GEMM's result was stored
      return st(o.reshape(B, S, H) @ gw(lp + 'attention.output_weight').t(), lp + 'att_out') + g(lp + 'attention.output_bias')
    def ffn(h):
      u = st(h @ gw(lp + 'intermediate_weight').t(), lp + 'ffn_u')           # kept without its bias (layers._FfnFn)
      y = st(_gelu_tanh(u + g(lp + 'intermediate_bias')), lp + 'ffn_gelu')
      return st(y @ gw(lp + 'ffn_output_weight').t(), lp + 'ffn_out') + g(lp + 'ffn_output_bias')
    ln1 = lambda h: st(_ln(h, g(lp + 'attention_layer_norm.weight'), g(lp + 'attention_layer_norm.bias')), lp + 'ln1')
    ln2 = lambda h: st(_ln(h, g(lp + 'ffn_layer_norm.weight'), g(lp + 'ffn_layer_norm.bias')), lp + 'ln2')
    if pre:
      t = att(ln1(x))
      if masks is not None or hook is not None:
        t = _drop(t, site('h1', l), f'h1.{l}', hook)
      x = st(x + t, lp + 'x1')
      see(f'x1.{l}', x)
      h = ln2(x)
      see(f'ln2.{l}', h)
      t = ffn(h)
      if masks is not None or hook is not None:
        t = _drop(t, site('h2', l), f'h2.{l}', hook)
      x = st(x + t, lp + 'x2')
      see(f'x2.{l}', x)
    else:
      x = ln1(st(x + att(x), lp + 'x1'))
      x = ln2(st(x + ffn(x), lp + 'x2'))
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


def pretraining_loss(sd, cfg, inputs, labels, dtype=torch.float64, masks=None, store=None, hook=None):
  """mlm + mpp + itm loss of MmtPretrainingModel + PretrainingTask.build_losses; `masks`, `store`, `hook` as
  `encoder_forward` (the heads draw no masks: their `dropout_rate` is torch's)."""
  g = lambda name: sd[name].detach().to(dtype) if not sd[name].requires_grad else sd[name]
  st = _storer(store, hook)
  gw = lambda name: st(g(name), name)
  seq = encoder_forward(sd, cfg, inputs['word_ids'], inputs.get('segment_ids'), inputs.get('att_mask'),
                        inputs.get('relative_att_ids'), inputs.get('patch_embeddings'), dtype=dtype,
                        masks=masks, store=store, hook=hook)
  x = _gather(seq, inputs['mlm_positions'])
  # bias + GELU run in one fp32 pass over the stored GEMM result (layers.MaskedLM, bf16 branch)
  x = st(_gelu_tanh(st(x @ gw('masked_lm.dense_weight').t(), 'mlm_dense') + g('masked_lm.dense_bias')), 'mlm_gelu')
  x = st(_ln(x, g('masked_lm.layer_norm.weight'), g('masked_lm.layer_norm.bias')), 'mlm_ln')
  table = gw('encoder._word_embedding_layer.embedding_table')
  mlm_logits = st(x @ table.t() + gw('masked_lm.output_bias'), 'mlm_logits').view(*inputs['mlm_positions'].shape, -1)
  y = _gather(seq, inputs['mpp_positions'])
  y = st(_ln(y, g('masked_pp.layer_norm.weight'), g('masked_pp.layer_norm.bias')), 'mpp_ln')
  y = st(_gelu_tanh(st(y @ gw('masked_pp.dense_weight').t() + gw('masked_pp.dense_bias'), 'mpp_dense')), 'mpp_gelu')
  y = st(y + gw('masked_pp.bias'), 'mpp_logits')
  mpp_logits = y.view(*inputs['mpp_positions'].shape, -1)
  itm = labels['itm_label_ids'].unsqueeze(1).to(dtype)
  loss = weighted_sparse_ce(mlm_logits, labels['mlm_label_ids'], labels['mlm_label_weights'] * itm)
  loss = loss + weighted_sparse_ce(mpp_logits, labels['mpp_label_ids'], labels['mpp_label_weights'] * itm)
  c = seq[:, 0]
  c = st(c @ gw('classification_heads.0.dense_weight').t() + gw('classification_heads.0.dense_bias'), 'itm_dense')
  c = st(torch.tanh(c) if store is None else _TanhStored.apply(c, store), 'itm_tanh')
  itm_logits = st(c @ gw('classification_heads.0.out_proj_weight').t() + gw('classification_heads.0.out_proj_bias'),
                  'itm_logits')
  loss = loss + weighted_sparse_ce(itm_logits, labels['itm_label_ids'], labels['itm_label_weights'])
  return loss
