"""The one parity harness of the attention feature suites: a device call through `mmt_amd`, the dense fp64 oracle on
the same arrays, and the comparison against the standing bars of tests/_cases.py.

A feature file turns its case into dense side inputs (tests/_cases.py) plus the keyword arguments of the call, and
goes through device_call / oracle_call / check_against.  Results are dicts by tensor name: 'out', 'lse' (where the
forward API was used) and the gradients GRAD_NAMES.

Below the attention harness: the tiny models, and the train-step comparison against oracle/encoder.py -- hand-made cases,
the recorder of the dropout sites, the oracle's step and the bf16 bars measured on the storage model."""
import numpy as np
import torch

from oracle import attention as oa
from oracle import side_inputs as si
from tests._cases import ENC_GRAD_TOL, ENC_TOL, grad_error, grad_tol, out_tol, pair_tol

GRAD_NAMES = ('dq', 'dk', 'dv', 'drel_emb', 'drel_bias')
ACCUM_SEED = {'drel_emb': 0.25, 'drel_bias': -0.5}      # what the rel_grads_accum buffers hold before the call


def make_pattern(*, radius=1 << 30, g0=0, ng=0, id_mode=1, m=3, P=0, r=0, a=0, g=2, gidx=None):
  import mmt_amd
  return mmt_amd.AttentionPattern(local_radius=radius, global_start=g0, n_global=ng, id_mode=id_mode, max_dist=m,
                                  patches_per_row=P, core_layers=r, global_index=gidx, grid_radius=a, grid_start=g)


def tuning_bits():
  from mmt_amd import _lib
  return {n: getattr(_lib, n) for n in dir(_lib) if n.startswith('MMT_TUNE_')}


def to_dev(x, dtype):
  return None if x is None else torch.from_numpy(x).cuda().to(dtype).contiguous()


def device_call(arrays, dtype, *, backward=True, accum=False, **call_kw):
  """One call on the device with `call_kw` handed through unchanged.  backward: `relative_attention` and autograd, giving
  out and the gradients; else `relative_attention_forward`, giving out and lse.  accum (MMT_FLAG_ACCUM_REL_GRADS): a
  second, explicit backward adds the table gradients onto buffers holding ACCUM_SEED, and those buffers are returned
  as drel_emb / drel_bias.  fp32 tensors on the device."""
  import mmt_amd
  q, k, v, emb, bias, dout = arrays
  ts = [None if x is None else to_dev(x, dtype).requires_grad_(backward) for x in (q, k, v, emb, bias)]
  if not backward:
    out, lse = mmt_amd.relative_attention_forward(*ts, **call_kw)
    torch.cuda.synchronize()
    return {'out': out.float(), 'lse': lse}
  out = mmt_amd.relative_attention(*ts, **call_kw)
  if accum:
    bufs = [None if t is None else torch.full(t.shape, ACCUM_SEED[n], dtype=torch.float32, device='cuda')
            for n, t in zip(GRAD_NAMES[3:], ts[3:])]
    det = [None if t is None else t.detach() for t in ts]
    lse = mmt_amd.relative_attention_forward(*det, **call_kw)[1]
    mmt_amd.relative_attention_backward(to_dev(dout, dtype), *det, out.detach(), lse, rel_grads_accum=tuple(bufs), **call_kw)
  out.backward(to_dev(dout, dtype))
  torch.cuda.synchronize()
  got = {'out': out.detach().float()}
  got.update({n: t.grad.float() for n, t in zip(GRAD_NAMES, ts) if t is not None})
  if accum:
    got.update({n: b for n, b in zip(GRAD_NAMES[3:], bufs) if b is not None})
  return got


def dropout_seed_rule(seed):
  """The seed the kernels mix for a call made with `dropout_seed=seed` outside a captured step: the host's epoch added."""
  from mmt_amd import step_scalars
  dev = torch.device('cuda:0')
  assert step_scalars.epoch_ptr(dev) is None
  return (seed + step_scalars.host_epoch(dev)) & (2**64 - 1)


def oracle_call(arrays, mask, ids, *, scale_before_add=False, dropout=None, backward=True):
  """The dense oracle on the arrays of the device call: out, lse and (backward) the gradients the call has.  dropout =
  (p, seed of the call): the oracle is fed the restated keep mask."""
  q, k, v, emb, bias, dout = arrays
  okw = dict(scale_after_add=not scale_before_add)
  if dropout:
    B, S, N, _ = q.shape
    keep, keep_prob = oa.dropout_keep_mask(B, N, S, dropout[0], dropout_seed_rule(dropout[1]))
    okw.update(keep_mask=keep, keep_prob=keep_prob)
  out, lse = oa.relative_attention_fwd(q, k, v, emb, bias, mask, ids, **okw)
  ref = {'out': out, 'lse': lse}
  if backward:
    grads = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, ids, **okw)
    ref.update({n: g for n, g in grads.items() if g is not None})
  return ref


def _numpy(x):
  return x.detach().float().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def check_against(got, ref, dtype, label='', seed_grads=None):
  """Every tensor of `got` against `ref` (+ seed_grads) and the standing bars; returns the measured errors by name.
  `got` must hold exactly the tensors of `ref` -- lse alone may be left out (the autograd path does not return it) -- so
  that a gradient the call should have produced, or one it should not, cannot pass by not being compared."""
  assert set(got) | {'lse'} == set(ref) | {'lse'}, f'{label} compared {sorted(got)}, expected {sorted(ref)}'
  errs = {}
  for name in got:
    g, w = _numpy(got[name]), ref[name] + (seed_grads or {}).get(name, 0.0)
    assert g.shape == w.shape, (label, name, g.shape, w.shape)
    assert np.isfinite(g).all(), f'{label} {name}: not finite'
    if name in ('out', 'lse'):
      err, bar, what = np.abs(g - w).max(), out_tol(dtype), 'max abs err'
    else:
      err, bar = grad_error(g, w, dtype), grad_tol(dtype)
      what = 'max abs err' if dtype == torch.float32 else 'max err relative to max |grad|'
    print(f'{label} {name}: {what} {err:.3e}')
    assert err < bar, f'{label} {name}: {what} {err}'
    errs[name] = err
  return errs


def assert_structured_equals_dense_under_dropout(arrays, dtype, structured_kw, dense_kw, *, seed=1234, p=0.1,
                                                 standing_bars=False):
  """The structured call and the dense operator on the materialised side inputs draw the same keep mask (same seed) and
  agree in the output and every gradient: error / max(1, max |dense|) below pair_tol; with standing_bars the absolute
  output bar and the gradient bars of the oracle cases instead."""
  a, b = (device_call(arrays, dtype, dropout_p=p, dropout_seed=seed, **kw) for kw in (structured_kw, dense_kw))
  assert set(a) == set(b) == {'out', *GRAD_NAMES}
  for name in a:
    x, y = _numpy(a[name]), _numpy(b[name])
    if not standing_bars:
      err, bar = np.abs(x - y).max() / max(1.0, np.abs(y).max()), pair_tol(dtype)
    elif name == 'out':
      err, bar = np.abs(x - y).max(), out_tol(dtype)
    else:
      err, bar = grad_error(x, y, dtype), grad_tol(dtype)
    print(f'{name}: {err:.3e}')
    assert err < bar, (name, err)


# ---- tiny models -----------------------------------------------------------------------------------------------------
def tiny_experiment(S=256, image=224, m=12, R=32, core=0, radius=1 << 30, n_global=0, pre=True):
  from mmt_amd import configs
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'task': {
      'model': {'encoder': {'mmt': dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
                                        intermediate_size=512, vocab_size=2000, relative_vocab_size=R,
                                        relative_pos_max_distance=m, relative_att_num_core_layers=core,
                                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                        use_pre_activation_order=pre)},
                'cls_heads': [{'inner_dim': 128, 'num_classes': 2, 'name': 'itm'}]},
      'train_data': dict(max_seq_len=S, image_size=image, patch_size=16, relative_pos_max_distance=m,
                         relative_att_num_core_layers=core, mlm_max_selections_per_seq=8,
                         mpp_max_selections_per_seq=6, local_radius=radius, num_global_tokens=n_global,
                         tasks='mlm,itm')}})
  return exp


def dense_inputs_cpu(inputs, data_cfg):
  """CPU copies + the dense [B,S,S] side inputs the reference would feed (from the oracle)."""
  S = data_cfg.max_seq_len
  out = {k: v.detach().cpu() for k, v in inputs.items() if torch.is_tensor(v)}
  pat = inputs.get('attention_pattern')
  if pat is not None:
    vl = inputs['valid_len'].cpu().tolist()
    out['att_mask'] = torch.tensor(np.stack([si.sparse_pattern_mask(S, v, min(pat.local_radius, S), pat.global_start,
                                                                     pat.n_global) for v in vl]))
    if pat.id_mode:
      ids = si.relative_ids_from_desc(S, pat.id_mode, pat.max_dist, pat.patches_per_row, pat.core_layers)
      out['relative_att_ids'] = torch.tensor(ids)[None].expand(len(vl), S, S)
  return out


# ---- hand-made train-step cases --------------------------------------------------------------------------------------
# Model and batch are made on the CPU from seeds, so that the host tests (tests/test_oracle_encoder.py) size the bf16
# bars on the very weights, inputs and keep masks of the GPU cases (tests/test_gpu_train_step_oracle.py).
# name -> (tiny_experiment keywords, vocabulary size, valid lengths, seed of the inputs).  The seeds are chosen: every
# gradient flows through 8 + 6 + 1 head rows per example, so the storage model's worst tensor lands between 1e-2 and 2e-2
# of its maximum depending on the draw (far more when the two examples' ITM terms cancel), and the bf16 bars need
# 2 * that under BF16_GRAD_TOL.
STEP_CASES = {
    'band-global': (dict(), 2000, (256, 231), 4),
    '2d': (dict(core=2, R=49), 2000, (256, 231), 4),
    'vocab-8193': (dict(), 8193, (256, 231), 8),            # 8193 = 3 x 2731: the tied logits' three-slice dgrad
    'micro-steps': (dict(), 2000, (256, 231, 243, 250), 2),
}
STEP_P_DROP = 0.1
STEP_NUMBER = 7                 # the train step whose masks the cases draw


def step_case(case, dtype=torch.float32, dropout=True, pre=True):
  """(task, model on the CPU with fp32 masters, (inputs, labels)) of a hand-made case: the tiny model at S = 256, band 32 +
  8 global tokens at 198, ragged valid lengths, 8 MLM and 6 MPP positions per example; structured side inputs
  (`dense_inputs_cpu` gives the oracle's).  Biases and LayerNorm weights are moved off their initial 0 / 1."""
  import mmt_amd
  from mmt_amd import input_utils
  kw, vocab, valid, seed = STEP_CASES[case]
  S, n_img = 256, 198
  exp = tiny_experiment(S=S, radius=32, n_global=8, pre=pre, **kw)
  enc = exp.task.model.encoder.mmt
  enc.vocab_size = vocab
  if dropout:
    enc.hidden_dropout_prob = enc.attention_probs_dropout_prob = STEP_P_DROP
  task = mmt_amd.tasks.get_task(exp.task, compute_dtype=dtype)
  torch.manual_seed(1)
  model = task.build_model()
  g = torch.Generator().manual_seed(seed)
  with torch.no_grad():
    for p in model.parameters():
      if p.dim() == 1:
        p.add_(0.05 * torch.randn(p.shape, generator=g))
  B = len(valid)
  ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int32)
  vl = torch.tensor(valid, dtype=torch.int32)
  word_ids = ri(1000, vocab, (B, S))
  inputs = {
      'word_ids': torch.where(torch.arange(S)[None] < vl[:, None], word_ids, torch.zeros_like(word_ids)),
      'segment_ids': torch.tensor(np.stack([si.make_segment_ids(n_img, v - n_img, S) for v in valid])),
      'patch_embeddings': torch.randn(B, n_img - 2, 768, generator=g),
      'mlm_positions': ri(n_img + 1, min(valid), (B, 8)),
      'mpp_positions': ri(2, n_img, (B, 6)),
      'attention_pattern': input_utils.attention_pattern_from_config(exp.task.train_data),
      'valid_len': vl,
  }
  mlm_w = torch.ones(B, 8)
  mlm_w[1, 6:] = 0                             # unused selection slots carry weight 0
  labels = {
      'mlm_label_ids': ri(0, vocab, (B, 8)), 'mlm_label_weights': mlm_w,
      'mpp_label_ids': ri(0, model.masked_pp.bias.shape[0], (B, 6)), 'mpp_label_weights': torch.ones(B, 6),
      'itm_label_ids': ri(0, 2, (B,)), 'itm_label_weights': torch.ones(B),
  }
  return task, model, (inputs, labels), exp.task.train_data


def restated_dropout_seeds(step, micro_step, rank, L):
  """The effective seeds of one eager forward pass in site order (embed, then per layer att, h1, h2), restated from the
  rule "a pure function of (train step, micro-step, rank, site)": the stream of `fused.set_seed_stream` / `next_seed`,
  the `>> 24` of `MmtEncoder.forward`, `dropout_seed * 131 + layer` of the attention sites, and the step's epoch
  (`step_scalars.epoch_of`) added where the descriptors are filled in."""
  m63, m64 = (1 << 63) - 1, (1 << 64) - 1
  base = ((micro_step * 0xC2B2AE3D27D4EB4F) ^ ((rank + 1) * 0x165667B19E3779F9)) & m63
  nth = lambda n, b=0: (base + b * 0x9E3779B97F4A7C15 + n * 0xD1B54A32D192ED03) & m63
  epoch = (step * 0x9E3779B97F4A7C15) & m64
  layers_seed = nth(2) >> 24
  seeds = [nth(1)]
  for l in range(L):
    seeds += [layers_seed * 131 + l, nth(3 + 2 * l, layers_seed), nth(4 + 2 * l, layers_seed)]
  return [(s + epoch) & m64 for s in seeds]


def keep_masks_from_seeds(seeds, B, S, H, N, hidden_p, att_p):
  """The `masks` dict of oracle.encoder from the effective seeds of one forward pass in site order, through the oracle's
  two keep-mask restatements (the ops are proven against exactly these at op level)."""
  from oracle import layer_ops as lo
  def hidden(seed):
    keep, inv_keep = lo.dropout_keep_mask(B * S, H, hidden_p, seed)
    return torch.from_numpy(keep).view(B, S, H), 1.0 / inv_keep
  def probs(seed):
    keep, keep_prob = oa.dropout_keep_mask(B, N, S, att_p, seed)
    return torch.from_numpy(keep), keep_prob
  L = (len(seeds) - 1) // 3
  return {'embed': hidden(seeds[0]), 'att': [probs(seeds[1 + 3 * l]) for l in range(L)],
          'h1': [hidden(seeds[2 + 3 * l]) for l in range(L)], 'h2': [hidden(seeds[3 + 3 * l]) for l in range(L)]}


class DropoutSites:
  """Records the dropout sites of the eager model: wraps `fused.embed_assemble`, `fused.residual_block` and
  `ops.relative_attention_qkv` (looked up through their modules at call time by encoder.py / layers.py) and passes
  everything through.  One entry per call in `seen`: (kind, p, effective seed, shape of the call's leading tensor),
  kind 'embed' | 'att' | 'res'.  The effective seed is what the kernels mix: the call's seed plus the host's epoch AT
  CALL TIME (`train_step` resets the epoch when it returns).  `sinks` holds, per 'att' call, whether `rel_grad_sinks`
  was set."""

  def __init__(self, monkeypatch):
    from mmt_amd import fused, ops, step_scalars
    self.seen, self.sinks = [], []

    def effective(seed, device):
      assert step_scalars.epoch_ptr(device) is None, 'the recorder restates the host epoch: eager steps only'
      return (int(seed) + step_scalars.host_epoch(device)) & (2**64 - 1)

    real_embed, real_res, real_att = fused.embed_assemble, fused.residual_block, ops.relative_attention_qkv

    def embed(word_ids, *a, **k):
      self.seen.append(('embed', float(k.get('p', 0.0)), effective(k.get('seed', 0), word_ids.device), tuple(word_ids.shape)))
      return real_embed(word_ids, *a, **k)

    def res(o, bias, x, gamma=None, beta=None, eps=1e-12, p=0.0, seed=0):
      self.seen.append(('res', float(p), effective(seed, x.device), tuple(x.shape)))
      return real_res(o, bias, x, gamma, beta, eps, p, seed)

    def att(qkv, rel_emb=None, rel_bias=None, rel_grad_sinks=None, **kw):
      self.seen.append(('att', float(kw.get('dropout_p', 0.0)), effective(kw.get('dropout_seed', 0), qkv.device),
                        tuple(qkv.shape)))
      self.sinks.append(rel_grad_sinks is not None)
      return real_att(qkv, rel_emb, rel_bias, rel_grad_sinks=rel_grad_sinks, **kw)

    monkeypatch.setattr(fused, 'embed_assemble', embed)
    monkeypatch.setattr(fused, 'residual_block', res)
    monkeypatch.setattr(ops, 'relative_attention_qkv', att)

  def forwards(self, L):
    """`seen` split into forward passes of 1 + 3 * L sites each."""
    n = 1 + 3 * L
    assert len(self.seen) % n == 0, (len(self.seen), n)
    return [self.seen[i:i + n] for i in range(0, len(self.seen), n)]

  def masks(self, B, S, H, N, *, hidden_p, att_p, entries=None, seed_shift=0):
    """The `masks` dict of oracle.encoder for ONE forward pass (`entries`, default all of `seen`), through the oracle's
    two keep-mask restatements -- the ops are proven against exactly these at op level.  Asserts the order (one embed,
    then per layer att, h1, h2), the count, the shapes, that all effective seeds differ and that every p is the configured
    one.  `seed_shift` is added to every seed: the masks the product did NOT draw."""
    entries = self.seen if entries is None else entries
    assert (len(entries) - 1) % 3 == 0 and len(entries) >= 4, len(entries)
    L = (len(entries) - 1) // 3
    assert [e[0] for e in entries] == ['embed'] + ['att', 'res', 'res'] * L, [e[0] for e in entries]
    seeds = [e[2] for e in entries]
    assert len(set(seeds)) == len(seeds), 'two dropout sites share an effective seed'
    for kind, p, _, shape in entries:
      assert p == (att_p if kind == 'att' else hidden_p), (kind, p)
      assert shape == {'embed': (B, S), 'res': (B, S, H)}.get(kind, shape) and shape[:2] == (B, S), (kind, shape)
      assert kind != 'att' or shape[2:4] == (3, N), shape
    return keep_masks_from_seeds([(s + seed_shift) & (2**64 - 1) for s in seeds], B, S, H, N, hidden_p, att_p)


def oracle_train_step(model, cpu_inputs, labels, masks=None, store=None):
  """(loss, {parameter name: gradient | None}) of the dense CPU oracle with autograd on float64 copies of the model's
  weights; `masks` / `store` as oracle.encoder."""
  from oracle import encoder as oenc
  sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
  ref_loss = oenc.pretraining_loss(sd, model.encoder.get_config(), cpu_inputs, {k: v.cpu() for k, v in labels.items()},
                                   masks=masks, store=store)
  ref_loss.backward()
  return float(ref_loss.detach()), {k: v.grad for k, v in sd.items()}


def oracle_micro_steps(model, cpu_inputs, labels, masks_per_step, micro, factor, store=None):
  """The reference of `train_step` with micro-steps of `micro` examples: (mean of the slices' oracle losses, sum over the
  slices of `factor` x the oracle gradient of that slice's loss under that micro-step's masks)."""
  n = len(masks_per_step)
  ref_loss, ref_grads = 0.0, None
  for i, masks in enumerate(masks_per_step):
    sl = slice(i * micro, (i + 1) * micro)
    li, gi = oracle_train_step(model, {k: v[sl] for k, v in cpu_inputs.items()}, {k: v[sl] for k, v in labels.items()},
                               masks=masks, store=store)
    ref_loss += li / n
    gi = {k: None if g is None else g * factor for k, g in gi.items()}
    ref_grads = gi if ref_grads is None else {k: None if g is None else ref_grads[k] + g for k, g in gi.items()}
  return ref_loss, ref_grads


def train_step_errors(model, loss, ref):
  """{'loss': |loss - oracle|, name: max |grad - oracle| / max(1e-3, max |oracle|)} of a model whose backward has run
  against ref = (loss, gradients by name); a parameter the oracle gives no gradient must have none or zeros."""
  ref_loss, ref_grads = ref
  errs = {'loss': abs(float(loss) - ref_loss)}
  for name, p in model.named_parameters():
    want = ref_grads[name]
    if want is None:
      assert p.grad is None or float(p.grad.abs().max()) == 0, name
      continue
    assert p.grad is not None, name
    got = p.grad.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), name
    errs[name] = float((got - want).abs().max()) / max(1e-3, float(want.abs().max()))
  return errs


def assert_train_step_matches_oracle(model, loss, cpu_inputs, labels, masks=None, store=None, loss_tol=ENC_TOL,
                                     grad_tol=ENC_GRAD_TOL, ref=None):
  """Loss and every parameter gradient of a model whose `loss.backward()` has run, against the float64 dense CPU oracle
  with autograd on copies of the same weights: loss ENC_TOL, gradients ENC_GRAD_TOL of each tensor's max.  `masks` /
  `store` go to the oracle; `ref` = (loss, gradients by name) is a reference computed beforehand (several micro-steps);
  `grad_tol` may be a dict by parameter name.  Returns the errors (`train_step_errors`)."""
  if ref is None:
    ref = oracle_train_step(model, cpu_inputs, labels, masks, store)
  print(f'loss {float(loss):.6f} oracle {ref[0]:.6f}')
  errs = train_step_errors(model, loss, ref)
  assert errs['loss'] < loss_tol, ('loss', errs['loss'], loss_tol)
  for name, err in errs.items():
    if name != 'loss':
      bar = grad_tol[name] if isinstance(grad_tol, dict) else grad_tol
      assert err < bar, (name, err, bar)
  return errs


def storage_model_bars(ref64, ref_store):
  """The bf16 bars of the train-step tests, measured against the reference alone: for the loss and every gradient
  e_ref = |storage model - float64 oracle| / max(1e-3, max |float64 oracle|) and
  bar = min(max(2 * e_ref, 2^-8), BF16_GRAD_TOL): factor 2 because the product rounds at the model's points but draws
  other rounding errors, 2^-8 one bf16 ulp of the tensor's maximum, the ceiling the standing bf16 gradient bar.
  Returns (e_ref, bar), both by name with 'loss' among them."""
  from tests._cases import BF16_GRAD_TOL
  e_ref = {'loss': abs(ref_store[0] - ref64[0]) / max(1e-3, abs(ref64[0]))}
  for name, want in ref64[1].items():
    if want is not None:
      e_ref[name] = float((ref_store[1][name] - want).abs().max()) / max(1e-3, float(want.abs().max()))
  return e_ref, {k: min(max(2 * e, 2.0 ** -8), BF16_GRAD_TOL) for k, e in e_ref.items()}


def assert_runs_agree(runs):
  """Two runs of one model, each (loss, sequence output | None, {parameter name: gradient}): the bars above."""
  (l0, s0, g0), (l1, s1, g1) = runs
  assert abs(l0 - l1) < ENC_TOL
  if s0 is not None:
    assert float((s0 - s1).abs().max()) < ENC_TOL
  assert g0.keys() == g1.keys()
  for name in g0:
    err = float((g0[name] - g1[name]).abs().max()) / max(1e-3, float(g1[name].abs().max()))
    assert err < ENC_GRAD_TOL, (name, err)
