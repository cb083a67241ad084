"""The one parity harness of the attention feature suites: a device call through `mmt_amd`, the dense fp64 oracle on
the same arrays, and the comparison against the standing bars of tests/_cases.py.

A feature file turns its case into dense side inputs (tests/_cases.py) plus the keyword arguments of the call, and
goes through device_call / oracle_call / check_against.  Results are dicts by tensor name: 'out', 'lse' (where the
forward API was used) and the gradients GRAD_NAMES."""
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


def assert_train_step_matches_oracle(model, loss, cpu_inputs, labels):
  """Loss and every parameter gradient of a model whose `loss.backward()` has run, against the float64 dense CPU oracle
  with autograd on copies of the same weights: loss ENC_TOL, gradients ENC_GRAD_TOL of each tensor's max."""
  from oracle import encoder as oenc
  sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
  ref_loss = oenc.pretraining_loss(sd, model.encoder.get_config(), cpu_inputs, {k: v.cpu() for k, v in labels.items()})
  ref_loss.backward()
  print(f'loss {float(loss):.6f} oracle {float(ref_loss):.6f}')
  assert abs(float(loss) - float(ref_loss)) < ENC_TOL
  for name, p in model.named_parameters():
    want = sd[name].grad
    if want is None:
      assert p.grad is None or float(p.grad.abs().max()) == 0, name
      continue
    got = p.grad.detach().cpu().double()
    err = float((got - want).abs().max()) / max(1e-3, float(want.abs().max()))
    assert err < ENC_GRAD_TOL, (name, err)


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
