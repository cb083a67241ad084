"""The train step as it is trained -- dropout on, bf16, `task.train_step` with micro-steps -- against the dense CPU oracle
(oracle/encoder.py) fed the keep masks the product drew.

The recorder (`tests._parity.DropoutSites`) notes seed and probability of every dropout site of the eager forward; the
oracle's restatements of the two mask generators (proven against the kernels at op level) turn them into masks.  fp32
cases hold the standing bars ENC_TOL / ENC_GRAD_TOL.  The bf16 bars are measured against the reference alone
(`tests._parity.storage_model_bars`): the float64 oracle with bf16 storage gives e_ref per tensor, the product must stay
below max(2 * e_ref, 2^-8), never above BF16_GRAD_TOL.  The bf16 and micro-step cases run on weights and batches made on
the CPU from seeds (`tests._parity.step_case`), so that tests/test_oracle_encoder.py checks on the host that the
reference alone stays under that ceiling on the very data of each case; the fp32 cases take the synthetic batch.
Tiny model (2 layers, H = 128, 2 heads, I = 512), S = 256, batch 2, ragged, band 32 + 8 global tokens unless a case says otherwise.  The heads' dropout_rate stays 0 (torch's generator)."""
import pytest
import torch

from tests._cases import ENC_GRAD_TOL
from tests._parity import (STEP_NUMBER, STEP_P_DROP as P_DROP, DropoutSites, assert_train_step_matches_oracle,
                           dense_inputs_cpu, oracle_micro_steps, oracle_train_step, restated_dropout_seeds, step_case,
                           storage_model_bars, tiny_experiment, train_step_errors)

pytestmark = pytest.mark.gpu

BAND = dict(radius=32, n_global=8)
DEV = torch.device('cuda:0')


def _setup(kw, *, dropout=True, dense=False, batch=2, seed=1):
  """(task, model, (inputs, labels), cpu inputs of the oracle, (B, S, H, N)) of an fp32 case on the synthetic batch."""
  import mmt_amd
  exp = tiny_experiment(S=256, **kw)
  enc = exp.task.model.encoder.mmt
  if dropout:
    enc.hidden_dropout_prob = enc.attention_probs_dropout_prob = P_DROP
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(seed)
  model = task.build_model().cuda()
  inputs, labels = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=batch, ragged=True,
                                          dense_side_inputs=dense))
  if dense:
    cpu = {k: v.cpu() for k, v in inputs.items() if torch.is_tensor(v)}
  else:
    cpu = dense_inputs_cpu(inputs, exp.task.train_data)
  cfg = model.encoder.get_config()
  dims = (batch, 256, cfg['hidden_size'], cfg['num_attention_heads'])
  return task, model, (inputs, labels), cpu, dims


def _forward_backward(task, model, batch, training=True):
  """One forward and backward as micro-step 0 of train step STEP_NUMBER would run it; the host epoch is put back afterwards."""
  from mmt_amd import fused, step_scalars
  inputs, labels = batch
  fused.set_seed_stream(STEP_NUMBER, 0, 0)
  try:
    loss = task.build_losses(labels, model(**inputs, training=training))
    loss.backward()
    torch.cuda.synchronize()
  finally:
    step_scalars.set_step(0)
  return loss.detach()


def _print_table(label, errs, e_ref=None, bars=None):
  for name in errs:
    if e_ref is None:
      print(f'{label} {name}: err {errs[name]:.3e}')
    else:
      print(f'{label} {name}: err {errs[name]:.3e} e_ref {e_ref[name]:.3e} bar {bars[name]:.3e}')


FP32_CASES = {'band-global': (BAND, False), '2d': (dict(core=2, R=49, **BAND), False), 'dense-pattern': (dict(), False),
              'dense-inputs': (BAND, True)}


@pytest.mark.parametrize('case', list(FP32_CASES))
def test_fp32_dropout_step_matches_oracle_fed_the_drawn_masks(case, monkeypatch):
  kw, dense = FP32_CASES[case]
  task, model, batch, cpu, dims = _setup(kw, dense=dense)
  sites = DropoutSites(monkeypatch)
  loss = _forward_backward(task, model, batch)
  masks = sites.masks(*dims, hidden_p=P_DROP, att_p=P_DROP)
  errs = assert_train_step_matches_oracle(model, loss, cpu, batch[1], masks=masks)
  _print_table(case, errs)


def test_oracle_fed_other_masks_misses_the_bars(monkeypatch):
  """The comparison can fail: masks of the seeds + 1 put a transformer-layer gradient more than 10x outside its bar."""
  task, model, batch, cpu, dims = _setup(BAND)
  sites = DropoutSites(monkeypatch)
  loss = _forward_backward(task, model, batch)
  wrong = sites.masks(*dims, hidden_p=P_DROP, att_p=P_DROP, seed_shift=1)
  errs = train_step_errors(model, loss, oracle_train_step(model, cpu, batch[1], masks=wrong))
  layer_errs = {k: v for k, v in errs.items() if '_transformer_layers' in k}
  worst = max(layer_errs, key=layer_errs.get)
  print(f'wrong masks: loss err {errs["loss"]:.3e}, worst {worst} {layer_errs[worst]:.3e}')
  assert layer_errs[worst] > 10 * ENC_GRAD_TOL
  with pytest.raises(AssertionError):
    assert_train_step_matches_oracle(model, loss, cpu, batch[1], masks=wrong)


def test_training_false_draws_no_mask(monkeypatch):
  """Dropout configured, `training=False`: no site is handed a probability, and the step is the no-dropout oracle's."""
  task, model, batch, cpu, dims = _setup(BAND)
  sites = DropoutSites(monkeypatch)
  loss = _forward_backward(task, model, batch, training=False)
  L = model.encoder.get_config()['num_hidden_layers']
  assert len(sites.seen) == 1 + 3 * L
  assert all(p == 0.0 for _, p, _, _ in sites.seen), sites.seen
  assert_train_step_matches_oracle(model, loss, cpu, batch[1])


class PathCounters:
  """Pass-through counters on the bf16-only paths: what `layers._ffn_ok` answered, the `.grad` buffers the weight-gradient
  kernels accepted (`fused.wgrad_accumulate_deferred_` / `fused.wgrad_accumulate_` returning true), and the operand
  shapes `torch.bmm` saw."""

  def __init__(self, monkeypatch):
    from mmt_amd import fused, layers
    self.ffn_ok, self.wgrad_ptrs, self.bmm_shapes = [], set(), []
    real_ok, real_def, real_now, real_bmm = layers._ffn_ok, fused.wgrad_accumulate_deferred_, fused.wgrad_accumulate_, torch.bmm

    def ffn_ok(*a):
      self.ffn_ok.append(real_ok(*a))
      return self.ffn_ok[-1]

    def wgrad(real):
      def f(dw, *a, **k):
        took = real(dw, *a, **k)
        if took:
          self.wgrad_ptrs.add(dw.data_ptr())
        return took
      return f

    def bmm(a, b, *rest, **k):
      self.bmm_shapes.append((tuple(a.shape), tuple(b.shape)))
      return real_bmm(a, b, *rest, **k)

    monkeypatch.setattr(layers, '_ffn_ok', ffn_ok)
    monkeypatch.setattr(fused, 'wgrad_accumulate_deferred_', wgrad(real_def))
    monkeypatch.setattr(fused, 'wgrad_accumulate_', wgrad(real_now))
    monkeypatch.setattr(torch, 'bmm', bmm)

  def assert_bf16_paths_ran(self, model, sites):
    blocks = model.encoder.transformer_layers.layers
    assert self.ffn_ok == [True] * len(blocks), self.ffn_ok                 # the GELU' GEMM epilogue path, every block
    for i, block in enumerate(blocks):
      took = [n for n, p in block.named_parameters() if p.grad is not None and p.grad.data_ptr() in self.wgrad_ptrs]
      assert took, f'no weight-gradient kernel accepted a product of block {i}'
    assert sites.sinks and all(sites.sinks), sites.sinks                    # fp32 table gradients through the sinks


def _setup_step_case(case, dtype, dropout=True):
  """(task, model, (inputs, labels), cpu inputs of the oracle, (B, S, H, N)) of a hand-made case (`tests._parity.step_case`):
  made on the CPU, so the host tests size the bf16 bars on these very weights, inputs and masks."""
  task, model, (inputs, labels), data_cfg = step_case(case, dtype, dropout)
  cpu = dense_inputs_cpu(inputs, data_cfg)
  model = model.cuda()
  assert all(p.dtype == torch.float32 for p in model.parameters())          # fp32 masters in either compute dtype
  inputs = {k: v.cuda() if torch.is_tensor(v) else v for k, v in inputs.items()}
  labels = {k: v.cuda() for k, v in labels.items()}
  cfg = model.encoder.get_config()
  return task, model, (inputs, labels), cpu, (len(cpu['word_ids']), 256, cfg['hidden_size'], cfg['num_attention_heads'])


def _assert_within_storage_model_bars(label, model, loss, ref64, ref_store):
  """The product against the float64 oracle, every error below the bar the storage model gives that tensor."""
  e_ref, bars = storage_model_bars(ref64, ref_store)
  errs = train_step_errors(model, loss, ref64)
  errs['loss'] /= max(1e-3, abs(ref64[0]))
  _print_table(label, errs, e_ref, bars)
  assert errs.keys() == bars.keys()
  missed = {k: (errs[k], e_ref[k], bars[k]) for k in errs if not errs[k] < bars[k]}
  assert not missed, missed


@pytest.mark.parametrize('dropout', [False, True], ids=['no-dropout', 'dropout'])
@pytest.mark.parametrize('case', ['band-global', '2d', 'vocab-8193'])
def test_bf16_step_matches_oracle_within_the_storage_model_bars(case, dropout, monkeypatch):
  """One forward and backward in bf16 against the float64 oracle, every tensor below the bar its storage-model error gives.

  Closest to its bar (MI355X, the measured table is in DESIGN.md section 2): [band-global-dropout],
  `layers.1.ffn_layer_norm.weight`, product error 1.299e-2 of the tensor's max, e_ref 6.637e-3, bar 1.327e-2.  If a
  tensor misses, read the product for the storage point the model lacks and add it to the oracle's `store` mode with the
  line it restates (as P ahead of the keep scaling, the gradient of the scores and the ITM head's kept tanh result
  are); the factor, the floor and the ceiling stay."""
  task, model, batch, cpu, dims = _setup_step_case(case, torch.bfloat16, dropout)
  L = model.encoder.get_config()['num_hidden_layers']
  sites, paths = DropoutSites(monkeypatch), PathCounters(monkeypatch)
  loss = _forward_backward(task, model, batch)
  paths.assert_bf16_paths_ran(model, sites)
  vocab = model.encoder.get_config()['vocab_size']
  if case == 'vocab-8193':                      # V = 3 x 2731 >= 8192: the tied logits' dgrad as three K slices
    M, H = batch[0]['mlm_positions'].numel(), dims[2]
    assert ((3, M, vocab // 3), (3, vocab // 3, H)) in paths.bmm_shapes, paths.bmm_shapes
  if dropout:
    masks = sites.masks(*dims, hidden_p=P_DROP, att_p=P_DROP)
    assert [e[2] for e in sites.seen] == restated_dropout_seeds(STEP_NUMBER, 0, 0, L)
  else:
    masks = None
    assert len(sites.seen) == 1 + 3 * L and all(p == 0.0 for _, p, _, _ in sites.seen)
  ref64 = oracle_train_step(model, cpu, batch[1], masks=masks)
  ref_store = oracle_train_step(model, cpu, batch[1], masks=masks, store=torch.bfloat16)
  _assert_within_storage_model_bars(f'{case} {"dropout" if dropout else "no-dropout"}', model, loss, ref64, ref_store)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_train_step_with_two_micro_steps_matches_oracle(dtype, monkeypatch):
  """`task.train_step`, batch 4 as two micro-steps of 2, step 7: the gradients left in `.grad` are the sum over the two
  slices of the oracle gradient of loss_i times the factor train_step applies, each slice under the masks its micro-step
  drew; the returned loss is the mean of the two."""
  from mmt_amd import step_scalars
  task, model, batch, cpu, dims = _setup_step_case('micro-steps', dtype)
  dims = (2,) + dims[1:]
  L = model.encoder.get_config()['num_hidden_layers']
  before = {k: v.detach().clone() for k, v in model.named_parameters()}
  opt = torch.optim.SGD(model.parameters(), lr=0.0)                         # parameters stay put, .grad survives the step
  sites = DropoutSites(monkeypatch)

  def step(n):
    del sites.seen[:]
    out = task.train_step(batch, model, opt, micro_batch_size=2, clip_norm=None, reducer=None, step=n)
    torch.cuda.synchronize()
    assert step_scalars.host_epoch(DEV) == 0
    return float(out['loss']), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

  loss, grads = step(STEP_NUMBER)
  forwards = sites.forwards(L)
  assert len(forwards) == 2 and len(sites.seen) == 2 * (1 + 3 * L)
  seeds = [[e[2] for e in f] for f in forwards]
  assert not set(seeds[0]) & set(seeds[1]), 'micro-step 1 reuses seeds of micro-step 0'
  assert seeds == [restated_dropout_seeds(STEP_NUMBER, i, 0, L) for i in range(2)]

  # tasks.py train_step: scale_loss differentiates loss / num_replicas, else loss / num_small_steps
  num_small_steps, num_replicas = 2, task.num_replicas
  factor = 1.0 / num_replicas if task.task_config.scale_loss else 1.0 / num_small_steps
  masks = [sites.masks(*dims, hidden_p=P_DROP, att_p=P_DROP, entries=entries) for entries in forwards]
  ref64 = oracle_micro_steps(model, cpu, batch[1], masks, 2, factor)
  if dtype == torch.float32:
    errs = assert_train_step_matches_oracle(model, loss, None, None, ref=ref64)
    _print_table('micro-steps f32', errs)
  else:
    ref_store = oracle_micro_steps(model, cpu, batch[1], masks, 2, factor, store=torch.bfloat16)
    _assert_within_storage_model_bars('micro-steps bf16', model, loss, ref64, ref_store)
  for k, p in model.named_parameters():
    assert torch.equal(p.detach(), before[k]), k

  # the seeds are a pure function of (step, micro-step, rank, site): the same step again draws the same masks
  seen7 = list(sites.seen)
  loss_again, grads_again = step(STEP_NUMBER)
  assert sites.seen == seen7 and loss_again == loss
  assert grads.keys() == grads_again.keys()
  for k in grads:
    assert torch.equal(grads[k], grads_again[k]), k
  step(STEP_NUMBER + 1)
  assert not {e[2] for e in sites.seen} & {e[2] for e in seen7}
