"""LAMB on the GPU (csrc/lamb.hip through mmt_amd/optimization.py `FusedLamb`): the three kernels against the float64 oracle
of tests/_lamb_cases.py within its bound; the same bits whatever the slab layout, on every run, with the step scalars
in device memory and replayed from a HIP graph; and the trainer loop with `optimizer_type=lamb`."""
import numpy as np
import pytest
import torch

from tests import _lamb_cases as C

pytestmark = pytest.mark.gpu


def _named():
  params, _ = C.inputs()
  return [(n, torch.nn.Parameter(torch.from_numpy(params[n].copy()).cuda())) for n in C.NAMES]


def _run(bucket_mb=48.0, steps=C.STEPS, device_scalars=False, check=None, given_scales=None):
  """`steps` FusedLamb steps on the test model with the reducer's clip factor as grad_scale (or `given_scales`, floats).
  Returns the optimizer, the named parameters and the clip factors; `check(step, opt, named)` runs after every step."""
  from mmt_amd import distribute, optimization, step_scalars
  named = _named()
  reducer = distribute.DataParallelStrategy(None, bucket_mb=bucket_mb).make_reducer([p for _, p in named])
  opt = optimization.FusedLamb(named, C.optimizer_config(), reducer)
  _, grads = C.inputs()
  scales = []
  for step in range(steps):
    reducer.zero_grad()
    for n, p in named:
      p.grad.copy_(torch.from_numpy(grads[step][n].copy()))
    scale = reducer.clip_by_global_norm(C.CLIP, apply=False)
    if given_scales is not None:
      scale = torch.tensor(given_scales[step], dtype=torch.float32, device='cuda')
    scales.append(float(scale))
    if device_scalars:
      sc = step_scalars.DeviceStepScalars(torch.device('cuda', torch.cuda.current_device()))
      sc.enable()
      try:
        sc.write(step + 1, C.LR, opt.t + 1, C.BETA_1, C.BETA_2)
        optimization.set_learning_rate(opt, 123.0)                  # the descriptor's own scalars must not be read
        opt.step(grad_scale=scale)
      finally:
        sc.disable()
        optimization.set_learning_rate(opt, C.LR)
    else:
      opt.step(grad_scale=scale)
    if check is not None:
      check(step, opt, named)
  return opt, named, scales


def _state(opt, named):
  """name -> (param, m, v) clones, read through the reducer's layout."""
  names = {p: n for n, p in named}
  out = {}
  for p, gi, off in opt.reducer.layout:
    s = opt.slabs[gi]
    k = p.numel()
    out[names[p]] = (p.detach().clone(), s['m'][off:off + k].clone(), s['v'][off:off + k].clone())
  return out


def test_fused_lamb_matches_the_oracle():
  from mmt_amd import optimization
  want = C.oracle()
  worst = {'param': 0.0, 'm': 0.0, 'v': 0.0}

  def check(step, opt, named):
    st = _state(opt, named)
    for i, key in enumerate(('param', 'm', 'v')):
      worst[key] = max(worst[key], C.max_error({n: st[n][i] for n in C.NAMES}, want[step][i]))
    pad = [torch.ones(s['param'].numel(), dtype=torch.bool, device='cuda') for s in opt.slabs]
    for p, gi, off in opt.reducer.layout:
      pad[gi][off:off + p.numel()] = False
      assert torch.equal(p._mmt_shadow, p.detach().to(torch.bfloat16))
      assert float(p.grad.abs().max()) == 0.0
    for s, mask in zip(opt.slabs, pad):
      assert int(mask.sum()) > 0
      for key in ('param', 'm', 'v', 'grad'):
        assert not bool(s[key][mask].any()), key                    # every padding element still exactly zero
      assert not bool(s['shadow'][mask].any())

  opt, named, scales = _run(check=check)
  assert isinstance(opt, optimization.FusedLamb) and len(opt.slabs) == 1 and opt.slabs[0]['n_segments'] == len(C.NAMES)
  print('FusedLamb: max |ours - oracle| =', worst, 'clip factors', scales)
  assert max(scales) < 1.0 and abs(scales[1] - want[1][3]) < 1e-6 * want[1][3] + 1e-9
  assert max(worst.values()) < C.BOUND
  # create_optimizer gives this class under the condition that gives FusedAdamW
  from mmt_amd import distribute
  m = torch.nn.Linear(8, 8).cuda()
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(m.parameters()))
  assert type(optimization.create_optimizer(m, C.optimizer_config(), reducer=reducer)) is optimization.FusedLamb
  assert type(optimization.create_optimizer(m, C.optimizer_config())) is optimization.Lamb


def test_results_do_not_depend_on_the_slab_layout_or_the_run():
  """Every parameter in a bucket of its own (or nearly) against all in one slab, and a second fresh run: the same bits.
  The slab runs are handed the first run's clip factors: mmt_grad_clip_scale adds the gradients in an order that follows
  the bucket layout, so its factor may differ in the last bit between layouts, which is not LAMB's business."""
  opt1, named1, scales = _run()
  one = _state(opt1, named1)
  optn, namedn, _ = _run(bucket_mb=0.01, given_scales=scales)
  assert len(optn.slabs) == 4 and len(opt1.slabs) == 1       # 10 KB buckets: {zero, one, exact}, {wide}, {beta, gamma, bias}, {dense/kernel}
  many = _state(optn, namedn)
  opt2, named2, scales2 = _run()
  assert scales2 == scales
  again = _state(opt2, named2)
  for n in C.NAMES:
    for a, b, c in zip(one[n], many[n], again[n]):
      assert torch.equal(a, b), n
      assert torch.equal(a, c), n


def test_step_scalars_in_device_memory_equal_the_descriptor():
  opt1, named1, _ = _run()
  opt2, named2, _ = _run(device_scalars=True)
  a, b = _state(opt1, named1), _state(opt2, named2)
  for n in C.NAMES:
    for x, y in zip(a[n], b[n]):
      assert torch.equal(x, y), n


def _tiny_graphed(eager: bool):
  from tests._parity import tiny_experiment
  from mmt_amd import graphed, optimization, tasks, distribute
  exp = tiny_experiment(S=256, radius=32, n_global=8)
  exp.override({'task': {'model': {'encoder': {'mmt': {'hidden_dropout_prob': 0.1, 'attention_probs_dropout_prob': 0.1}}},
                         'micro_batch_size': 2},
                'trainer': {'optimizer_config': {'optimizer_type': 'lamb', 'initial_learning_rate': 1e-3}}})
  task = tasks.PretrainingTask(exp.task, compute_dtype=torch.bfloat16, num_replicas=1)
  torch.manual_seed(0)
  model = task.build_model().cuda()
  opt_cfg = exp.trainer.optimizer_config
  reducer = distribute.DataParallelStrategy(None).make_reducer(list(model.parameters()))
  optimizer = optimization.create_optimizer(model, opt_cfg, reducer=reducer)
  assert isinstance(optimizer, optimization.FusedLamb)
  batch = next(task.build_inputs(exp.task.train_data, device='cuda', batch_size=2))
  gs = graphed.GraphedTrainStep(task, model, optimizer, reducer, opt_cfg, clip_norm=opt_cfg.gradient_clip_norm, eager_steps=1,
                                static_inputs=True)
  if eager:
    gs.eager_left = 1 << 62
  return gs, batch


def test_graphed_lamb_step_equals_the_eager_one():
  """Five steps through GraphedTrainStep (one eager, then the recorded graph replayed four times) against five eager
  steps of a twin: the same losses and parameters bit for bit -- nothing in FusedLamb.step waits for the device, and the
  learning rate and bias corrections of a replay come from device memory."""
  res = {}
  for eager in (True, False):
    gs, batch = _tiny_graphed(eager)
    losses = [float(gs(batch, step)['loss']) for step in range(1, 6)]
    assert (gs.graph is None) == eager and gs.optimizer.t == 5
    res[eager] = (losses, torch.cat([s['param'] for s in gs.optimizer.slabs]).clone(), torch.cat([s['m'] for s in gs.optimizer.slabs]).clone())
    gs.close()
  assert res[True][0] == res[False][0]
  assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
  assert len(set(res[False][0])) > 3 and all(np.isfinite(res[False][0]))


def test_trainer_loop_with_lamb_and_resume(tmp_path, monkeypatch):
  """`train.run_experiment` on the synthetic input with trainer.optimizer_config.optimizer_type=lamb: three steps, a
  finite loss, a FusedLamb behind it; a run resumed from its checkpoint continues bit for bit for one more step."""
  from tests._parity import tiny_experiment
  from mmt_amd import optimization, tasks, train
  monkeypatch.setenv('MMT_STEP_GRAPH', '0')
  made = []
  real = optimization.create_optimizer

  def spy(*a, **k):
    made.append(real(*a, **k))
    return made[-1]
  monkeypatch.setattr(optimization, 'create_optimizer', spy)

  def experiment(steps):
    exp = tiny_experiment(S=256, radius=32, n_global=8)
    exp.override({'task': {'train_data': {'global_batch_size': 4}, 'micro_batch_size': 4},
                  'runtime': {'mixed_precision_dtype': 'bfloat16'},
                  'trainer': {'train_steps': steps, 'checkpoint_interval': 3}})
    exp.override({'trainer.optimizer_config.optimizer_type': 'lamb'})
    return exp

  exp = experiment(3)
  model_a, logs_a = train.run_experiment(exp, 'train', str(tmp_path), log_every=1)
  assert len(made) == 1 and isinstance(made[0], optimization.FusedLamb) and made[0].t == 3
  assert len(logs_a) == 3 and all(np.isfinite(e['loss']) for e in logs_a) and len({e['loss'] for e in logs_a}) == 3
  # the uninterrupted continuation: a fourth step of the same objects, on the batch a restarted run draws first (the
  # synthetic input restarts with the process)
  opt_a, opt_cfg = made[0], exp.trainer.optimizer_config
  task = tasks.get_task(exp.task, compute_dtype=torch.bfloat16, num_replicas=1)
  batch = next(task.build_inputs(exp.task.train_data, device=torch.device('cuda', 0), rank=0))
  optimization.set_learning_rate(opt_a, optimization.learning_rate_at(opt_cfg, 3))
  out = task.train_step(batch, model_a, opt_a, reducer=opt_a.reducer, clip_norm=opt_cfg.gradient_clip_norm, step=4)
  model_c, logs_c = train.run_experiment(experiment(4), 'train', str(tmp_path), log_every=1)     # resumes from ckpt-3
  assert [e['step'] for e in logs_c] == [3] and logs_c[0]['loss'] == float(out[task.loss])
  assert len(made) == 2 and isinstance(made[1], optimization.FusedLamb) and made[1].t == 4
  for (n, p), q in zip(model_a.named_parameters(), model_c.parameters()):
    assert torch.equal(p, q), n
  for sa, sc in zip(opt_a.slabs, made[1].slabs):
    assert torch.equal(sa['m'], sc['m']) and torch.equal(sa['v'], sc['v'])
