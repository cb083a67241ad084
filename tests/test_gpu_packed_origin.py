"""Packed multimodal examples (`example_starts=`, `MMT_FLAG_EXAMPLE_STARTS`) on the GPU: an example of a packed row sees
what it would see alone at the start of a row.

The oracle states that directly: for each run of equal ids of length L the single-example `sparse_pattern_mask(L, L, ..)`
(ORed with `grid_mask` where the pattern has a grid) and `relative_ids_from_desc(L, ..)` go on the diagonal of [S,S],
everything off the blocks is masked, and the result is fed to the dense fp64 oracle.  A padding tail is a run like any
other.  Tolerances are the standing ones of test_gpu_packed.py (fp32 output 1e-3, bf16 output 2e-2, fp32 gradients 2e-3
absolute, bf16 gradients 3e-2 of max |grad|).

Every 2-D case asserts on the CPU, before the GPU call, that the composed ids of every example after the first of a row
differ from the row-aligned ids on an allowed pair: the case cannot pass on row-aligned semantics."""
import numpy as np
import pytest
import torch

from oracle import attention as oa
from oracle import side_inputs as si
from tests.test_gpu_packed import BF16_TOL, DTYPES, F32_TOL, _inputs, _pattern, check_against
from tests.test_image_grid_host import grid_mask

pytestmark = pytest.mark.gpu


def runs_of(row, S):
  """Run lengths of a row: its examples and, if they do not fill it, the padding tail."""
  row = [int(n) for n in row]
  return row + ([S - sum(row)] if sum(row) < S else [])


def single_example(L, radius, id_mode, m, P, r, grid, g0=0, ng=0):
  """([L,L] mask, [L,L] ids | None) of one example alone at the start of a row of its own length.  A run shorter than the
  image keeps the leading part of the ids of a P^2-long one (its positions below P^2 are image positions)."""
  mask = si.sparse_pattern_mask(L, L, min(radius, L), g0, ng).astype(bool)
  if grid:
    mask = mask | grid_mask(L, grid[1], P, grid[0])
  ids = None
  if id_mode:
    Lp = max(L, P * P) if id_mode == 2 else L
    ids = si.relative_ids_from_desc(Lp, id_mode, m, P, r)[:L, :L]
  return mask.astype(np.int32), ids


def composed(lengths, S, radius, id_mode, m, P=0, r=0, grid=None, g0=0, ng=0):
  B = len(lengths)
  mask = np.zeros((B, S, S), np.int32)
  rel = np.zeros((B, S, S), np.int32) if id_mode else None
  for b, row in enumerate(lengths):
    at = 0
    for L in runs_of(row, S):
      pm, pi = single_example(L, radius, id_mode, m, P, r, grid, g0, ng)
      mask[b, at:at + L, at:at + L] = pm
      if rel is not None:
        rel[b, at:at + L, at:at + L] = pi
      at += L
  return mask, rel


def assert_differs_from_row_aligned(lengths, S, mask, rel, id_mode, m, P, r):
  """Every example after the first of a row has an allowed pair whose composed id is not the row-aligned one."""
  aligned = si.relative_ids_from_desc(S, id_mode, m, P, r)
  for b, row in enumerate(lengths):
    at = 0
    for i, L in enumerate(runs_of(row, S)):
      sl = slice(at, at + L)
      if i > 0:
        assert ((rel[b, sl, sl] != aligned[sl, sl]) & (mask[b, sl, sl] != 0)).any(), (b, i)
      at += L


def layout(lengths, S):
  import mmt_amd
  ids, starts, _, _ = mmt_amd.packed_example_layout(lengths, [[True] * len(r) for r in lengths], S)
  return ids, starts


def run_origin(dtype, *, lengths, S, N=2, R, radius=1 << 30, id_mode=2, m, P=0, r=0, D=64, grid=None, g0=0, ng=0, seed=0,
               accum=False, scale_before_add=False, dropout=0.0, zero_starts=False, starts=True, oracle=True):
  """Structured (or, with global tokens, dense-route) call with example ids and starts, forward and backward through
  autograd, against the composed oracle.  Returns (out, grads) as torch tensors."""
  import mmt_amd
  from mmt_amd import step_scalars
  ids, st = layout(lengths, S)
  if zero_starts:
    st = torch.zeros_like(st)
  B = ids.shape[0]
  if oracle:
    mask, rel = composed(lengths, S, radius, id_mode, m, P, r, grid, g0, ng)
    if id_mode == 2:
      assert_differs_from_row_aligned(lengths, S, mask, rel, id_mode, m, P, r)
  q, k, v, emb, bias, dout = _inputs(B, S, N, R, dtype, seed, D)
  dev = lambda x, dt=dtype: torch.from_numpy(x).cuda().to(dt).contiguous()
  tq, tk, tv, te, tb = (dev(x).requires_grad_(True) for x in (q, k, v, emb, bias))
  gkw = dict(grid_radius=grid[0], grid_start=grid[1]) if grid else {}
  pat = _pattern(radius, g0, ng, id_mode, m, P, r, **gkw)
  kw = dict(pattern=pat, example_ids=ids.cuda(), scale_before_add=scale_before_add)
  if starts:
    kw['example_starts'] = st.cuda()
  if dropout:
    kw.update(dropout_p=dropout, dropout_seed=4321)
  out = mmt_amd.relative_attention(tq, tk, tv, te, tb, **kw)
  seed_grads = {}
  if accum:
    seed_grads = {'drel_emb': np.full(emb.shape, 0.25, np.float32), 'drel_bias': np.full(bias.shape, -0.5, np.float32)}
    demb, dbias = (torch.from_numpy(seed_grads[n]).cuda() for n in ('drel_emb', 'drel_bias'))
    det = [t.detach() for t in (tq, tk, tv, te, tb)]
    lse = mmt_amd.relative_attention_forward(*det, **kw)[1]
    mmt_amd.relative_attention_backward(dev(dout), *det, out.detach(), lse, rel_grads_accum=(demb, dbias), **kw)
  out.backward(dev(dout))
  torch.cuda.synchronize()
  t_out = out.detach().float()
  t_grads = {n: t.grad.float() for n, t in (('dq', tq), ('dk', tk), ('dv', tv), ('drel_emb', te), ('drel_bias', tb))}
  if accum:
    t_grads['drel_emb'], t_grads['drel_bias'] = demb, dbias
  if oracle:
    okw = dict(scale_after_add=not scale_before_add)
    if dropout:
      assert step_scalars.epoch_ptr(torch.device('cuda:0')) is None
      dseed = (4321 + step_scalars.host_epoch(torch.device('cuda:0'))) & ((1 << 64) - 1)
      keep, keep_prob = oa.dropout_keep_mask(B, N, S, dropout, dseed)
      okw.update(keep_mask=keep, keep_prob=keep_prob)
    ref, _ = oa.relative_attention_fwd(q, k, v, emb, bias, mask, rel, **okw)
    want = oa.relative_attention_bwd(dout, q, k, v, emb, bias, mask, rel, **okw)
    check_against(t_out.cpu().numpy(), {n: g.cpu().numpy() for n, g in t_grads.items()}, ref, want, dtype, seed_grads)
  return t_out, t_grads


FULL = dict(R=33, m=3, P=4, r=1, S=150, lengths=[[30, 45, 51, 24], [61, 18, 40, 31]])
BAND = dict(R=49, m=12, P=6, r=2, radius=8, S=200, lengths=[[90, 38, 72], [50, 150]])
CASES = {
    # starts off the tile boundaries, images straddling a 32-tile edge, several examples inside one 32-row block; part ids
    # 31 / 32 index real table rows
    '2d-full': FULL,
    # banded attention with per-example 2-D ids (part ids >= R contribute 0)
    '2d-band': BAND,
    # grid with 1-D ids: blocks inside one example (GridWalk around its image) and blocks that straddle examples
    'grid-1d': dict(R=32, id_mode=1, m=12, P=9, grid=(1, 2), radius=4, S=256, lengths=[[103, 128, 25], [90, 83, 83]]),
    # grid plus 2-D ids at head size 128
    'grid-2d-d128': dict(R=49, m=12, P=8, r=2, grid=(2, 2), radius=6, S=192, N=1, D=128, lengths=[[100, 92], [66, 126]]),
    '2d-dropout': dict(FULL, dropout=0.1),
    # grid at radius >= S: a block inside one example walks its example only (the id-range test cuts the row-wide band)
    'grid-full': dict(R=32, id_mode=1, m=12, P=5, grid=(1, 2), S=160, lengths=[[64, 64, 32], [100, 60]]),
}


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_origin_forward_and_backward_against_composed_oracle(name, dtype):
  run_origin(dtype, **CASES[name])


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_origin_backward_accumulates_table_gradients(dtype):
  run_origin(dtype, accum=True, **BAND)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_origin_scale_before_add(dtype):
  run_origin(dtype, scale_before_add=True, **BAND)


@pytest.mark.parametrize('id_mode', [1, 2], ids=['1d', '2d'])
def test_zero_starts_without_grid_equal_example_ids_alone_bitwise(id_mode):
  """Starts that are all zero make every local position the row position: the call computes, on kernels of the same
  code, what the call with `example_ids` alone computes -- fp32, bit for bit, forward and the five gradients."""
  cfg = dict(BAND, id_mode=id_mode, R=49 if id_mode == 2 else 32)
  a_out, a_grads = run_origin(torch.float32, zero_starts=True, oracle=False, **cfg)
  b_out, b_grads = run_origin(torch.float32, starts=False, oracle=False, **cfg)
  assert torch.equal(a_out, b_out)
  for n in b_grads:
    assert torch.equal(a_grads[n], b_grads[n]), n


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_starts_with_global_tokens_take_the_dense_route(dtype):
  """8 global tokens at local [20, 28) of every example: refused by the structured kernels, served by the dense operator
  on the composed mask and ids."""
  run_origin(dtype, g0=20, ng=8, **BAND)


# ---- encoder and heads: packed rows against every example alone ----------------------------------------------------
ENC_LENGTHS = [[256, 200], [210, 246]]       # S = 512; both rows end in a 56-position padding tail
ENC_S = 512


@pytest.fixture(scope='module')
def packed_model():
  """Tiny pretraining model (L = 2, H = 128, 2-D ids, P = 14) and one packed batch: four imaged examples in two rows."""
  import mmt_amd
  from tests.test_gpu_encoder import tiny_experiment
  exp = tiny_experiment(S=256, core=2, R=49)
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(0)
  model = task.build_model().cuda().eval()
  g = torch.Generator().manual_seed(1)
  word_ids = torch.randint(5, 2000, (2, ENC_S), generator=g, dtype=torch.int32)
  patches = torch.randn(4, 196, 768, generator=g)
  ids, starts, slots, first = mmt_amd.packed_example_layout(ENC_LENGTHS, [[True, True], [True, True]], ENC_S)
  pat = mmt_amd.input_utils.attention_pattern_from_config(exp.task.train_data)
  assert pat.id_mode == 2 and pat.n_global == 0 and pat.grid_radius == 0
  return dict(model=model, word_ids=word_ids, patches=patches, ids=ids, starts=starts, slots=slots, first=first, pat=pat)


def _examples(pm):
  e = 0
  for b, row in enumerate(ENC_LENGTHS):
    at = 0
    for L in row:
      yield e, b, at, L
      at += L
      e += 1


def test_packed_encoder_rows_match_each_example_alone(packed_model):
  """`MmtEncoder.forward` on packed rows: the rows of each example against `oracle.encoder.encoder_forward` on that
  example alone (full attention, its own 2-D ids, its own patches and positions); test_gpu_encoder.py's fp32 tolerance."""
  from oracle import encoder as oenc
  pm = packed_model
  model, pat = pm['model'], pm['pat']
  got = model.encoder(word_ids=pm['word_ids'].cuda(), patch_embeddings=pm['patches'].cuda(), attention_pattern=pat,
                      example_ids=pm['ids'].cuda(), example_starts=pm['starts'].cuda(), patch_slots=pm['slots'].cuda(),
                      training=False)['sequence_output'].float().cpu()
  sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
  for e, b, at, L in _examples(pm):
    rel = si.relative_ids_from_desc(L, 2, pat.max_dist, pat.patches_per_row, pat.core_layers)
    want = oenc.encoder_forward(sd, model.encoder.get_config(), pm['word_ids'][b:b + 1, at:at + L], None,
                                torch.ones(1, L, L, dtype=torch.int32), torch.from_numpy(rel)[None], pm['patches'][e:e + 1])
    err = float((got[b, at:at + L].double() - want[0]).abs().max())
    print(f'example {e}: max |packed - alone| = {err:.3e}')
    assert err < 1e-3, (e, err)


def test_packed_classification_logits_match_each_example_alone(packed_model):
  """Every head reads `first position + cls_token_idx` of every example: logits [E_all, 2] in (row, run) order, equal to
  the model's own run on each example alone within the encoder test's tolerance."""
  pm = packed_model
  model, pat = pm['model'], pm['pat']
  out = model(word_ids=pm['word_ids'].cuda(), patch_embeddings=pm['patches'].cuda(), attention_pattern=pat,
              example_ids=pm['ids'].cuda(), example_starts=pm['starts'].cuda(), patch_slots=pm['slots'].cuda(),
              first_positions=pm['first'].cuda(), training=False)
  logits = out['itm_logits'].float().cpu()
  assert tuple(logits.shape) == (4, 2)
  for e, b, at, L in _examples(pm):
    alone = model(word_ids=pm['word_ids'][b:b + 1, at:at + L].contiguous().cuda(), patch_embeddings=pm['patches'][e:e + 1].cuda(),
                  attention_pattern=pat, training=False)['itm_logits'].float().cpu()
    err = float((logits[e] - alone[0]).abs().max())
    print(f'example {e}: max |packed - alone| logits = {err:.3e}')
    assert err < 1e-3, (e, err)


def test_packed_embedding_gradients_fused_against_torch_branch():
  """The one-kernel assembly with `example_starts` / `patch_slots` (`mmt_embed_fwd_packed` / `mmt_embed_bwd_packed`)
  against the torch branch of `embed` on the same packed rows: output and the gradients of the word table, the position
  table (gathered by LOCAL position), the patch projection weight / bias (through the compact `dpatch` scatter) and the
  LayerNorm, at test_gpu_encoder.py's fp32 tolerances (1e-3 output, 2e-3 of max |grad|).  Row 0 holds an example without
  an image and an imaged one too short for its nine patches (the rest of its `dpatch` entry stays zero); both rows end
  in a padding tail."""
  import mmt_amd
  torch.manual_seed(0)
  enc = mmt_amd.MmtEncoder(vocab_size=200, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                           max_absolute_position_embeddings=40, relative_vocab_size=32, patch_embedding_size=24,
                           hidden_dropout_prob=0.1).cuda()
  S = 48
  lengths, has = [[20, 15, 9], [30, 12]], [[True, False, True], [True, True]]
  ids, starts, slots, _ = mmt_amd.packed_example_layout(lengths, has, S, device='cuda')
  g = torch.Generator().manual_seed(5)
  word_ids = torch.randint(0, 200, (2, S), generator=g, dtype=torch.int32).cuda()
  word_ids[0, 3] = word_ids[1, 7] = word_ids[0, 30]            # one id in several examples
  patches = torch.randn(4, 9, 24, generator=g).cuda()
  dout = torch.randn(2, S, 128, generator=g).cuda()
  names = ('_word_embedding_layer.embedding_table', '_position_embeddings', '_patch_projection_weight',
           '_patch_projection_bias', '_embedding_norm_layer.weight', '_embedding_norm_layer.bias',
           '_segment_embedding_layer.embedding_table')
  params = dict(enc.named_parameters())

  def run(fused_path):
    enc.use_fused_embedding = fused_path
    for p in params.values():
      p.grad = None
    out = enc.embed(word_ids, None, patches, False, example_starts=starts, patch_slots=slots)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach().float(), {n: params[n].grad.detach().float().clone() for n in names}

  assert enc._fused_embed_ok(word_ids)
  out_f, g_f = run(True)
  out_t, g_t = run(False)
  err = float((out_f - out_t).abs().max())
  print(f'max |fused - torch| = {err:.3e}')
  assert err < 1e-3
  for n in names:
    assert float(g_t[n].abs().max()) > 0, n
    e = float((g_f[n] - g_t[n]).abs().max()) / max(1e-3, float(g_t[n].abs().max()))
    print(f'{n}: {e:.3e}')
    assert e < 2e-3, (n, e)
