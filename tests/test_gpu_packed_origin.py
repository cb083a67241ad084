"""Packed multimodal examples (`example_starts=`, `MMT_FLAG_EXAMPLE_STARTS`) on the GPU: an example of a packed row sees
what it would see alone at the start of a row.

The oracle states that directly: for each run of equal ids of length L the single-example `sparse_pattern_mask(L, L, ..)`
(ORed with `grid_mask` where the pattern has a grid) and `relative_ids_from_desc(L, ..)` go on the diagonal of [S,S],
everything off the blocks is masked, and the result is fed to the dense fp64 oracle.  A padding tail is a run like any
other (tests/_cases.py `composed`).  Tolerances are the standing bars of tests/_cases.py.

Every 2-D case asserts on the CPU, before the GPU call, that the composed ids of every example after the first of a row
differ from the row-aligned ids on an allowed pair: the case cannot pass on row-aligned semantics."""
import pytest
import torch

from oracle import side_inputs as si
from tests._cases import DTYPES, ENC_GRAD_TOL, ENC_TOL, composed, parity_inputs, runs_of
from tests._parity import ACCUM_SEED, check_against, device_call, make_pattern, oracle_call, tiny_experiment

pytestmark = pytest.mark.gpu

DROP_SEED = 4321


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
  autograd, against the composed oracle.  Returns the device results."""
  ids, st = layout(lengths, S)
  if zero_starts:
    st = torch.zeros_like(st)
  if oracle:
    mask, rel = composed(lengths, S, radius, id_mode, m, P, r, grid, g0, ng)
    if id_mode == 2:
      assert_differs_from_row_aligned(lengths, S, mask, rel, id_mode, m, P, r)
  arrays = parity_inputs(ids.shape[0], S, N, R, dtype, seed, D)
  a, g = grid or (0, 2)
  kw = dict(pattern=make_pattern(radius=radius, g0=g0, ng=ng, id_mode=id_mode, m=m, P=P, r=r, a=a, g=g),
            example_ids=ids.cuda(), scale_before_add=scale_before_add)
  if starts:
    kw['example_starts'] = st.cuda()
  if dropout:
    kw.update(dropout_p=dropout, dropout_seed=DROP_SEED)
  got = device_call(arrays, dtype, accum=accum, **kw)
  if oracle:
    ref = oracle_call(arrays, mask, rel, scale_before_add=scale_before_add, dropout=(dropout, DROP_SEED) if dropout else None)
    check_against(got, ref, dtype, seed_grads=ACCUM_SEED if accum else None)
  return got


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
  a = run_origin(torch.float32, zero_starts=True, oracle=False, **cfg)
  b = run_origin(torch.float32, starts=False, oracle=False, **cfg)
  assert a.keys() == b.keys() and len(b) == 6
  for n in b:
    assert torch.equal(a[n], b[n]), n


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
    assert err < ENC_TOL, (e, err)


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
    assert err < ENC_TOL, (e, err)


def test_packed_embedding_gradients_fused_against_torch_branch():
  """The one-kernel assembly with `example_starts` / `patch_slots` (`mmt_embed_fwd_packed` / `mmt_embed_bwd_packed`)
  against the torch branch of `embed` on the same packed rows: output and the gradients of the word table, the position
  table (gathered by LOCAL position), the patch projection weight / bias (through the compact `dpatch` scatter) and the
  LayerNorm, at test_gpu_encoder.py's fp32 tolerances (ENC_TOL output, ENC_GRAD_TOL of max |grad|).  Row 0 holds an example without
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
  assert err < ENC_TOL
  for n in names:
    assert float(g_t[n].abs().max()) > 0, n
    e = float((g_f[n] - g_t[n]).abs().max()) / max(1e-3, float(g_t[n].abs().max()))
    print(f'{n}: {e:.3e}')
    assert e < ENC_GRAD_TOL, (n, e)
