"""Per-example global tokens on packed multimodal rows (`example_starts=` with a global range, `MMT_FLAG_EXAMPLE_GLOBALS`)
on the structured kernels: every example of a packed row has its global tokens at [g0, g0 + ng) of its OWN positions.

The oracle is the one of test_gpu_packed_origin.py: `composed(.., g0, ng)` puts the single-example mask (band | global |
grid) and ids of every run on the diagonal of [S,S], fed to the dense fp64 oracle; the standing bars of tests/_cases.py.

Every case asserts on the CPU, before the device call, that the composed mask differs from the mask with ng = 0 on a pair
of every example long enough to hold a global token (the case cannot pass by ignoring the global term) and that the call
stays on the structured route.  `full-radius` is the one exception, by design: at radius >= S the global term adds no
pair, and the case asserts exactly that."""
import pytest
import torch

from oracle import side_inputs as si
from tests._cases import DTYPES, ENC_TOL, composed, parity_inputs, runs_of
from tests._parity import (ACCUM_SEED, GRAD_NAMES, assert_structured_equals_dense_under_dropout, check_against, device_call,
                           make_pattern, oracle_call, tiny_experiment, to_dev)

pytestmark = pytest.mark.gpu

DROP_SEED = 4321


def layout(lengths, S):
  import mmt_amd
  ids, starts, _, _ = mmt_amd.packed_example_layout(lengths, [[True] * len(r) for r in lengths], S)
  return ids, starts


def assert_global_term_matters(lengths, S, mask, plain, g0, adds_pairs=True):
  """`mask` against `plain` (the same case with ng = 0): every run longer than g0 differs on at least one pair -- or,
  with adds_pairs = False, the two are equal everywhere."""
  if not adds_pairs:
    assert (mask == plain).all()
    return
  n = 0
  for b, row in enumerate(lengths):
    at = 0
    for L in runs_of(row, S):
      sl = slice(at, at + L)
      if L > g0:
        assert (mask[b, sl, sl] != plain[b, sl, sl]).any(), (b, at, L)
        n += 1
      else:
        assert (mask[b, sl, sl] == plain[b, sl, sl]).all(), (b, at, L)
      at += L
  assert n > 0


def case(*, lengths, S, N=2, R, radius=1 << 30, id_mode=1, m=12, P=0, r=0, D=64, grid=None, g0, ng, adds_pairs=True):
  """CPU side of a case, computed once per case: layout, composed oracle inputs, the pattern; the two assertions."""
  from mmt_amd import ops
  ids, st = layout(lengths, S)
  mask, rel = composed(lengths, S, radius, id_mode, m, P, r, grid, g0, ng)
  plain, _ = composed(lengths, S, radius, id_mode, m, P, r, grid, 0, 0)
  assert_global_term_matters(lengths, S, mask, plain, g0, adds_pairs)
  a, g = grid or (0, 2)
  pattern = make_pattern(radius=radius, g0=g0, ng=ng, id_mode=id_mode, m=m, P=P, r=r, a=a, g=g)
  q = torch.zeros(len(lengths), S, N, D)
  assert ops._resolve_pattern(pattern, None, None, None, q, ids, st) == (pattern, None, None)     # the structured route
  return dict(ids=ids, st=st, mask=mask, rel=rel, pattern=pattern, shape=(len(lengths), S, N, R), D=D)


CASES = {
    # single-example blocks several tiles from their global tile, globals past band_hi, a 38-long run with no global
    # token, blocks that straddle examples
    'far-global': dict(S=200, lengths=[[90, 38, 72], [50, 150]], radius=8, g0=40, ng=8, id_mode=1, R=32, m=12),
    # three examples and their global rows in one 32-row block; no relative ids
    'many-in-block': dict(S=101, lengths=[[10, 12, 9, 70], [50, 51]], radius=4, g0=5, ng=3, id_mode=0, R=0),
    # the range crosses a tile edge in local and in row coordinates, more than 32 globals, one example ends inside the
    # range; 2-D ids: the GEN kernels
    'tile-edge': dict(S=192, lengths=[[100, 92], [66, 126]], radius=6, g0=30, ng=40, id_mode=2, R=49, m=12, P=5, r=2),
    # the grid-2d-d128 shape of test_gpu_packed_origin.py with the globals behind the image
    'grid-globals-d128': dict(S=192, lengths=[[100, 92], [66, 126]], radius=6, g0=2 + 8 * 8, ng=8, id_mode=2, R=49, m=12,
                              P=8, r=2, grid=(2, 2), N=1, D=128),
    # radius >= S: the global term adds no pair; the walk (whole examples either way) must not visit a tile twice
    'full-radius': dict(S=150, lengths=[[30, 45, 51, 24], [61, 18, 40, 31]], g0=20, ng=8, id_mode=1, R=32, m=12,
                        adds_pairs=False),
}
_BUILT = {}


def built(name):
  if name not in _BUILT:
    _BUILT[name] = case(**CASES[name])
  return _BUILT[name]


def call_kw(c, **extra):
  return dict(pattern=c['pattern'], example_ids=c['ids'].cuda(), example_starts=c['st'].cuda(), **extra)


def run(name, dtype, *, seed=0, accum=False, scale_before_add=False, dropout=0.0):
  c = built(name)
  arrays = parity_inputs(*c['shape'], dtype, seed, c['D'])
  kw = call_kw(c, scale_before_add=scale_before_add)
  if dropout:
    kw.update(dropout_p=dropout, dropout_seed=DROP_SEED)
  got = device_call(arrays, dtype, accum=accum, **kw)
  ref = oracle_call(arrays, c['mask'], c['rel'], scale_before_add=scale_before_add,
                    dropout=(dropout, DROP_SEED) if dropout else None)
  check_against(got, ref, dtype, label=name, seed_grads=ACCUM_SEED if accum else None)
  return got


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_globals_forward_and_backward_against_composed_oracle(name, dtype):
  run(name, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_globals_dropout_against_the_restated_keep_mask(dtype):
  run('far-global', dtype, dropout=0.1)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_globals_backward_accumulates_table_gradients(dtype):
  run('far-global', dtype, accum=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_globals_scale_before_add(dtype):
  run('far-global', dtype, scale_before_add=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_structured_equals_dense_operator_under_dropout(dtype):
  """The structured route and the dense operator on `composed`'s arrays draw the same keep mask and agree."""
  c = built('far-global')
  arrays = parity_inputs(*c['shape'], dtype, 7)
  assert_structured_equals_dense_under_dropout(
      arrays, dtype, call_kw(c),
      dict(att_mask=torch.from_numpy(c['mask']).cuda(), relative_att_ids=torch.from_numpy(c['rel']).cuda()))


def test_two_backward_calls_give_identical_bits():
  """fp32: the dK / dV / table-gradient sums keep one fixed order (a block with a global token walks its example's tiles
  ascending; no atomics across waves)."""
  c = built('far-global')
  arrays = parity_inputs(*c['shape'], torch.float32, 3)
  a, b = (device_call(arrays, torch.float32, **call_kw(c)) for _ in range(2))
  assert set(a) == set(b) == {'out', *GRAD_NAMES}
  for n in a:
    assert torch.equal(a[n], b[n]), n


def _raw_call(arrays, pattern, ids, st, extra_flags):
  """Forward and backward through the C ABI on a descriptor built by `ops._make_desc`, with `extra_flags` ORed in."""
  from mmt_amd import _lib, ops
  L = _lib.lib()
  q, k, v, emb, bias, dout = (to_dev(x, torch.float32) for x in arrays)
  B, S, N, D = q.shape
  R = emb.shape[0]
  out, lse = torch.empty_like(q), torch.empty((B, N, S), dtype=torch.float32, device='cuda')
  d = ops._make_desc(q, k, v, out, R, pattern, None, None, -10000.0, False, 0.0, 0, 0, ids, st)
  d.flags |= extra_flags
  ws = torch.empty((max(L.mmt_workspace_bytes(d), 16),), dtype=torch.uint8, device='cuda')
  stream = torch.cuda.current_stream().cuda_stream
  p = lambda t: t.data_ptr()
  _lib.check(L.mmt_attn_fwd(d, p(q), p(k), p(v), p(emb), p(bias), None, None, p(out), p(lse), p(ws), ws.numel(), stream))
  dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
  de, db = torch.empty((R, N, D), device='cuda'), torch.empty((R, N), device='cuda')
  _lib.check(L.mmt_attn_bwd(d, p(q), p(k), p(v), p(emb), p(bias), None, None, p(out), p(dout), p(lse), p(dq), p(dk), p(dv),
                            p(de), p(db), p(ws), ws.numel(), stream))
  torch.cuda.synchronize()
  return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, drel_emb=de, drel_bias=db)


def test_flag_without_global_tokens_is_the_origin_call_bitwise():
  """MMT_FLAG_EXAMPLE_GLOBALS with n_global = 0 takes the route and the kernels of the call without it."""
  from mmt_amd import _lib
  cfg = CASES['far-global']
  ids, st = layout(cfg['lengths'], cfg['S'])
  pattern = make_pattern(radius=cfg['radius'], id_mode=1, m=cfg['m'])
  arrays = parity_inputs(len(cfg['lengths']), cfg['S'], 2, cfg['R'], torch.float32, 5)
  a = _raw_call(arrays, pattern, ids.cuda(), st.cuda(), _lib.MMT_FLAG_EXAMPLE_GLOBALS)
  b = _raw_call(arrays, pattern, ids.cuda(), st.cuda(), 0)
  for n in b:
    assert torch.equal(a[n], b[n]), n


# ---- encoder: packed rows with per-example global tokens against every example alone ---------------------------------
ENC_LENGTHS = [[256, 200], [210, 246]]       # S = 512; both rows end in a 56-position padding tail (no global token there)
ENC_S = 512


def test_packed_encoder_with_global_tokens_matches_each_example_alone():
  """`MmtEncoder.forward` on packed rows under the config's own pattern (band 16 + 8 global tokens at 2 + 14^2 = 198 of
  every example; the 200-long example holds two of them): the rows of each example against
  `oracle.encoder.encoder_forward` on that example alone with its own sparse mask and 2-D ids."""
  import mmt_amd
  from mmt_amd import ops
  from oracle import encoder as oenc
  exp = tiny_experiment(S=256, core=2, R=49, radius=16, n_global=8)
  task = mmt_amd.tasks.get_task(exp.task)
  torch.manual_seed(0)
  model = task.build_model().cuda().eval()
  g = torch.Generator().manual_seed(1)
  word_ids = torch.randint(5, 2000, (2, ENC_S), generator=g, dtype=torch.int32)
  patches = torch.randn(4, 196, 768, generator=g)
  ids, starts, slots, _ = mmt_amd.packed_example_layout(ENC_LENGTHS, [[True, True], [True, True]], ENC_S)
  pat = mmt_amd.input_utils.attention_pattern_from_config(exp.task.train_data)
  assert (pat.id_mode, pat.local_radius, pat.global_start, pat.n_global) == (2, 16, 198, 8)
  assert ops._resolve_pattern(pat, None, None, None, torch.zeros(2, ENC_S, 2, 64), ids, starts) == (pat, None, None)
  with torch.no_grad():
    got = model.encoder(word_ids=word_ids.cuda(), patch_embeddings=patches.cuda(), attention_pattern=pat,
                        example_ids=ids.cuda(), example_starts=starts.cuda(), patch_slots=slots.cuda(),
                        training=False)['sequence_output'].float().cpu()
  sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
  e = 0
  for b, row in enumerate(ENC_LENGTHS):
    at = 0
    for L in row:
      rel = si.relative_ids_from_desc(L, 2, pat.max_dist, pat.patches_per_row, pat.core_layers)
      mask = si.sparse_pattern_mask(L, L, 16, pat.global_start, pat.n_global)
      assert (mask != si.sparse_pattern_mask(L, L, 16)).any()
      want = oenc.encoder_forward(sd, model.encoder.get_config(), word_ids[b:b + 1, at:at + L], None,
                                  torch.from_numpy(mask)[None], torch.from_numpy(rel)[None], patches[e:e + 1])
      err = float((got[b, at:at + L].double() - want[0]).abs().max())
      print(f'example {e}: max |packed - alone| = {err:.3e}')
      assert err < ENC_TOL, (e, err)
      at += L
      e += 1
