"""Shared seeded inputs, dense side inputs, tolerances and numpy restatements of the parity tests (oracle vs HIP path).

Needs numpy, torch (dtypes and bf16 rounding only) and the oracle; everything that touches the device or `mmt_amd`
lives in tests/_parity.py."""
import numpy as np
import torch

from oracle import side_inputs as si

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ['f32', 'bf16']

# ---- the standing bars: defined here and nowhere else ----------------------------------------------------------------
# Output and lse, max abs error on O(1) values: fp32 1e-3 (north_star; observed ~1e-5); bf16 2e-2 against the oracle run
# on the bf16-rounded inputs (bf16 output rounding 2^-9 relative plus bf16 P in the PV product).
F32_TOL, BF16_TOL = 1e-3, 2e-2
# Gradients: fp32 2e-3 absolute (gradients are O(1..10); observed ~1e-5); bf16 3e-2 of max(1, max |want|) (bf16 outputs
# plus bf16 P / dS operands).
F32_GRAD_TOL, BF16_GRAD_TOL = 2e-3, 3e-2
# Two device calls that draw the same dropout mask ("structured equals dense"): error / max(1, max |reference|), for the
# output and every gradient.
F32_PAIR_TOL, BF16_PAIR_TOL = 2e-3, 3e-2
# Encoder and train step, fp32, dropout off (test_gpu_encoder.py): loss and outputs 1e-3 (north_star); parameter
# gradients 2e-3 of each tensor's max.
ENC_TOL, ENC_GRAD_TOL = 1e-3, 2e-3


def out_tol(dtype):
  return F32_TOL if dtype == torch.float32 else BF16_TOL


def grad_tol(dtype):
  return F32_GRAD_TOL if dtype == torch.float32 else BF16_GRAD_TOL


def pair_tol(dtype):
  return F32_PAIR_TOL if dtype == torch.float32 else BF16_PAIR_TOL


def grad_error(got, want, dtype):
  """The figure grad_tol bounds: max abs error, in bf16 divided by max(1, max |want|)."""
  err = np.abs(got - want).max()
  return err if dtype == torch.float32 else err / max(1.0, np.abs(want).max())


def attention_inputs(B, S, N, R, seed=0, D=64, scale_q=1.0):
  rng = np.random.default_rng(seed)
  q = (rng.standard_normal((B, S, N, D)) * scale_q).astype(np.float32)
  k = rng.standard_normal((B, S, N, D)).astype(np.float32)
  v = rng.standard_normal((B, S, N, D)).astype(np.float32)
  emb = (rng.standard_normal((R, N, D)) * 0.5).astype(np.float32) if R else None
  bias = (rng.standard_normal((R, N)) * 0.5).astype(np.float32) if R else None
  return q, k, v, emb, bias


def parity_inputs(B, S, N, R, dtype, seed, D=64, use_bias=True):
  """(q, k, v, emb, bias, dout) of a parity case: attention_inputs plus dout from its own stream, all rounded to bf16
  when that is the dtype under test (the oracle then sees what the device sees)."""
  q, k, v, emb, bias = attention_inputs(B, S, N, R, seed, D)
  dout = np.random.default_rng(seed + 100).standard_normal(q.shape).astype(np.float32)
  arrays = (q, k, v, emb, bias if use_bias else None, dout)
  if dtype == torch.bfloat16:
    arrays = tuple(None if x is None else bf16_round(x) for x in arrays)
  return arrays


def grid_mask(S, g, P, a):
  """grid(q,k) of include/mmt_attn.h as an [S,S] bool array: both in the image [g, g + P^2), at most `a` image rows
  and `a` columns apart (raster order, no wrap across rows)."""
  pos = np.arange(S)
  x = pos - g
  img = (x >= 0) & (x < P * P)
  row, col = np.where(img, x // P, 0), np.where(img, x % P, 0)
  return (a > 0) & img[:, None] & img[None, :] & (np.abs(row[:, None] - row[None, :]) <= a) & \
      (np.abs(col[:, None] - col[None, :]) <= a)


def image_origin_ids(S, m, P, r, g):
  """[S,S] ids of id_mode 3 from its definition (include/mmt_attn.h): the reference generator's image x image block
  placed at [g, g + P^2), text_part_id on image rows x other columns, image_part_id on other rows x image columns,
  the 1-D clipped id of k - q (on sequence positions) everywhere else."""
  I = P * P
  gen = si.MmtRelativePositionGenerator(P, r, m)
  block = gen.make_relative_att_ids(I, 1)[0]                     # [I,I]: the sequence is the image
  image_part = I + 8 + 2 * m + 1
  ids = si.RelativePositionGenerator1D(m).make_relative_att_ids(S, 1)[0].astype(np.int32).copy()
  img = np.zeros(S, bool)
  img[g:g + I] = True
  ids[img, :] = image_part + 1                                   # text_part_id
  ids[np.ix_(~img, img)] = image_part
  ids[np.ix_(img, img)] = block
  return ids


def relative_ids(S, id_mode, m, P=0, r=0, g=2):
  """[S,S] ids of a descriptor's id_mode: 1 and 2 the oracle's generators, 3 the 2-D ids with the image at g."""
  return image_origin_ids(S, m, P, r, g) if id_mode == 3 else si.relative_ids_from_desc(S, id_mode, m, P, r)


def dense_side_inputs(B, S, valid, radius, g0, ng, id_mode, m, P=0, r=0, gidx=None, a=0, g=2, example_ids=None):
  """Materialised [B,S,S] mask + ids for a pattern (what the reference would be fed).  The mask is the oracle's band /
  global mask (range [g0, g0 + ng) or the listed set `gidx`), segmented by `valid`; ORed with grid & segmented when the
  grid radius a > 0 (image at [g, g + P^2)); ANDed with the segmented mask of `example_ids` [B,S] for packed rows.
  `g` is also the image origin of id_mode 3."""
  valid = valid if valid is not None else [S] * B
  gm = grid_mask(S, g, P, a) if a else None
  masks = []
  for b, vl in enumerate(valid):
    mask = si.sparse_pattern_mask(S, vl, min(radius, S), g0, ng, gidx)
    if a:
      ex = np.arange(S) < vl
      mask = mask | (gm & (ex[:, None] == ex[None, :]))
    if example_ids is not None:
      mask = mask & si.make_segmented_att_mask(example_ids[b])
    masks.append(mask)
  ids = np.broadcast_to(relative_ids(S, id_mode, m, P, r, g), (B, S, S)).astype(np.int32).copy() if id_mode else None
  return np.stack(masks).astype(np.int32), ids


# ---- packed rows with per-example origin: a different definition, stated on its own ----------------------------------
def runs_of(row, S):
  """Run lengths of a row: its examples and, if they do not fill it, the padding tail."""
  row = [int(n) for n in row]
  return row + ([S - sum(row)] if sum(row) < S else [])


def single_example(L, radius, id_mode, m, P, r, grid, g0=0, ng=0, g=2):
  """([L,L] mask, [L,L] ids | None) of one example alone at the start of a row of its own length.  A run shorter than the
  image keeps the leading part of the ids of one long enough to hold it (its positions inside the image are image
  positions): the image is at [0, P^2) for id_mode 2 and at [g, g + P^2) for id_mode 3."""
  mask = si.sparse_pattern_mask(L, L, min(radius, L), g0, ng).astype(bool)
  if grid:
    mask = mask | grid_mask(L, grid[1], P, grid[0])
  ids = None
  if id_mode:
    Lp = max(L, {2: P * P, 3: g + P * P}.get(id_mode, L))
    ids = relative_ids(Lp, id_mode, m, P, r, g)[:L, :L]
  return mask.astype(np.int32), ids


def composed(lengths, S, radius, id_mode, m, P=0, r=0, grid=None, g0=0, ng=0, g=2):
  """Every run of a row (its examples and the padding tail) alone on the diagonal of [S,S]; all else masked."""
  B = len(lengths)
  mask = np.zeros((B, S, S), np.int32)
  rel = np.zeros((B, S, S), np.int32) if id_mode else None
  for b, row in enumerate(lengths):
    at = 0
    for L in runs_of(row, S):
      pm, pi = single_example(L, radius, id_mode, m, P, r, grid, g0, ng, g)
      mask[b, at:at + L, at:at + L] = pm
      if rel is not None:
        rel[b, at:at + L, at:at + L] = pi
      at += L
  return mask, rel


def bf16_round(x):
  return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


# ---- strided [B,S,N,D] views inside poisoned storages (the layouts include/mmt_attn.h promises to take) --------------
# One bit pattern serves inputs and outputs: a QUIET NaN (top mantissa bit set, so that it propagates through any
# arithmetic that reads it) whose low bits are recognisable, so that "untouched" is checked bit for bit through an
# integer view of the storage.
POISON_BITS = {'torch.bfloat16': 0x7FE5, 'torch.float32': 0x7FE5A5A5}
LAYOUTS = ('contiguous', 'head_major', 'time_major', 'qkv_slices', 'qkv_per_head', 'padded', 'gapped_batch')
BROADCAST_LAYOUTS = ('broadcast_heads', 'broadcast_batch')


def align_unit(dtype):
  """Elements in 16 bytes: the unit every stride must be a multiple of."""
  return 8 if dtype == torch.bfloat16 else 4


def layout_geometry(layout, shape, dtype, slot=1):
  """(strides of (b, s, n), offset, storage elements) of a named layout for a logical [B,S,N,D] array; `slot` picks
  the q / k / v place of the two fused layouts.  A tuple `(strides, offset, numel)` passes through (hand-made cases)."""
  if not isinstance(layout, str):
    strides, offset, numel = layout
    return tuple(int(s) for s in strides), int(offset), int(numel)
  B, S, N, D = shape
  a = align_unit(dtype)
  if layout == 'contiguous':
    return (S * N * D, N * D, D), 0, B * S * N * D
  if layout == 'head_major':                      # storage [B,N,S,D]
    return (N * S * D, D, S * D), 0, B * S * N * D
  if layout == 'time_major':                      # storage [S,B,N,D]
    return (N * D, B * N * D, D), 0, B * S * N * D
  if layout == 'qkv_slices':                      # storage [B,S,3,N,D]
    return (S * 3 * N * D, 3 * N * D, D), slot * N * D, B * S * 3 * N * D
  if layout == 'qkv_per_head':                    # storage [B,S,N,3,D]
    return (S * N * 3 * D, N * 3 * D, 3 * D), slot * D, B * S * N * 3 * D
  if layout == 'padded':                          # storage [B,S,N,D+a] sliced to D, base moved by a: rows 16-byte, not 128-byte aligned
    return (S * N * (D + a), N * (D + a), D + a), a, B * S * N * (D + a) + a
  if layout == 'gapped_batch':                    # poison between the examples
    gap = 41 * a
    return (S * N * D + gap, N * D, D), 0, B * (S * N * D + gap)
  if layout == 'broadcast_heads':                 # storage [B,S,1,D]
    return (S * D, D, 0), 0, B * S * D
  if layout == 'broadcast_batch':                 # storage [1,S,N,D]
    return (0, N * D, D), 0, S * N * D
  raise ValueError(f'unknown layout {layout!r}')


def _int_view(t):
  return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _poison_int(dtype):
  bits = POISON_BITS[str(dtype)]
  width = 16 if '16' in str(dtype) else 32
  return bits - (1 << width) if bits >= 1 << (width - 1) else bits


def strided_view(x, layout, poison=True, slot=1):
  """Places the logical [B,S,N,D] tensor `x` (bf16 or fp32, any device) into a larger flat storage and returns
  (view, storage): `view` has x's shape and values and the strides of `layout` (layout_geometry), every other element
  of `storage` holds POISON_BITS (zero with poison=False).  For the two broadcast layouts x must be constant along the
  broadcast axis (the view reads one copy)."""
  B, S, N, D = x.shape
  strides, offset, numel = layout_geometry(layout, x.shape, x.dtype, slot)
  storage = torch.empty(numel, dtype=x.dtype, device=x.device)
  _int_view(storage).fill_(_poison_int(x.dtype) if poison else 0)
  view = storage.as_strided((B, S, N, D), strides + (1,), offset)
  if strides[0] == 0:
    assert bool((_int_view(x.contiguous()) == _int_view(x[:1].expand_as(x).contiguous())).all()), 'x varies along the batch'
    view[:1].copy_(x[:1])
  elif strides[2] == 0:
    assert bool((_int_view(x.contiguous()) == _int_view(x[:, :, :1].expand_as(x).contiguous())).all()), 'x varies along the heads'
    view[:, :, :1].copy_(x[:, :, :1])
  else:
    view.copy_(x)
  return view, storage


def assert_gaps_untouched(storage, view, chunk=1 << 27):
  """Every element of `storage` outside `view` still holds POISON_BITS, bit for bit.  The view's own elements are set
  to the pattern for the duration of the check (and put back), so that the comparison is one pass over the storage in
  chunks, with no index tensor of the storage's size."""
  pat = _poison_int(storage.dtype)
  views = []
  for view in (view if isinstance(view, (list, tuple)) else [view]):      # several disjoint views of one storage
    if view.stride(0) == 0:                     # a broadcast view: one copy is stored
      view = view[:1]
    if view.stride(2) == 0:
      view = view[:, :, :1]
    views.append(view)
  keeps = [view.clone() for view in views]
  iv = _int_view(storage)
  try:
    for view in views:
      iv.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(pat)
    for lo in range(0, iv.numel(), chunk):
      part = iv[lo:lo + chunk]
      bad = part != pat
      if bool(bad.any()):
        at = lo + int(bad.nonzero()[0])
        raise AssertionError(f'storage element {at} outside the view was written: bits {int(iv[at]) & 0xFFFFFFFF:#x}')
  finally:
    for view, keep in zip(views, keeps):
      view.copy_(keep)


# ---- image front end: the float64 numpy yardstick (tests/test_image_frontend.py explains its standing) ---------------
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float64)
SOURCE_SIZES = [(1, 1), (5, 7), (37, 23), (64, 48)]          # + (image_size, image_size); see batch()
CONFIGS = [(32, 16), (24, 8), (20, 8)]                       # (image_size, patch_size); 20 / 8: remainder dropped, P = 2
EDGE_EPS = 1e-3                                              # ids: patches this close to a bin edge are left out
SEED = 20211


def _axis(n_in, n_out):
  src = (np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5
  fl = np.floor(src)
  return np.maximum(fl, 0).astype(np.int64), np.minimum(np.ceil(src), n_in - 1).astype(np.int64), src - fl


def resize_bilinear(x, size):
  """tf.image.resize(x, [size, size]) with TF2 defaults, float64: half-pixel centres, no antialiasing, 2x2 taps;
  horizontal lerp (top, bottom), then vertical."""
  y0, y1, ty = _axis(x.shape[0], size)
  x0, x1, tx = _axis(x.shape[1], size)
  tx, ty = tx[None, :, None], ty[:, None, None]
  top = x[y0][:, x0] + (x[y0][:, x1] - x[y0][:, x0]) * tx
  bot = x[y1][:, x0] + (x[y1][:, x1] - x[y1][:, x0]) * tx
  return top + (bot - top) * ty


def patches(im, patch_size):
  P = im.shape[0] // patch_size
  im = im[:P * patch_size, :P * patch_size]
  return im.reshape(P, patch_size, P, patch_size, 3).transpose(0, 2, 1, 3, 4).reshape(P * P, patch_size * patch_size * 3)


def restatement(images, image_size, patch_size, flip=None, bits=0):
  """The six steps for a list of uint8 [h, w, 3] arrays.  Returns normalised, unnormalised [B, P*P, E] float64, label
  ids [B, P*P] (or None) and, per patch, the distance of the closest channel mean (x255) to a bin edge."""
  norm, unnorm = [], []
  for b, u8 in enumerate(images):
    x = u8.astype(np.float64) / 255.0
    n = resize_bilinear((x - MEAN) / MEAN, image_size)       # the reference's order: normalise, then resize
    r = resize_bilinear(x, image_size)
    if flip is not None and flip[b]:
      n, r = n[:, ::-1], r[:, ::-1]
    norm.append(patches(n, patch_size)); unnorm.append(patches(r, patch_size))
  norm, unnorm = np.stack(norm), np.stack(unnorm)
  ids = dist = None
  if bits:
    bin_size = 256 // 2 ** bits
    avg = (unnorm * 255.0).reshape(*unnorm.shape[:2], patch_size * patch_size, 3).mean(-2)
    digit = np.minimum(np.floor(avg / bin_size), 2 ** bits - 1).astype(np.int64)
    ids = (digit * (2 ** bits) ** np.arange(3)).sum(-1).astype(np.int32)
    dist = np.abs(avg / bin_size - np.round(avg / bin_size)).max(-1) * bin_size
  return norm, unnorm, ids, dist


def batch(image_size, seed=SEED):
  rng = np.random.default_rng(seed)
  return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SOURCE_SIZES + [(image_size, image_size)]]


def check_outputs(out, images, image_size, patch_size, flip, bits, bf16=False):
  """The issue's bounds: fp32 |out - ref| <= 1e-5 (three lerps and a scale, each at most one ulp on values <= 1.5,
  amplified by 1 / 0.406: below 1e-6, ten times that allowed); bf16 |out - ref| <= 2^-8 |ref| + 1e-5; ids bit-equal
  away from bin edges, with at most 2 % of the patches left out."""
  norm, unnorm, ids, dist = restatement(images, image_size, patch_size, flip, bits)
  got = out['patch_embeddings'].double().cpu().numpy()
  assert got.shape == norm.shape
  err = np.abs(got - norm)
  print('normalised max err', err.max())
  assert (err <= (2.0 ** -8 * np.abs(norm) + 1e-5 if bf16 else 1e-5)).all(), err.max()
  if 'unnormalized_patch_embeddings' in out:
    err = np.abs(out['unnormalized_patch_embeddings'].double().cpu().numpy() - unnorm).max()
    print('unnormalised max err', err)
    assert err <= 1e-5, err
  if bits:
    keep = dist > EDGE_EPS
    print('patches left out', int((~keep).sum()), 'of', keep.size)
    assert (~keep).mean() <= 0.02
    assert np.array_equal(out['mpp_label_ids'].cpu().numpy()[keep], ids[keep])
  P = image_size // patch_size
  assert out['num_image_wordpieces'] == 2 + P * P
