"""mmt_image_patches on the GPU, through the ctypes boundary, against the float64 restatement of
tests/test_image_frontend.py (the reference's order: normalise, then resize).  Bounds as check_outputs there states
them: fp32 1e-5 absolute, bf16 2^-8 relative + 1e-5, label ids bit-equal away from bin edges; two calls are
bit-identical.  The 1x1 and 5x7 sources exercise every clamp (taps at the image border on both axes, h = w = 1); no case feeds out-of-range metadata."""
import numpy as np
import pytest
import torch

from tests._cases import CONFIGS, batch, check_outputs, restatement

pytestmark = pytest.mark.gpu

FLIPS = {'noflip': None, 'flip': [1, 0, 1, 0, 1]}
GUARD = 64            # sentinel elements behind every output: nothing may be written past the end


def run_kernel(images, image_size, patch_size, flip=None, dtype=torch.float32, want_unnorm=True, bits=3, want_ids=True):
  """One call of the C entry point on caller-owned buffers; returns the dict images_to_patch_features would."""
  from mmt_amd import _lib
  B, P, E = len(images), image_size // patch_size, patch_size * patch_size * 3
  pixels = torch.from_numpy(np.concatenate([x.reshape(-1) for x in images])).cuda()
  sizes = np.array([x.shape[:2] for x in images], dtype=np.int32)
  offsets = torch.from_numpy(np.cumsum([0] + [x.size for x in images[:-1]]).astype(np.int64)).cuda()
  heights, widths = torch.from_numpy(sizes[:, 0].copy()).cuda(), torch.from_numpy(sizes[:, 1].copy()).cuda()
  tflip = None if flip is None else torch.tensor(flip, dtype=torch.uint8).cuda()
  d = _lib.ImageDesc()
  d.B, d.image_size, d.patch_size, d.channel_bits = B, image_size, patch_size, bits
  d.out_dtype = _lib.MMT_F32 if dtype == torch.float32 else _lib.MMT_BF16
  d.mean[:] = [0.485, 0.456, 0.406]
  n = B * P * P
  norm = torch.full((n * E + GUARD,), -77.0, dtype=dtype, device='cuda')
  unnorm = torch.full((n * E + GUARD,), -77.0, device='cuda') if want_unnorm else None
  ids = torch.full((n + GUARD,), -77, dtype=torch.int32, device='cuda') if want_ids else None
  ptr = lambda t: None if t is None else t.data_ptr()
  _lib.check(_lib.lib().mmt_image_patches(d, pixels.data_ptr(), pixels.numel(), offsets.data_ptr(), heights.data_ptr(),
                                          widths.data_ptr(), ptr(tflip), norm.data_ptr(), ptr(unnorm), ptr(ids),
                                          torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()
  out = {'num_image_wordpieces': 2 + P * P, 'patch_embeddings': norm[:n * E].reshape(B, P * P, E)}
  assert (norm[n * E:] == -77.0).all()
  if want_unnorm:
    assert (unnorm[n * E:] == -77.0).all()
    out['unnormalized_patch_embeddings'] = unnorm[:n * E].reshape(B, P * P, E)
  if want_ids:
    assert (ids[n:] == -77).all()
    if bits:
      out['mpp_label_ids'] = ids[:n].reshape(B, P * P)
    else:
      assert (ids == -77).all()          # channel_bits = 0: no ids, the buffer is left alone
  return out


@pytest.mark.parametrize('flip', list(FLIPS), ids=list(FLIPS))
@pytest.mark.parametrize('image_size,patch_size', CONFIGS)
def test_mixed_sizes_fp32(image_size, patch_size, flip):
  """1x1, 5x7 (growing), 37x23 (one axis each way), 64x48 (shrinking) and image_size^2 in one batch; B * P * P is 20, 45
  (not a multiple of 4: the last workgroup is partial) and 20; flip vector with both values, and flip = NULL."""
  images = batch(image_size)
  out = run_kernel(images, image_size, patch_size, FLIPS[flip])
  check_outputs(out, images, image_size, patch_size, FLIPS[flip], 3)


@pytest.mark.parametrize('image_size,patch_size', CONFIGS)
def test_mixed_sizes_bf16(image_size, patch_size):
  images = batch(image_size)
  out = run_kernel(images, image_size, patch_size, FLIPS['flip'], dtype=torch.bfloat16)
  assert out['patch_embeddings'].dtype == torch.bfloat16
  check_outputs(out, images, image_size, patch_size, FLIPS['flip'], 3, bf16=True)      # unnormalised stays fp32: 1e-5


def test_other_channel_bits():
  """1 and 8 bits per channel.  With 8 bits every integer is a bin edge, which a constant patch (the 1x1 source) sits
  on exactly, so that source is left out of the 8-bit batch: the cap on excluded patches stays at 2 %."""
  images = batch(24)
  check_outputs(run_kernel(images, 24, 8, bits=1), images, 24, 8, None, 1)
  check_outputs(run_kernel(images[1:], 24, 8, bits=8), images[1:], 24, 8, None, 8)


def test_optional_outputs_and_determinism():
  """unnormalised NULL, ids NULL, both NULL, channel_bits 0 with an ids buffer: what is still written is bit-identical
  to the full call, and a second full call repeats the first bit for bit, ids included."""
  images = batch(24)
  full = run_kernel(images, 24, 8, FLIPS['flip'])
  again = run_kernel(images, 24, 8, FLIPS['flip'])
  for k in ('patch_embeddings', 'unnormalized_patch_embeddings', 'mpp_label_ids'):
    assert torch.equal(full[k], again[k]), k
  for kw in (dict(want_unnorm=False), dict(want_ids=False), dict(want_unnorm=False, want_ids=False), dict(bits=0)):
    part = run_kernel(images, 24, 8, FLIPS['flip'], **kw)
    assert ('mpp_label_ids' in part) == ('want_unnorm' in kw and len(kw) == 1), kw
    for k, v in part.items():
      if k != 'num_image_wordpieces':
        assert torch.equal(v, full[k]), (kw, k)


def test_python_entry_and_encoder_embed():
  """feature_pipeline.images_to_patch_features on device tensors (list and packed form) gives the kernel's outputs, and
  its patch_embeddings go through MmtEncoder.embed like those made from the restatement's resize: 1e-5 on the fp32
  embeddings, the bound of tests/test_gpu_embed.py."""
  from mmt_amd import MmtEncoder
  from mmt_amd import feature_pipeline as fp
  image_size, patch_size = 32, 16
  images = batch(image_size)
  flip = FLIPS['flip']
  dev = [torch.from_numpy(x).cuda() for x in images]
  out = fp.images_to_patch_features(dev, image_size, patch_size, flip=torch.tensor(flip, dtype=torch.bool).cuda(),
                                    keep_unnormalized=True, output_channel_bits=3)
  check_outputs(out, images, image_size, patch_size, flip, 3)
  direct = run_kernel(images, image_size, patch_size, flip)
  for k in ('patch_embeddings', 'unnormalized_patch_embeddings', 'mpp_label_ids'):
    assert torch.equal(out[k], direct[k]), k
  assert torch.equal(fp.make_mpp_label_ids(out['unnormalized_patch_embeddings'], patch_size), out['mpp_label_ids'])
  packed = (torch.cat([x.reshape(-1) for x in dev]), torch.tensor(np.cumsum([0] + [x.size for x in images[:-1]])).cuda(),
            torch.tensor([x.shape[0] for x in images], dtype=torch.int32).cuda(),
            torch.tensor([x.shape[1] for x in images], dtype=torch.int32).cuda())
  lean = fp.images_to_patch_features(packed, image_size, patch_size)
  assert set(lean) == {'patch_embeddings', 'num_image_wordpieces'}
  assert torch.equal(lean['patch_embeddings'], run_kernel(images, image_size, patch_size)['patch_embeddings'])

  torch.manual_seed(0)
  B, S = len(images), 12
  enc = MmtEncoder(vocab_size=50, hidden_size=64, num_hidden_layers=0, num_attention_heads=1, intermediate_size=64,
                   max_absolute_position_embeddings=16, patch_embedding_size=patch_size * patch_size * 3).cuda()
  word, seg = torch.randint(0, 50, (B, S)).cuda(), torch.randint(0, 3, (B, S)).cuda()
  want_pe = torch.from_numpy(restatement(images, image_size, patch_size, flip)[0]).float().cuda()
  with torch.no_grad():
    got = enc.embed(word, seg, out['patch_embeddings'])
    want = enc.embed(word, seg, want_pe)
    bare = enc.embed(word, seg, None)
  assert got.shape == (B, S, 64)
  err = float((got - want).abs().max())
  print('embed max err', err)
  assert err < 1e-5
  assert float((got - bare)[:, 2:2 + 4].abs().max()) > 1e-3          # the patches did arrive at [2, 2 + P*P)
