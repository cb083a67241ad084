"""Device-side feature pipeline of the data layer's contract: the per-example
tensor transforms the reference runs inside tf.data on the host, as batched torch ops on the GPU
(integer / byte work: gathers, reshapes, bucketize -- nothing here is a GEMM).

  decode_jpeg_images         src/data/data_utils.py:195      (`tf.io.decode_image(example['image_data'])` for JPEG bytes: markers on
                                                              the host, Huffman decoding on the host or, with entropy='device', in
                                                              HIP; IDCT, upsampling and colour in HIP)
  decode_png_images          src/data/data_utils.py:195      (the same call for PNG bytes: chunk walk and the library's own inflate on
                                                              the host, or with inflate='device' the inflate in HIP too;
                                                              unfiltering, de-interlacing, expansion and palette in HIP)
  decode_images              src/data/data_utils.py:195      (a batch of JPEG and PNG files, each to its decoder by its signature)
  decode_image_features      src/data/data_utils.py:195-222  (`decode_fn` from the encoded bytes or the decoded pixels on, driven by the
                                                              data config: RandAugment and the flip coin when training, then the line below)
  rand_augment(_plan)        src/data/data_utils.py:125-145, 199-202  (`RandAugment(num_layers=1)`, the reference's 14 operations,
                                                              on the decoded uint8 images -- HIP)
  images_to_patch_features   src/data/data_utils.py:195-222  (decoded uint8 images of mixed sizes: /255, bilinear resize,
                                                              (im - MEAN) / MEAN, flip, patches, MPP colour ids -- one HIP kernel)
  convert_image_to_patches   src/data/data_utils.py:147-180  (tf.image.extract_patches 16x16 VALID + raster order)
  make_mpp_label_ids         src/data/data_utils.py:448-481  (mean colour per channel -> 2^bits bins -> base-2^bits id)
  make_matching_features     src/data/data_utils.py:642-712  (in-batch negatives for ITM: tile images, roll texts)

The text half of `decode_fn` (:241-278: WordPiece tokenisation, trim, field tokens, [SEP], padding, word starts) is
mmt_amd/text_frontend.py (`decode_text_features`, HIP: csrc/text_tokens.hip); its outputs are the text_token_ids,
num_text_wordpieces and text_word_start that `make_mlm_and_mpp_features` below takes.
JPEG decode (baseline and extended sequential files; DESIGN.md section 4 lists what is accepted) is `decode_jpeg_images`,
PNG decode (RGB at depth 8, grey and palette at depths 1 to 8; the Fashion-Gen shards) is `decode_png_images`, and
`decode_images` sends each file of a batch to its decoder by its signature; GIF and BMP stay out of scope.  The TFRecord container in front of all of this, and
the loader that strings these stages together, are mmt_amd/records.py and mmt_amd/pretrain_dataloader.py."""
from __future__ import annotations

import ctypes
import math
from concurrent.futures import ThreadPoolExecutor
from typing import Dict

import numpy as np

import torch

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)    # src/data/data_utils.py: the reference's normalisation constant


def convert_image_to_patches(images: torch.Tensor, patch_size: int) -> torch.Tensor:
  """[B, H, W, C] -> [B, P*P, patch_size*patch_size*C], P = H // patch_size, raster scan; inside a
  patch the order is (row, column, channel), as tf.image.extract_patches flattens it."""
  if images.dim() != 4:
    raise ValueError('images must be [batch, height, width, channels]')
  B, H, W, C = images.shape
  if H != W:
    raise ValueError('square images expected (image_size x image_size)')
  P = H // patch_size
  x = images[:, :P * patch_size, :P * patch_size]           # VALID padding: the remainder is dropped
  x = x.reshape(B, P, patch_size, P, patch_size, C).permute(0, 1, 3, 2, 4, 5)
  return x.reshape(B, P * P, patch_size * patch_size * C)


def make_mpp_label_ids(mpp_embeddings: torch.Tensor, patch_size: int, channels: int = 3,
                       output_channel_bits: int = 3, max_pixel_val: int = 256) -> torch.Tensor:
  """[..., patch_size^2 * channels] pixel values in [0, 1] -> int32 class ids in [0, 2^(bits*channels)):
  the mean of each channel, scaled to 0..255, is bucketized into 2^bits equal bins and the per-channel
  bins are combined as digits of base 2^bits (channel 0 least significant)."""
  lead = mpp_embeddings.shape[:-1]
  bin_size = max_pixel_val // (2 ** output_channel_bits)
  x = mpp_embeddings.to(torch.float32) * (max_pixel_val - 1)
  avg = x.reshape(*lead, patch_size * patch_size, channels).mean(dim=-2)
  bins = torch.arange(bin_size, max_pixel_val, bin_size, device=avg.device, dtype=torch.float32)
  digit = torch.bucketize(avg, bins, right=True)             # boundaries[i-1] <= x < boundaries[i]
  weight = (2 ** output_channel_bits) ** torch.arange(channels, device=avg.device)
  return (digit * weight).sum(-1).to(torch.int32)


# ---------------------------------------------------------------------------------------------------
# Image front end (`decode_fn`, src/data/data_utils.py:195-222): decoded uint8 images -> patch features.
# ---------------------------------------------------------------------------------------------------
def _resize_axis(n_in: int, n_out: int, device):
  """Taps of tf.image.resize (TF2 defaults: half-pixel centres, no antialiasing) on one axis:
  src = (dst + 0.5) * in / out - 0.5, lo = max(floor(src), 0), hi = min(ceil(src), in - 1), t = src - floor(src).
  The coordinate is formed in float64, as the kernel does, so that t carries one float32 rounding only."""
  src = (torch.arange(n_out, dtype=torch.float64, device=device) + 0.5) * (float(n_in) / float(n_out)) - 0.5
  fl = torch.floor(src)
  lo = fl.clamp(min=0).to(torch.int64)
  hi = torch.ceil(src).clamp(max=n_in - 1).to(torch.int64)
  return lo, hi, (src - fl).to(torch.float32)


def _resize_bilinear_u8(image: torch.Tensor, size: int) -> torch.Tensor:
  """uint8 [h, w, 3] -> float32 [size, size, 3] in [0, 1]: /255 (tf.io.decode_image(dtype=float32)), then the 2x2-tap
  bilinear resize, horizontal lerp first."""
  x = image.to(torch.float32) / 255.0
  y0, y1, ty = _resize_axis(image.shape[0], size, image.device)
  x0, x1, tx = _resize_axis(image.shape[1], size, image.device)
  tx, ty = tx[None, :, None], ty[:, None, None]
  top_rows, bot_rows = x[y0], x[y1]
  top = top_rows[:, x0] + (top_rows[:, x1] - top_rows[:, x0]) * tx
  bot = bot_rows[:, x0] + (bot_rows[:, x1] - bot_rows[:, x0]) * tx
  return top + (bot - top) * ty


def _pack_images(images):
  """list of uint8 [h, w, 3] tensors -> (pixels [sum h*w*3] uint8, offsets int64 [B], heights, widths int32 [B])."""
  if len(images) == 0:
    raise ValueError('images is empty')
  dev = images[0].device
  hs, ws, offs, n = [], [], [], 0
  for i, im in enumerate(images):
    if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8:
      raise ValueError(f'images[{i}] must be a uint8 tensor (decoded pixels)')
    if im.dim() != 3 or im.shape[2] != 3:
      raise ValueError(f'images[{i}] must be [height, width, 3], got {tuple(im.shape)}')
    if im.shape[0] < 1 or im.shape[1] < 1:
      raise ValueError(f'images[{i}] is empty: {tuple(im.shape)}')
    if im.device != dev:
      raise ValueError('all images must live on one device')
    hs.append(im.shape[0]); ws.append(im.shape[1]); offs.append(n)
    n += im.numel()
  pixels = torch.cat([im.reshape(-1) for im in images])
  meta = lambda v, dt: torch.tensor(v, dtype=dt).to(dev)
  return pixels, meta(offs, torch.int64), meta(hs, torch.int32), meta(ws, torch.int32)


def _check_packed(packed):
  if len(packed) != 4:
    raise ValueError('packed images are a (pixels, offsets, heights, widths) tuple')
  pixels, offsets, heights, widths = packed
  if pixels.dtype != torch.uint8 or pixels.dim() != 1 or pixels.numel() < 1:
    raise ValueError('pixels must be a non-empty 1-D uint8 tensor')
  B = offsets.shape[0] if offsets.dim() == 1 else -1
  if B < 1 or offsets.dtype != torch.int64:
    raise ValueError('offsets must be int64 [B], B >= 1')
  for name, t in (('heights', heights), ('widths', widths)):
    if t.dtype != torch.int32 or t.shape != (B,):
      raise ValueError(f'{name} must be int32 [B]')
  if any(t.device != pixels.device for t in (offsets, heights, widths)):
    raise ValueError('pixels, offsets, heights and widths must live on one device')
  if not pixels.is_cuda:         # on the device the values are not read back: the kernel clamps them (include/mmt_layer.h)
    if int(heights.min()) < 1 or int(widths.min()) < 1:
      raise ValueError('heights and widths must be positive')
    end = offsets + heights.to(torch.int64) * widths.to(torch.int64) * 3
    if int(offsets.min()) < 0 or int(end.max()) > pixels.numel():
      raise ValueError('an image leaves the pixel buffer')
  return pixels.contiguous(), offsets.contiguous(), heights.contiguous(), widths.contiguous()


# ---------------------------------------------------------------------------------------------------
# JPEG decode (`tf.io.decode_image`, src/data/data_utils.py:195): encoded bytes -> the packed layout.  The host parses
# and Huffman-decodes (csrc/jpeg_decode.hip, plain C++; ctypes releases the GIL, so a thread pool spreads the files),
# the device dequantises, transforms, upsamples and converts.  DESIGN.md section 4 "JPEG decode" has the rules.
# ---------------------------------------------------------------------------------------------------
def _default_device(device):
  return torch.device(device) if device is not None else torch.device('cuda' if torch.cuda.is_available() else 'cpu')


def _is_encoded(item) -> bool:
  return isinstance(item, (bytes, bytearray, memoryview, np.ndarray))


def _maybe_decode(images, device, entropy='host', uploaded=None, png_inflate='host'):
  """A list whose items are encoded bytes (JPEG or PNG files, `decode_images`) is decoded first; a list of tensors or a
  packed tuple passes unchanged."""
  if isinstance(images, tuple):
    return images
  images = list(images)
  if images and all(_is_encoded(im) for im in images):
    return decode_images(images, device, entropy=entropy, uploaded=uploaded, png_inflate=png_inflate)
  return images


# Defaults of the device entropy decode, from profiles/jpeg_decode_timing.json ("JPEG entropy decode
# on the device"): the fastest of 64 / 128 / 256 / 512 bytes, and the most rounds a file of the set needed (2) plus two.
JPEG_ENTROPY_SUBSEQ_BYTES = 128
JPEG_ENTROPY_MAX_ROUNDS = 4


def _up16(n: int) -> int:
  return (n + 15) & ~15


def _jpeg_entropy_stage(L, _lib, bufs, images, n_coef, device, workers, subseq_bytes, max_rounds, uploaded=None):
  """The `entropy='device'` stage of decode_jpeg_images: (coef int16 [n_coef], qtab int16 [B * 192]) on `device`.
  mmt_jpeg_scan_plan per file over the thread pool; file bytes and plans in one buffer (pinned for a GPU) and one upload;
  mmt_jpeg_entropy (mmt_jpeg_entropy_host for 'cpu'); one read-back of the status words.  A file whose plan was refused
  or whose status is not 0 goes through mmt_jpeg_coefficients and its planes are copied into the same coef buffer, so the
  result does not depend on the path a file took; what the host decode refuses raises ValueError as the host path does.
  uploaded: (bytes uint8 tensor on `device`, offsets): file i already lives at bytes[offsets[i]:] there (the record
  loader's blob), so the kernels read it in place and only the plans are uploaded."""
  B = len(bufs)
  on_gpu = device.type == 'cuda'
  sb, rounds = int(subseq_bytes), int(max_rounds)

  def plan(i):
    scan = _lib.JpegScan()
    a = bufs[i]
    rc = L.mmt_jpeg_scan_plan(a.ctypes.data, a.size, ctypes.byref(images[i]), sb, ctypes.byref(scan), None, None, None, 0, None, 0)
    if rc != 0:
      return None
    huff = np.empty(6 * _lib.MMT_JPEG_HUFF_WORDS, dtype=np.uint32)
    qt = np.empty(192, dtype=np.uint16)
    seg = np.empty(scan.n_segments * 4, dtype=np.int32)
    sub = np.empty(scan.n_subseq, dtype=np.int32)
    rc = L.mmt_jpeg_scan_plan(a.ctypes.data, a.size, ctypes.byref(images[i]), sb, ctypes.byref(scan), huff.ctypes.data, qt.ctypes.data,
                              seg.ctypes.data, scan.n_segments, sub.ctypes.data, scan.n_subseq)
    return None if rc != 0 else (scan, huff, qt, seg, sub)

  if workers == 1 or B == 1:
    plans = [plan(i) for i in range(B)]
  else:
    with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
      plans = list(pool.map(plan, range(B)))

  # one buffer: bytes of the planned files | huff | segments | subseqs | scans | images | qtables | (status, device side)
  scans = (_lib.JpegScan * B)()
  at_bytes, at_seg, at_sub = 0, 0, 0
  for i, pl in enumerate(plans):
    if pl is None:
      continue                                                  # a zeroed scan: no subsequence, the status word says so
    scan = pl[0]
    scan.byte_offset += at_bytes if uploaded is None else int(uploaded[1][i])
    scan.segment_offset, scan.subseq_offset = at_seg, at_sub
    scans[i] = scan
    if uploaded is None:
      at_bytes += bufs[i].size
    at_seg += scan.n_segments
    at_sub += scan.n_subseq
  planned = [i for i, pl in enumerate(plans) if pl is not None]
  max_sub = max([plans[i][0].n_subseq for i in planned], default=0)
  o_huff = _up16(max(at_bytes, 1))
  o_seg = o_huff + B * 6 * _lib.MMT_JPEG_HUFF_WORDS * 4
  o_sub = _up16(o_seg + max(at_seg, 1) * 16)
  o_scan = _up16(o_sub + max(at_sub, 1) * 4)
  o_img = _up16(o_scan + ctypes.sizeof(scans))
  o_qt = _up16(o_img + ctypes.sizeof(images))
  total = _up16(o_qt + B * 384)
  stage = torch.zeros(total, dtype=torch.uint8, pin_memory=on_gpu)
  view = stage.numpy()
  at = 0
  for i in planned:
    _, huff, qt, seg, sub = plans[i]
    if uploaded is None:
      view[at:at + bufs[i].size] = bufs[i]
      at += bufs[i].size
    view[o_huff + i * huff.nbytes:o_huff + (i + 1) * huff.nbytes] = huff.view(np.uint8)
    view[o_seg + scans[i].segment_offset * 16:o_seg + scans[i].segment_offset * 16 + seg.nbytes] = seg.view(np.uint8)
    view[o_sub + scans[i].subseq_offset * 4:o_sub + scans[i].subseq_offset * 4 + sub.nbytes] = sub.view(np.uint8)
    view[o_qt + i * 384:o_qt + (i + 1) * 384] = qt.view(np.uint8)
  view[o_scan:o_scan + ctypes.sizeof(scans)] = np.frombuffer(bytes(scans), dtype=np.uint8)
  view[o_img:o_img + ctypes.sizeof(images)] = np.frombuffer(bytes(images), dtype=np.uint8)

  def host_decode(i):                                           # the host path for one file, into buffers of its own
    im = _lib.JpegImage.from_buffer_copy(images[i])
    base = im.coef_offset[0]
    for c in range(3):
      im.coef_offset[c] -= base
    coef = torch.empty(im.coef_elems, dtype=torch.int16, pin_memory=on_gpu)
    qt = torch.empty(192, dtype=torch.int16, pin_memory=on_gpu)
    rc = L.mmt_jpeg_coefficients(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(im), coef.data_ptr(), im.coef_elems, qt.data_ptr())
    if rc != 0:
      raise ValueError(f'data[{i}] cannot be decoded: {L.mmt_last_error().decode()}')
    return base, coef, qt

  def run(stage_d, stream):
    coef_d = torch.empty(n_coef, dtype=torch.int16, device=device)
    status_d = torch.zeros(B, dtype=torch.int32, device=device)
    base = stage_d.data_ptr()
    if planned:
      need = L.mmt_jpeg_entropy_workspace_bytes(B, at_sub, max_sub, sb, rounds)
      work = torch.empty(need, dtype=torch.uint8, device=device)
      src, src_len = (base, max(at_bytes, 1)) if uploaded is None else (uploaded[0].data_ptr(), uploaded[0].numel())
      args = (B, src, src_len, base + o_img, base + o_scan, base + o_huff, base + o_seg, max(at_seg, 1), base + o_sub, at_sub,
              max_sub, sb, rounds, coef_d.data_ptr(), n_coef, status_d.data_ptr(), work.data_ptr(), need)
      _lib.check(L.mmt_jpeg_entropy(*args, stream) if on_gpu else L.mmt_jpeg_entropy_host(*args))
      status = status_d.cpu().tolist()                          # the one read-back; waits for the kernels
    else:
      status = [0] * B
    qtab_d = stage_d[o_qt:o_qt + B * 384].view(torch.int16)
    for i in range(B):
      if plans[i] is None or status[i] != 0:
        off, coef, qt = host_decode(i)
        coef_d[off:off + coef.numel()].copy_(coef, non_blocking=True)
        qtab_d[i * 192:(i + 1) * 192].copy_(qt, non_blocking=True)
    return coef_d, qtab_d

  if on_gpu:
    with torch.cuda.device(device):
      return run(stage.to(device, non_blocking=True), torch.cuda.current_stream(device).cuda_stream)
  return run(stage, None)


def decode_jpeg_images(data, device, *, workers: int = 8, out: torch.Tensor = None, entropy: str = 'host',
                       subseq_bytes: int = None, max_rounds: int = None, uploaded=None):
  """JPEG files -> the packed (pixels uint8 [n], offsets int64 [B], heights int32 [B], widths int32 [B]) tuple on
  `device` that `rand_augment` and `images_to_patch_features` take; image b is RGB, row-major, back to back.

  data: a list of bytes, bytearray, memoryview or uint8 numpy arrays, one file each.  libjpeg's default decode
  (JDCT_ISLOW, fancy upsampling), bit for bit; a greyscale file gives R = G = B.  Per item mmt_jpeg_info; one
  coefficient buffer for the batch (pinned when the device is a GPU); mmt_jpeg_coefficients spread over `workers` threads
  (clamped to 1..16); one asynchronous upload; one mmt_jpeg_pixels.  With device 'cpu' the same buffers go through
  mmt_jpeg_pixels_host.  out: a contiguous uint8 tensor on `device` of at least the needed size (allocated when None;
  bytes behind the last image are not written).  A file the library refuses raises ValueError naming the example.

  entropy: 'host' (the default) is the path above.  'device' uploads the encoded bytes instead of the coefficients and
  runs the Huffman decode as kernels (mmt_jpeg_scan_plan per file on the thread pool, then mmt_jpeg_entropy in front of
  mmt_jpeg_pixels on the same stream; with device 'cpu' mmt_jpeg_entropy_host); files it does not serve (more than one
  scan), files that need more than max_rounds rounds and corrupt files go through the host decode, so pixels and errors
  are those of 'host'.  'auto' is 'device' on a GPU and 'host' otherwise.  subseq_bytes (a power of two in [8, 1024]) and
  max_rounds (>= 1) default to JPEG_ENTROPY_SUBSEQ_BYTES and JPEG_ENTROPY_MAX_ROUNDS.

  uploaded: None, or (bytes, offsets) -- a 1-D uint8 tensor on `device` (16-byte aligned) that already holds the files,
  file i at bytes[offsets[i] : offsets[i] + len(data[i])] -- which the device entropy decode then reads in place instead
  of uploading the files again (the record loader's blob).  `data` still names the host copies: the markers are parsed
  there.  The host path ignores it."""
  from . import _lib
  L = _lib.lib()
  device = torch.device(device)
  if entropy not in ('host', 'device', 'auto'):
    raise ValueError(f"entropy must be 'host', 'device' or 'auto', got {entropy!r}")
  if entropy == 'auto':
    entropy = 'device' if device.type == 'cuda' else 'host'
  subseq_bytes = JPEG_ENTROPY_SUBSEQ_BYTES if subseq_bytes is None else int(subseq_bytes)
  max_rounds = JPEG_ENTROPY_MAX_ROUNDS if max_rounds is None else int(max_rounds)
  if subseq_bytes < 8 or subseq_bytes > 1024 or subseq_bytes & (subseq_bytes - 1):
    raise ValueError(f'subseq_bytes must be a power of two in [8, 1024], got {subseq_bytes}')
  if max_rounds < 1:
    raise ValueError(f'max_rounds must be at least 1, got {max_rounds}')
  items = list(data)
  B = len(items)
  if B == 0:
    raise ValueError('data is empty')
  bufs = []
  for i, item in enumerate(items):
    if not _is_encoded(item):
      raise ValueError(f'data[{i}] must be bytes, bytearray, memoryview or a uint8 numpy array, got {type(item).__name__}')
    arr = np.ascontiguousarray(item) if isinstance(item, np.ndarray) else np.frombuffer(item, dtype=np.uint8)
    if arr.dtype != np.uint8 or arr.ndim != 1:
      raise ValueError(f'data[{i}] must be a 1-D uint8 array of encoded bytes')
    bufs.append(arr)
  workers = min(max(int(workers), 1), 16)
  images = (_lib.JpegImage * B)()
  n_coef, n_pix = 0, 0
  hs, ws, offs = [], [], []
  for i, arr in enumerate(bufs):
    rc = L.mmt_jpeg_info(arr.ctypes.data, arr.size, ctypes.byref(images[i]))
    if rc != 0:
      raise ValueError(f'data[{i}] cannot be decoded: {L.mmt_last_error().decode()}')
    im = images[i]
    for c in range(3):
      im.coef_offset[c] += n_coef
    im.pixel_offset = n_pix
    n_coef += im.coef_elems
    hs.append(im.height); ws.append(im.width); offs.append(n_pix)
    n_pix += im.height * im.width * 3
  on_gpu = device.type == 'cuda'
  if entropy == 'device':
    if uploaded is not None:
      blob, at = uploaded
      same = isinstance(blob, torch.Tensor) and blob.device.type == device.type and device.index in (None, blob.device.index)
      if not same or blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous() or blob.data_ptr() & 15 or len(at) != B:
        raise ValueError(f'uploaded must be (a contiguous 16-byte aligned 1-D uint8 tensor on {device}, {B} offsets)')
      if any(int(o) < 0 or int(o) + a.size > blob.numel() for o, a in zip(at, bufs)):
        raise ValueError('an uploaded file leaves the uploaded bytes')
    coef_t, qtab_t = _jpeg_entropy_stage(L, _lib, bufs, images, n_coef, device, workers, subseq_bytes, max_rounds, uploaded)
    if out is None:
      out = torch.zeros(n_pix, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < n_pix or out.device != device or not out.is_contiguous():
      raise ValueError(f'out must be a contiguous 1-D uint8 tensor of at least {n_pix} bytes on {device}')
    need = L.mmt_jpeg_workspace_bytes(n_coef)
    work = torch.empty(need, dtype=torch.uint8, device=device)
    if on_gpu:
      with torch.cuda.device(device):
        meta_d = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8).pin_memory().to(device, non_blocking=True)
        _lib.check(L.mmt_jpeg_pixels(B, meta_d.data_ptr(), coef_t.data_ptr(), n_coef, qtab_t.data_ptr(), out.data_ptr(), out.numel(),
                                     work.data_ptr(), need, torch.cuda.current_stream(device).cuda_stream))
    else:
      _lib.check(L.mmt_jpeg_pixels_host(B, ctypes.addressof(images), coef_t.data_ptr(), n_coef, qtab_t.data_ptr(), out.data_ptr(),
                                        out.numel(), work.data_ptr(), need))
    t = lambda v, dt: torch.tensor(v, dtype=dt).to(device)
    return out, t(offs, torch.int64), t(hs, torch.int32), t(ws, torch.int32)
  coef = torch.empty(n_coef, dtype=torch.int16, pin_memory=on_gpu)
  qtab = torch.empty(B * 192, dtype=torch.int16, pin_memory=on_gpu)       # uint16 values; torch has no such dtype everywhere
  coef_ptr, qtab_ptr = coef.data_ptr(), qtab.data_ptr()

  def entropy(i):                                               # the message is thread-local: read it on the worker
    rc = L.mmt_jpeg_coefficients(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(images[i]), coef_ptr, n_coef, qtab_ptr + i * 384)
    return None if rc == 0 else L.mmt_last_error().decode()

  if workers == 1 or B == 1:
    errors = [entropy(i) for i in range(B)]
  else:
    with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
      errors = list(pool.map(entropy, range(B)))
  for i, msg in enumerate(errors):
    if msg is not None:
      raise ValueError(f'data[{i}] cannot be decoded: {msg}')
  if out is None:
    out = torch.zeros(n_pix, dtype=torch.uint8, device=device)
  elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < n_pix or out.device != device or not out.is_contiguous():
    raise ValueError(f'out must be a contiguous 1-D uint8 tensor of at least {n_pix} bytes on {device}')
  need = L.mmt_jpeg_workspace_bytes(n_coef)
  meta = torch.frombuffer(bytearray(bytes(images)), dtype=torch.uint8)
  if on_gpu:
    with torch.cuda.device(device):
      stream = torch.cuda.current_stream(device).cuda_stream
      coef_d, qtab_d = coef.to(device, non_blocking=True), qtab.to(device, non_blocking=True)
      meta_d = meta.pin_memory().to(device, non_blocking=True)
      work = torch.empty(need, dtype=torch.uint8, device=device)
      _lib.check(L.mmt_jpeg_pixels(B, meta_d.data_ptr(), coef_d.data_ptr(), n_coef, qtab_d.data_ptr(), out.data_ptr(),
                                   out.numel(), work.data_ptr(), need, stream))
  else:
    work = torch.empty(need, dtype=torch.uint8)
    _lib.check(L.mmt_jpeg_pixels_host(B, ctypes.addressof(images), coef_ptr, n_coef, qtab_ptr, out.data_ptr(), out.numel(),
                                      work.data_ptr(), need))
  t = lambda v, dt: torch.tensor(v, dtype=dt).to(device)
  return out, t(offs, torch.int64), t(hs, torch.int32), t(ws, torch.int32)


# ---------------------------------------------------------------------------------------------------
# PNG decode (`tf.io.decode_image`, src/data/data_utils.py:195; the Fashion-Gen shards store PNG files): the host walks
# the chunks and inflates (csrc/png_decode.hip, the library's own inflate; a thread pool spreads the files), the device
# unfilters, de-interlaces, expands and looks the palette up.  DESIGN.md section 4 "PNG decode" has the rules.  Opt-in
# (inflate='device') the host only gathers the IDAT payloads and a kernel inflates them (csrc/png_inflate.hip; DESIGN.md
# section 4 "PNG inflate on the device").
# ---------------------------------------------------------------------------------------------------
PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _encoded_arrays(items):
  bufs = []
  for i, item in enumerate(items):
    if not _is_encoded(item):
      raise ValueError(f'data[{i}] must be bytes, bytearray, memoryview or a uint8 numpy array, got {type(item).__name__}')
    arr = np.ascontiguousarray(item) if isinstance(item, np.ndarray) else np.frombuffer(item, dtype=np.uint8)
    if arr.dtype != np.uint8 or arr.ndim != 1:
      raise ValueError(f'data[{i}] must be a 1-D uint8 array of encoded bytes')
    bufs.append(arr)
  return bufs


def decode_png_images(data, device, *, workers: int = 8, out: torch.Tensor = None, inflate: str = 'host', subseq_bytes: int = None):
  """PNG files -> the packed (pixels uint8 [n], offsets int64 [B], heights int32 [B], widths int32 [B]) tuple on `device`
  that `decode_jpeg_images` returns; image b is RGB, row-major, back to back.

  data: a list of bytes, bytearray, memoryview or uint8 numpy arrays, one file each.  libpng's decode with palette and
  low-bit grey expansion, bit for bit: RGB at depth 8; grey at depths 1, 2, 4, 8 (R = G = B); palette at depths 1, 2, 4, 8
  (an index beyond the palette's entries gives (0, 0, 0)); both interlace methods; no gamma, ancillary chunks ignored.
  Per item mmt_png_info; one buffer of filtered scanlines for the batch (pinned when the device is a GPU); mmt_png_inflate
  spread over `workers` threads (clamped to 1..16); one asynchronous upload of scanlines, palettes and metadata; one
  mmt_png_pixels.  With device 'cpu' the same buffers go through mmt_png_pixels_host.  out: a contiguous uint8 tensor on
  `device` of at least the needed size (allocated when None; bytes behind the last image are not written).  A file the
  library refuses (depth 16, alpha, tRNS, a corrupt or truncated stream) raises ValueError naming the example.

  inflate: 'host' (the default) is the path above.  'device' uploads the compressed bytes instead of the scanlines and
  inflates them in a kernel: mmt_png_gather per file on the thread pool (chunk walk, IDAT payloads back to back) into one
  pinned buffer of compressed bytes, palettes, metadata and stream descriptors; one asynchronous upload;
  mmt_png_scanlines (subseq_bytes: the bytes of a stream a lane owns in a round, a power of two in [8, 128], default
  PNG_INFLATE_SUBSEQ_BYTES); one read-back of the status words; mmt_png_pixels.  A file whose status is not 0 goes
  through mmt_png_inflate on the host: its refusal is raised as the host path raises it, and if the host accepts the
  file its scanlines are uploaded into the image's slice, so the pixels never depend on the path.  With device 'cpu'
  the same buffers go through mmt_png_scanlines_host."""
  from . import _lib
  if inflate not in ('host', 'device'):
    raise ValueError(f"inflate must be 'host' or 'device', got {inflate!r}")
  L = _lib.lib()
  device = torch.device(device)
  items = list(data)
  B = len(items)
  if B == 0:
    raise ValueError('data is empty')
  bufs = _encoded_arrays(items)
  workers = min(max(int(workers), 1), 16)
  if inflate == 'device':
    return _decode_png_device_inflate(L, _lib, bufs, device, workers, out, subseq_bytes)
  images = (_lib.PngImage * B)()
  n_raw, n_pix = 0, 0
  hs, ws, offs = [], [], []
  for i, arr in enumerate(bufs):
    rc = L.mmt_png_info(arr.ctypes.data, arr.size, ctypes.byref(images[i]))
    if rc != 0:
      raise ValueError(f'data[{i}] cannot be decoded: {L.mmt_last_error().decode()}')
    im = images[i]
    im.raw_offset, im.pixel_offset = n_raw, n_pix
    n_raw += im.raw_bytes
    hs.append(im.height); ws.append(im.width); offs.append(n_pix)
    n_pix += im.height * im.width * 3
  on_gpu = device.type == 'cuda'
  o_pal = _up16(n_raw)                                           # one buffer: scanlines | palettes | metadata
  o_img = o_pal + B * 768
  stage = torch.empty(_up16(o_img + ctypes.sizeof(images)), dtype=torch.uint8, pin_memory=on_gpu)
  base = stage.data_ptr()

  def inflate(i):                                               # the message is thread-local: read it on the worker
    rc = L.mmt_png_inflate(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(images[i]), base, n_raw, base + o_pal + i * 768)
    return None if rc == 0 else L.mmt_last_error().decode()

  if workers == 1 or B == 1:
    errors = [inflate(i) for i in range(B)]
  else:
    with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
      errors = list(pool.map(inflate, range(B)))
  for i, msg in enumerate(errors):
    if msg is not None:
      raise ValueError(f'data[{i}] cannot be decoded: {msg}')
  stage.numpy()[o_img:o_img + ctypes.sizeof(images)] = np.frombuffer(bytes(images), dtype=np.uint8)
  if out is None:
    out = torch.zeros(n_pix, dtype=torch.uint8, device=device)
  elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < n_pix or out.device != device or not out.is_contiguous():
    raise ValueError(f'out must be a contiguous 1-D uint8 tensor of at least {n_pix} bytes on {device}')
  need = L.mmt_png_workspace_bytes(n_raw)
  if on_gpu:
    with torch.cuda.device(device):
      stage_d = stage.to(device, non_blocking=True)
      work = torch.empty(need, dtype=torch.uint8, device=device)
      d = stage_d.data_ptr()
      _lib.check(L.mmt_png_pixels(B, d + o_img, d, n_raw, d + o_pal, out.data_ptr(), out.numel(), work.data_ptr(), need,
                                  torch.cuda.current_stream(device).cuda_stream))
  else:
    work = torch.empty(need, dtype=torch.uint8)
    _lib.check(L.mmt_png_pixels_host(B, base + o_img, base, n_raw, base + o_pal, out.data_ptr(), out.numel(), work.data_ptr(), need))
  t = lambda v, dt: torch.tensor(v, dtype=dt).to(device)
  return out, t(offs, torch.int64), t(hs, torch.int32), t(ws, torch.int32)


# Default of the device inflate, from profiles/png_inflate_timing.json ("PNG inflate on the device").
PNG_INFLATE_SUBSEQ_BYTES = 16


def _decode_png_device_inflate(L, _lib, bufs, device, workers, out, subseq_bytes):
  """The `inflate='device'` path of decode_png_images."""
  B = len(bufs)
  sb = PNG_INFLATE_SUBSEQ_BYTES if subseq_bytes is None else int(subseq_bytes)
  if sb < 8 or sb > 128 or sb & (sb - 1):
    raise ValueError(f'subseq_bytes must be a power of two in [8, 128], got {subseq_bytes!r}')
  images = (_lib.PngImage * B)()
  streams = (_lib.PngStream * B)()
  n_raw, n_pix, n_comp = 0, 0, 0
  hs, ws, offs = [], [], []
  for i, arr in enumerate(bufs):
    rc = L.mmt_png_info(arr.ctypes.data, arr.size, ctypes.byref(images[i]))
    if rc != 0:
      raise ValueError(f'data[{i}] cannot be decoded: {L.mmt_last_error().decode()}')
    im = images[i]
    im.raw_offset, im.pixel_offset = n_raw, n_pix
    n_raw += im.raw_bytes
    hs.append(im.height); ws.append(im.width); offs.append(n_pix)
    n_pix += im.height * im.width * 3
    streams[i].comp_offset = n_comp                             # the IDAT payloads are fewer bytes than the file
    n_comp += arr.size
  on_gpu = device.type == 'cuda'
  o_pal = _up16(n_comp)                                          # one buffer: compressed bytes | palettes | metadata | streams
  o_img = o_pal + B * 768
  o_str = _up16(o_img + ctypes.sizeof(images))
  stage = torch.empty(_up16(o_str + ctypes.sizeof(streams)), dtype=torch.uint8, pin_memory=on_gpu)
  base = stage.data_ptr()

  def host_inflate(i):                                          # (scanlines, None) or (None, the host path's message)
    im = _lib.PngImage.from_buffer_copy(images[i])
    im.raw_offset = 0
    raw = np.empty(max(im.raw_bytes, 1), dtype=np.uint8)
    pal = np.empty(768, dtype=np.uint8)
    rc = L.mmt_png_inflate(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(im), raw.ctypes.data, im.raw_bytes, pal.ctypes.data)
    return (raw, None) if rc == 0 else (None, L.mmt_last_error().decode())

  def gather(i):                                                # the message is thread-local: read it on the worker
    rc = L.mmt_png_gather(bufs[i].ctypes.data, bufs[i].size, ctypes.byref(images[i]), base, n_comp, ctypes.byref(streams[i]),
                          base + o_pal + i * 768)
    if rc == 0:
      return None
    msg = L.mmt_last_error().decode()
    return host_inflate(i)[1] or msg                            # the host path's words for what it refuses too

  if workers == 1 or B == 1:
    errors = [gather(i) for i in range(B)]
  else:
    with ThreadPoolExecutor(max_workers=min(workers, B)) as pool:
      errors = list(pool.map(gather, range(B)))
  for i, msg in enumerate(errors):
    if msg is not None:
      raise ValueError(f'data[{i}] cannot be decoded: {msg}')
  view = stage.numpy()
  view[o_img:o_img + ctypes.sizeof(images)] = np.frombuffer(bytes(images), dtype=np.uint8)
  view[o_str:o_str + ctypes.sizeof(streams)] = np.frombuffer(bytes(streams), dtype=np.uint8)
  if out is None:
    out = torch.zeros(n_pix, dtype=torch.uint8, device=device)
  elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < n_pix or out.device != device or not out.is_contiguous():
    raise ValueError(f'out must be a contiguous 1-D uint8 tensor of at least {n_pix} bytes on {device}')
  need_inf = L.mmt_png_scanlines_workspace_bytes(B)
  need = L.mmt_png_workspace_bytes(n_raw)

  def repair(raw_t, status):                                    # files the kernel refused: the host decides
    for i in np.flatnonzero(status):
      lines, msg = host_inflate(int(i))
      if msg is not None:
        raise ValueError(f'data[{int(i)}] cannot be decoded: {msg}')
      at = images[int(i)].raw_offset
      raw_t[at:at + lines.size].copy_(torch.from_numpy(lines))

  if on_gpu:
    with torch.cuda.device(device):
      stream = torch.cuda.current_stream(device).cuda_stream
      stage_d = stage.to(device, non_blocking=True)
      raw_t = torch.empty(n_raw, dtype=torch.uint8, device=device)
      status_t = torch.empty(B, dtype=torch.int32, device=device)
      work_inf = torch.empty(need_inf, dtype=torch.uint8, device=device)
      work = torch.empty(need, dtype=torch.uint8, device=device)
      d = stage_d.data_ptr()
      _lib.check(L.mmt_png_scanlines(B, d + o_img, d + o_str, d, n_comp, raw_t.data_ptr(), n_raw, status_t.data_ptr(), sb,
                                     work_inf.data_ptr(), need_inf, stream))
      repair(raw_t, status_t.cpu().numpy())
      _lib.check(L.mmt_png_pixels(B, d + o_img, raw_t.data_ptr(), n_raw, d + o_pal, out.data_ptr(), out.numel(), work.data_ptr(), need,
                                  stream))
  else:
    raw_t = torch.empty(n_raw, dtype=torch.uint8)
    status_t = torch.empty(B, dtype=torch.int32)
    work_inf = torch.empty(need_inf, dtype=torch.uint8)
    work = torch.empty(need, dtype=torch.uint8)
    _lib.check(L.mmt_png_scanlines_host(B, base + o_img, base + o_str, base, n_comp, raw_t.data_ptr(), n_raw, status_t.data_ptr(), sb,
                                        work_inf.data_ptr(), need_inf))
    repair(raw_t, status_t.numpy())
    _lib.check(L.mmt_png_pixels_host(B, base + o_img, raw_t.data_ptr(), n_raw, base + o_pal, out.data_ptr(), out.numel(), work.data_ptr(),
                                     need))
  t = lambda v, dt: torch.tensor(v, dtype=dt).to(device)
  return out, t(offs, torch.int64), t(hs, torch.int32), t(ws, torch.int32)


def _is_png(item) -> bool:
  return _is_encoded(item) and bytes(memoryview(item)[:8]) == PNG_SIGNATURE


def decode_images(data, device, *, workers: int = 8, out: torch.Tensor = None, entropy: str = 'host', subseq_bytes: int = None,
                  max_rounds: int = None, uploaded=None, png_inflate: str = 'host'):
  """`tf.io.decode_image` for a list of encoded files, JPEG or PNG each: the packed (pixels, offsets, heights, widths)
  tuple on `device`, images in the order of `data`.  An item that starts with the 8-byte PNG signature is a PNG file;
  everything else is taken for a JPEG file (and refused by `decode_jpeg_images` if it is none).

  A list without PNG files goes to `decode_jpeg_images` with exactly the arguments given; a list of PNG files only goes to
  `decode_png_images` (workers, out).  A mixed list decodes the two groups into disjoint slices of one `out` -- the JPEG
  files first, then the PNG files -- and returns offsets, heights and widths in the order of `data`; the images are then not
  in the order of their offsets, which the packed layout allows.  entropy, subseq_bytes and max_rounds are
  `decode_jpeg_images`'s; `uploaded` offsets are passed on for the JPEG items only.  png_inflate is `decode_png_images`'s
  `inflate` ('host' or 'device') and takes effect for the PNG items only.  A refusal names the example by its index in
  `data`."""
  if png_inflate not in ('host', 'device'):
    raise ValueError(f"png_inflate must be 'host' or 'device', got {png_inflate!r}")
  items = list(data)
  png = [i for i, item in enumerate(items) if _is_png(item)]
  if not png:
    return decode_jpeg_images(items, device, workers=workers, out=out, entropy=entropy, subseq_bytes=subseq_bytes, max_rounds=max_rounds,
                              uploaded=uploaded)
  if len(png) == len(items):
    return decode_png_images(items, device, workers=workers, out=out, inflate=png_inflate)
  device = torch.device(device)
  jpg = [i for i in range(len(items)) if i not in set(png)]

  def group(index, call):                                       # a refusal of a group names the example by its place in data
    try:
      return call()
    except ValueError as e:
      msg = str(e)
      if msg.startswith('data['):
        k = int(msg[5:msg.index(']')])
        raise ValueError(f'data[{index[k]}]' + msg[msg.index(']') + 1:]) from None
      raise

  up = None if uploaded is None else (uploaded[0], [uploaded[1][i] for i in jpg])
  jpeg_kw = dict(workers=workers, entropy=entropy, subseq_bytes=subseq_bytes, max_rounds=max_rounds, uploaded=up)
  if out is None:                                               # the sizes are not known yet: decode, then join
    a = group(jpg, lambda: decode_jpeg_images([items[i] for i in jpg], device, **jpeg_kw))
    b = group(png, lambda: decode_png_images([items[i] for i in png], device, workers=workers, inflate=png_inflate))
    pixels = torch.cat([a[0], b[0]])
  else:
    if out.dtype != torch.uint8 or out.dim() != 1 or out.device != device or not out.is_contiguous():
      raise ValueError(f'out must be a contiguous 1-D uint8 tensor on {device}')
    a = group(jpg, lambda: decode_jpeg_images([items[i] for i in jpg], device, out=out, **jpeg_kw))
    n_a = int(a[1][-1]) + int(a[2][-1]) * int(a[3][-1]) * 3
    if out.numel() <= n_a:
      raise ValueError(f'out must hold more than the {n_a} bytes of the JPEG files')
    b = group(png, lambda: decode_png_images([items[i] for i in png], device, workers=workers, out=out[n_a:], inflate=png_inflate))
    pixels = out
  n_a = int(a[0].numel()) if out is None else n_a
  B = len(items)
  order = torch.tensor(jpg + png, dtype=torch.int64, device=device)
  offsets = torch.empty(B, dtype=torch.int64, device=device)
  heights = torch.empty(B, dtype=torch.int32, device=device)
  widths = torch.empty(B, dtype=torch.int32, device=device)
  offsets[order] = torch.cat([a[1], b[1] + n_a])
  heights[order] = torch.cat([a[2], b[2]])
  widths[order] = torch.cat([a[3], b[3]])
  return pixels, offsets, heights, widths


def images_to_patch_features(images, image_size: int, patch_size: int, *, flip: torch.Tensor = None,
                             out_dtype: torch.dtype = torch.float32, keep_unnormalized: bool = False,
                             output_channel_bits: int = 0, mean=IMAGENET_DEFAULT_MEAN, device=None,
                             entropy: str = 'host', png_inflate: str = 'host') -> Dict[str, torch.Tensor]:
  """The tensor half of `decode_fn` (src/data/data_utils.py:195-222) for a batch of decoded RGB images of any sizes.

  images: list of uint8 [h, w, 3] tensors, or an already packed (pixels uint8 [n], offsets int64 [B], heights int32
  [B], widths int32 [B]) tuple (example b is heights[b] x widths[b] x 3 bytes, row-major, from pixels[offsets[b]]), or a
  list of encoded JPEG or PNG files (bytes, bytearray, memoryview, uint8 numpy arrays; the two may be mixed), which
  `decode_images` decodes first onto `device` (default: the GPU when there is one), JPEG files with its `entropy` mode,
  PNG files with its `png_inflate` mode.
  Per example: x = u8 / 255; bilinear resize to image_size x image_size (tf.image.resize, TF2 defaults);
  patch_embeddings from (r - mean) / mean -- the reference's line 204 divides by the MEAN -- and
  unnormalized_patch_embeddings from r; flip [B] (bool / uint8; the reference's training-time coin, :209-211, as an
  explicit input) mirrors both left-right after the resize; patches as `convert_image_to_patches`; mpp_label_ids as
  `make_mpp_label_ids(unnormalized, patch_size, 3, output_channel_bits)` (0: none).
  Returns patch_embeddings [B, P*P, patch_size^2 * 3] in `out_dtype` (float32 | bfloat16), num_image_wordpieces
  (2 + P*P: [CLS], [PATCH] and the patches, :239) and, when asked for, unnormalized_patch_embeddings (float32) and
  mpp_label_ids [B, P*P] int32.  On the GPU all of it is one launch of mmt_image_patches; CPU tensors go through the
  same arithmetic in torch ops."""
  image_size, patch_size, bits = int(image_size), int(patch_size), int(output_channel_bits)
  if image_size < 1 or patch_size < 1:
    raise ValueError('image_size and patch_size must be positive')
  if patch_size > image_size:
    raise ValueError(f'patch_size {patch_size} exceeds image_size {image_size}: no whole patch')
  if out_dtype not in (torch.float32, torch.bfloat16):
    raise ValueError(f'out_dtype must be float32 or bfloat16, got {out_dtype}')
  if not 0 <= bits <= 8:
    raise ValueError('output_channel_bits must be in [0, 8]')
  if len(mean) != 3 or any(float(m) == 0.0 for m in mean):
    raise ValueError('mean must be three non-zero numbers')
  images = _maybe_decode(images, _default_device(device), entropy, png_inflate=png_inflate)
  pixels, offsets, heights, widths = _check_packed(images) if isinstance(images, tuple) else _pack_images(list(images))
  B, dev = offsets.shape[0], pixels.device
  if flip is not None:
    if flip.shape != (B,) or flip.dtype not in (torch.bool, torch.uint8) or flip.device != dev:
      raise ValueError('flip must be a bool or uint8 [B] tensor on the images\' device')
    flip = flip.to(torch.uint8).contiguous()
  P = image_size // patch_size
  E = patch_size * patch_size * 3
  out = {'num_image_wordpieces': 2 + P * P}
  if pixels.is_cuda:
    from . import _lib
    d = _lib.ImageDesc()
    d.B, d.image_size, d.patch_size, d.channel_bits = B, image_size, patch_size, bits
    d.out_dtype = _lib.MMT_F32 if out_dtype == torch.float32 else _lib.MMT_BF16
    d.mean[:] = [float(m) for m in mean]
    norm = torch.empty(B, P * P, E, dtype=out_dtype, device=dev)
    unnorm = torch.empty(B, P * P, E, dtype=torch.float32, device=dev) if keep_unnormalized else None
    ids = torch.empty(B, P * P, dtype=torch.int32, device=dev) if bits else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().mmt_image_patches(d, pixels.data_ptr(), pixels.numel(), offsets.data_ptr(), heights.data_ptr(),
                                            widths.data_ptr(), ptr(flip), norm.data_ptr(), ptr(unnorm), ptr(ids),
                                            torch.cuda.current_stream(dev).cuda_stream))
  else:
    rows = []
    for b in range(B):
      h, w, o = int(heights[b]), int(widths[b]), int(offsets[b])
      r = _resize_bilinear_u8(pixels[o:o + h * w * 3].reshape(h, w, 3), image_size)
      rows.append(torch.flip(r, dims=(1,)) if flip is not None and bool(flip[b]) else r)
    r = convert_image_to_patches(torch.stack(rows), patch_size)
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32).repeat(patch_size * patch_size)
    norm = ((r - m) / m).to(out_dtype)
    unnorm = r if keep_unnormalized else None
    ids = make_mpp_label_ids(r, patch_size, 3, bits) if bits else None
  out['patch_embeddings'] = norm
  if keep_unnormalized:
    out['unnormalized_patch_embeddings'] = unnorm
  if bits:
    out['mpp_label_ids'] = ids
  return out


# ---------------------------------------------------------------------------------------------------
# RandAugment (`rand_aug.distort`, src/data/data_utils.py:125-145, 199-202): one of 14 operations per decoded uint8
# image, before the front end above.  The definitions are DESIGN.md section 4; csrc/rand_augment.hip runs them on the
# device, the torch ops below are the same arithmetic for CPU tensors (integers, and float32 with every product and
# sum a separate op), bit for bit.
# ---------------------------------------------------------------------------------------------------
RAND_AUGMENT_OPS = ('AutoContrast', 'Equalize', 'Rotate', 'Posterize', 'Solarize', 'Color', 'Contrast', 'Brightness',
                    'Sharpness', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'SolarizeAdd')


def rand_augment_plan(heights: torch.Tensor, widths: torch.Tensor, *, magnitude: float = 10.0,
                      translate_const: float = 100.0, generator: torch.Generator = None, ops: torch.Tensor = None,
                      signs: torch.Tensor = None):
  """The per-example operation and its arguments: (op int32 [B], arg float32 [B, 8]) on the device of `heights`.

  `ops` (ids into RAND_AUGMENT_OPS; -1 = none) and `signs` (+1 / -1, any non-negative value counts as +1) are drawn
  with `generator` -- first the ids, uniform over the 14, then one fair coin per example -- unless given.  With
  L = magnitude / 10 (10 is the Model Garden's default, which `RandAugment(num_layers=1)` takes):
    Color, Contrast, Brightness, Sharpness   arg[0] = 1.8 L + 0.1
    Posterize  arg[0] = int(4 L) bits;   Solarize  arg[0] = int(256 L);   SolarizeAdd  arg[0] = int(110 L)
    arg[0..5] = a0 a1 a2 b0 b1 b2 of the affine operations, with t = +-30 degrees * L, c = cos t, s = sin t:
      Rotate      a = [c, -s, ((w-1) - (c (w-1) - s (h-1))) / 2],   b = [s, c, ((h-1) - (s (w-1) + c (h-1))) / 2]
      ShearX      a = [1, +-0.3 L, 0],  b = [0, 1, 0];      ShearY      a = [1, 0, 0],  b = [+-0.3 L, 1, 0]
      TranslateX  a = [1, 0, +-translate_const L],  b = [0, 1, 0];   TranslateY  a = [1, 0, 0],  b = [0, 1, +-translate_const L]
  Coefficients are computed in float64 and rounded once to float32.  Everything is torch ops on the tensors' device:
  no value is read back to the host."""
  if heights.dim() != 1 or heights.shape != widths.shape or heights.device != widths.device:
    raise ValueError('heights and widths must be [B] tensors on one device')
  B, dev = heights.shape[0], heights.device
  if ops is None:
    ops = torch.randint(0, len(RAND_AUGMENT_OPS), (B,), generator=generator, device=dev)
  elif ops.shape != (B,) or ops.device != dev:
    raise ValueError('ops must be a [B] tensor on the device of heights')
  if signs is None:
    signs = torch.rand(B, generator=generator, device=dev) < 0.5
    signs = torch.where(signs, -1.0, 1.0)
  elif signs.shape != (B,) or signs.device != dev:
    raise ValueError('signs must be a [B] tensor on the device of heights')
  op = ops.to(torch.int32)
  sg = torch.where(signs.to(torch.float64) < 0, -1.0, 1.0).to(torch.float64)
  L = float(magnitude) / 10.0
  f64 = lambda v: torch.full((B,), float(v), dtype=torch.float64, device=dev)
  zero, one = f64(0.0), f64(1.0)
  w1, h1 = widths.to(torch.float64) - 1.0, heights.to(torch.float64) - 1.0
  theta = sg * math.radians(30.0 * L)
  c, s = torch.cos(theta), torch.sin(theta)
  shear, shift = sg * (0.3 * L), sg * (float(translate_const) * L)
  rows = {           # op id -> the six (or one) leading arguments
      2: (c, -s, (w1 - (c * w1 - s * h1)) / 2.0, s, c, (h1 - (s * w1 + c * h1)) / 2.0),
      3: (f64(int(4 * L)),), 4: (f64(int(256 * L)),), 13: (f64(int(110 * L)),),
      5: (f64(1.8 * L + 0.1),), 6: (f64(1.8 * L + 0.1),), 7: (f64(1.8 * L + 0.1),), 8: (f64(1.8 * L + 0.1),),
      9: (one, shear, zero, zero, one, zero), 10: (one, zero, zero, shear, one, zero),
      11: (one, zero, shift, zero, one, zero), 12: (one, zero, zero, zero, one, shift),
  }
  arg = torch.zeros(B, 8, dtype=torch.float64, device=dev)
  for k, vals in rows.items():
    row = torch.stack(list(vals) + [zero] * (8 - len(vals)), dim=1)
    arg = torch.where((op == k)[:, None], row, arg)
  return op, arg.to(torch.float32)


def _blend_u8(a: torch.Tensor, b: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
  """blend(a, b, f) = trunc(clip(a + f * (b - a), 0, 255)) on integer tensors, f a float32 scalar tensor: the difference
  is exact, the product and the sum are separate float32 ops."""
  d = (b - a).to(torch.float32)
  t = a.to(torch.float32) + f * d
  return t.clamp(0.0, 255.0).to(torch.int32)


def _grey(im: torch.Tensor) -> torch.Tensor:
  """Pillow's 'L' of an int32 [h, w, 3] image."""
  return (19595 * im[..., 0] + 38470 * im[..., 1] + 7471 * im[..., 2] + 32768) >> 16


def _rand_augment_image(u8: torch.Tensor, op: int, arg: torch.Tensor) -> torch.Tensor:
  """One operation on one uint8 [h, w, 3] CPU tensor; arg float32 [8]."""
  if not 0 <= op <= 13:
    return u8.clone()
  h, w = u8.shape[0], u8.shape[1]
  im = u8.to(torch.int32)
  f = arg[0]
  if op == 0:
    out = im.clone()
    for c in range(3):
      lo, hi = int(im[..., c].min()), int(im[..., c].max())
      if hi > lo:
        scale = torch.tensor(255.0, dtype=torch.float32) / torch.tensor(float(hi - lo), dtype=torch.float32)
        off = torch.tensor(-float(lo), dtype=torch.float32) * scale
        out[..., c] = (im[..., c].to(torch.float32) * scale + off).clamp(0.0, 255.0).to(torch.int32)
  elif op == 1:
    out = im.clone()
    for c in range(3):
      hist = torch.bincount(im[..., c].reshape(-1).to(torch.int64), minlength=256)
      last = int(hist[int(torch.nonzero(hist)[-1])])
      step = (int(hist.sum()) - last) // 255
      if step > 0:
        lut = ((torch.cumsum(hist, 0) - hist + step // 2) // step).clamp(max=255)
        lut[0] = 0
        out[..., c] = lut[im[..., c].to(torch.int64)].to(torch.int32)
  elif op == 3:
    shift = 8 - min(max(int(f), 0), 8)
    out = (im >> shift) << shift
  elif op == 4:
    out = torch.where(im < int(f), im, 255 - im)
  elif op == 13:
    add = min(max(int(f), -255), 255)
    out = torch.where(im < 128, (im + add).clamp(0, 255), im)
  elif op == 5:
    out = _blend_u8(_grey(im)[..., None], im, f)
  elif op == 6:
    g = _grey(im).to(torch.int64)
    n = g.numel()
    m = (int(g.sum()) + n // 2) // n
    out = _blend_u8(torch.full_like(im, m), im, f)
  elif op == 7:
    out = _blend_u8(torch.zeros_like(im), im, f)
  elif op == 8:
    out = im.clone()
    if h >= 3 and w >= 3:
      acc = 5 * im[1:-1, 1:-1]
      for dy in (0, 1, 2):
        for dx in (0, 1, 2):
          if (dy, dx) != (1, 1):
            acc = acc + im[dy:dy + h - 2, dx:dx + w - 2]
      out[1:-1, 1:-1] = _blend_u8(acc // 13, im[1:-1, 1:-1], f)
  else:                                                    # the affine gather: Rotate, ShearX / Y, TranslateX / Y
    x = torch.arange(w, dtype=torch.float32)[None, :]
    y = torch.arange(h, dtype=torch.float32)[:, None]
    sx = (arg[0] * x + arg[1] * y) + arg[2]
    sy = (arg[3] * x + arg[4] * y) + arg[5]
    rx, ry = torch.floor(sx + 0.5), torch.floor(sy + 0.5)
    ok = (rx.abs() < 2.0 ** 30) & (ry.abs() < 2.0 ** 30)   # false for NaN and infinity as well
    ix = torch.where(ok, rx, torch.full_like(rx, -1.0)).to(torch.int64)
    iy = torch.where(ok, ry, torch.full_like(ry, -1.0)).to(torch.int64)
    ok = ok & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    src = im[iy.clamp(0, h - 1), ix.clamp(0, w - 1)]
    out = torch.where(ok[..., None], src, torch.full_like(src, 128))
  return out.to(torch.uint8)


def rand_augment(images, op: torch.Tensor, arg: torch.Tensor, out: torch.Tensor = None):
  """One RandAugment operation per image.  images: list of uint8 [h, w, 3] tensors or a packed (pixels, offsets, heights,
  widths) tuple, as `images_to_patch_features` takes; op int32 [B] (ids into RAND_AUGMENT_OPS, any other value copies
  the image) and arg float32 [B, 8] as `rand_augment_plan` makes them; out: a uint8 tensor of the size of pixels that
  does not overlap it (allocated when None).  Returns the packed tuple with the new pixels (offsets, heights and widths
  are the inputs'), which `images_to_patch_features` consumes unchanged.  Bytes of `out` between the images are not
  written (zero when it is allocated here).  On the GPU it is one mmt_rand_augment call; CPU tensors go through the
  same arithmetic in torch ops, bit-identical to the kernels."""
  pixels, offsets, heights, widths = _check_packed(images) if isinstance(images, tuple) else _pack_images(list(images))
  B, dev = offsets.shape[0], pixels.device
  if op.shape != (B,) or op.dtype != torch.int32 or op.device != dev:
    raise ValueError('op must be an int32 [B] tensor on the images\' device')
  if arg.shape != (B, 8) or arg.dtype != torch.float32 or arg.device != dev:
    raise ValueError('arg must be a float32 [B, 8] tensor on the images\' device')
  if out is None:
    out = torch.zeros_like(pixels)
  elif out.dtype != torch.uint8 or out.shape != pixels.shape or out.device != dev or not out.is_contiguous():
    raise ValueError('out must be a contiguous uint8 tensor of the size of pixels on the images\' device')
  elif out.data_ptr() < pixels.data_ptr() + pixels.numel() and pixels.data_ptr() < out.data_ptr() + out.numel():
    raise ValueError('out must not overlap pixels')
  op, arg = op.contiguous(), arg.contiguous()
  if pixels.is_cuda:
    from . import _lib
    L = _lib.lib()
    need = L.mmt_rand_augment_workspace_bytes(B)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(L.mmt_rand_augment(B, pixels.data_ptr(), pixels.numel(), offsets.data_ptr(), heights.data_ptr(),
                                  widths.data_ptr(), op.data_ptr(), arg.data_ptr(), out.data_ptr(), ws.data_ptr(), need,
                                  torch.cuda.current_stream(dev).cuda_stream))
  else:
    for b in range(B):
      h, w, o = int(heights[b]), int(widths[b]), int(offsets[b])
      im = pixels[o:o + h * w * 3].reshape(h, w, 3)
      out[o:o + h * w * 3] = _rand_augment_image(im, int(op[b]), arg[b]).reshape(-1)
  return out, offsets, heights, widths


def decode_image_features(data_config, images, *, generator: torch.Generator = None,
                          out_dtype: torch.dtype = torch.float32, keep_unnormalized: bool = False,
                          device=None, entropy: str = 'host', uploaded=None, png_inflate: str = 'host') -> Dict[str, torch.Tensor]:
  """`decode_fn` (src/data/data_utils.py:195-222) as the data config drives it.  images: a list of uint8 [h, w, 3] tensors,
  a packed tuple, or a list of encoded JPEG or PNG files, which `decode_images` decodes first onto `device` (default: the
  GPU when there is one; `entropy` is the JPEG decode's mode, `png_inflate` the PNG decode's):
    is_training and use_rand_aug   `rand_augment` with a `rand_augment_plan` drawn from `generator`      (:199-202)
    is_training                    one flip coin per example, flipped when u > 0.5                        (:209-211)
    then `images_to_patch_features` with the config's image_size, patch_size and, where the config has the field,
    output_channel_bits (the pretraining loader's MPP ids).
  Draws come from `generator` in this order: operation ids, signs, flip coins.  With is_training false the result is
  `images_to_patch_features(images, image_size, patch_size, ...)` bit for bit.  `uploaded` is `decode_jpeg_images`'s; PNG
  files do not use it."""
  images = _maybe_decode(images, _default_device(device), entropy, uploaded, png_inflate)
  packed = _check_packed(images) if isinstance(images, tuple) else _pack_images(list(images))
  pixels, offsets, heights, widths = packed
  flip = None
  if bool(data_config.is_training):
    if bool(getattr(data_config, 'use_rand_aug', False)):
      op, arg = rand_augment_plan(heights, widths, generator=generator)
      packed = rand_augment(packed, op, arg)
    flip = torch.rand(offsets.shape[0], generator=generator, device=pixels.device) > 0.5
  return images_to_patch_features(packed, int(data_config.image_size), int(data_config.patch_size), flip=flip,
                                  out_dtype=out_dtype, keep_unnormalized=keep_unnormalized,
                                  output_channel_bits=int(getattr(data_config, 'output_channel_bits', 0)))


def make_matching_features(features: Dict[str, torch.Tensor], image_keys: torch.Tensor,
                           negative_positive_ratio: int = 1, min_shift: int = 5) -> Dict[str, torch.Tensor]:
  """In-batch negatives for image-text matching.  The batch is sorted by image (equal images adjacent),
  image-side features are tiled `ratio + 1` times, text-side features of copy i are rolled by
  `min_shift + i` examples, and copy 0 is the positive set: itm_label_ids = 1 for the first batch_size
  examples, itm_pos_weights = 1 + label * (ratio - 1)."""
  B = image_keys.shape[0]
  if not B > negative_positive_ratio + 1 + min_shift:
    raise ValueError('batch_size must exceed negative_positive_ratio + 1 + min_shift')
  if negative_positive_ratio <= 0:
    raise ValueError('negative_positive_ratio must be positive')
  _, idx = torch.unique(image_keys, return_inverse=True)     # ids in order of first appearance are not
  first = torch.full((int(idx.max()) + 1,), B, dtype=torch.long, device=idx.device)   # guaranteed: re-rank
  first.scatter_reduce_(0, idx, torch.arange(B, device=idx.device), reduce='amin')
  rank = torch.argsort(torch.argsort(first))[idx]            # tf.unique numbering: by first appearance
  order = torch.argsort(rank, stable=True)
  out = {k: v[order] for k, v in features.items()}
  copies = negative_positive_ratio + 1
  for k in ('patch_token_ids', 'patch_embeddings', 'num_image_wordpieces'):
    if k in out:
      out[k] = out[k].repeat(copies, *([1] * (out[k].dim() - 1)))
  base = torch.arange(B, device=image_keys.device)
  perm = torch.cat([base] + [torch.roll(base, shifts=min_shift + i) for i in range(1, copies)])
  for k in ('text_token_ids', 'num_text_wordpieces', 'mlm_positions', 'mlm_label_ids', 'mlm_label_weights',
            'mpp_positions', 'mpp_label_ids', 'mpp_label_weights'):
    if k in out:
      out[k] = out[k][perm]
  label = torch.zeros(B * copies, device=image_keys.device)
  label[:B] = 1.0
  out['itm_label_ids'] = label.to(torch.int32)
  out['itm_label_weights'] = torch.ones_like(label)
  out['itm_pos_weights'] = 1.0 + label * (negative_positive_ratio - 1)
  return out


def matching_batch_size(data_config, batch_size_per_replica: int) -> int:
  """Examples the matching step needs in hand so that no roll creates a false negative
  (`MmtClassificationDataLoader.load`, src/data/classification_dataloader.py:132-137)."""
  max_shift = int(data_config.negative_positive_ratio) + int(data_config.min_shift)
  return (max_shift // batch_size_per_replica + 2) * batch_size_per_replica


def make_matching_features_from_config(data_config, features: Dict[str, torch.Tensor],
                                       image_keys: torch.Tensor) -> Dict[str, torch.Tensor]:
  """`get_matching_fn(config, batch, config.negative_positive_ratio)` of the classification loader
  (classification_dataloader.py:138-140): the data config's `negative_positive_ratio` and `min_shift` drive the
  in-batch negatives (pretraining fixes the ratio at 1, pretrain_dataloader.py:184)."""
  return make_matching_features(features, image_keys,
                                negative_positive_ratio=int(getattr(data_config, 'negative_positive_ratio', 1)),
                                min_shift=int(data_config.min_shift))


def make_retrieval_labels(features: Dict[str, torch.Tensor], pos_weight: float = 1.0) -> Dict[str, torch.Tensor]:
  """`get_retrieval_label_fn` (src/data/data_utils.py:744-760): label 1 where the image is the text's ground-truth
  image, weight `pos_weight` on those pairs and 1 elsewhere (`MmtRetrievalDataConfig.pos_weight`)."""
  label = (features['image_index'] == features['gt_image_index']).to(torch.int32)
  out = dict(features)
  out['label_ids'] = label
  out['label_weights'] = label.to(torch.float32) * (float(pos_weight) - 1.0) + 1.0
  return out


# ---------------------------------------------------------------------------------------------------
# MLM / MPP masking (`get_masking_fn` -> `make_mlm_and_mpp_features`, src/data/data_utils.py:383-639),
# batched on the device.  The reference calls tf_text.mask_language_model with a RandomItemSelector and a
# MaskValuesChooser (tensorflow_text 2.5.0, src/requirements.txt); their published algorithm is restated
# here with the RANDOM DRAWS AS EXPLICIT INPUTS (one shuffle key and one value-choice uniform per item, one
# replacement id per token), so that the index outputs are a deterministic, bit-exact function of them.
# ---------------------------------------------------------------------------------------------------
def random_item_masking(token_ids: torch.Tensor, n_tokens: torch.Tensor, *, selection_rate: float,
                        max_selections: int, unselectable_ids, mask_token_id: int, item_keys: torch.Tensor,
                        value_u: torch.Tensor, random_ids: torch.Tensor, word_start: torch.Tensor = None,
                        mask_token_rate: float = 0.8, random_token_rate: float = 0.1, kernel: bool = None):
  """tf_text.mask_language_model(ids, RandomItemSelector(max_selections, selection_rate, unselectable_ids),
  MaskValuesChooser(vocab, mask_token_id, mask_token_rate)) for a padded batch.

  token_ids [B,T] int32 (entries at or beyond n_tokens[b] are padding); word_start [B,T] bool marks the first
  wordpiece of every item (None: every token is an item -- `mlm_use_whole_word=False`, data_utils.py:598-600).
  item_keys / value_u [B,T] float32 in [0,1): entry i belongs to item i of the row; random_ids [B,T] int32.
  Items with any unselectable wordpiece are never chosen; of the n selectable items
  min(ceil(n * selection_rate), max_selections) are chosen -- those with the smallest shuffle keys; a chosen
  item becomes [MASK] when its value_u < mask_token_rate, random ids when < mask_token_rate +
  random_token_rate, and stays as it is otherwise.
  Returns (masked_token_ids [B,T], positions [B,T] (ascending, first n_masked valid, rest 0), n_masked [B],
  original ids at those positions [B,T]).

  kernel: None -- GPU tensors inside the limits of `mmt_item_masking` (include/mmt_layer.h: int32 token_ids, T <= 8192,
  at most 8 unselectable ids; lengths [B], draws [B,T], `word_start` bool [B,T] or None) take its one launch on the
  current stream, everything else the torch ops below; False --
  the torch ops, the definition and the yardstick; True -- the kernel, or `mmt_item_masking_host` on CPU tensors, and
  an error outside the limits.  The three give the same bits."""
  unselectable_ids = tuple(unselectable_ids)
  if kernel is None:
    kernel = token_ids.is_cuda and _item_masking_kernel_serves(token_ids, n_tokens, unselectable_ids, mask_token_id, item_keys, value_u,
                                                               random_ids, word_start)
  if kernel:
    return _random_item_masking_kernel(token_ids, n_tokens, selection_rate, max_selections, [int(u) for u in unselectable_ids],
                                       mask_token_id, item_keys, value_u, random_ids, word_start, mask_token_rate, random_token_rate)
  B, T = token_ids.shape
  dev = token_ids.device
  pos = torch.arange(T, device=dev)[None]
  valid = pos < n_tokens[:, None]
  if word_start is None:
    item = pos.expand(B, T)
  else:
    item = torch.cumsum((word_start & valid).to(torch.int64), 1) - 1
  item = torch.where(valid, item, torch.full_like(item, T - 1)).clamp_(min=0)
  unsel_tok = torch.zeros_like(valid)
  for u in unselectable_ids:
    unsel_tok |= token_ids == int(u)
  unsel_tok &= valid
  item_unsel = torch.zeros(B, T, dtype=torch.int32, device=dev).scatter_reduce_(
      1, item, unsel_tok.to(torch.int32), reduce='amax', include_self=True).bool()
  item_exists = torch.zeros(B, T, dtype=torch.int32, device=dev).scatter_reduce_(
      1, item, valid.to(torch.int32), reduce='amax', include_self=True).bool()
  selectable = item_exists & ~item_unsel
  n_selectable = selectable.sum(1)
  n_sel = torch.minimum(torch.ceil(n_selectable.to(torch.float32) * torch.tensor(selection_rate, dtype=torch.float32, device=dev)),
                        torch.tensor(float(max_selections), device=dev)).to(torch.int64)
  keys = torch.where(selectable, item_keys.to(torch.float32), torch.full_like(item_keys, float('inf'), dtype=torch.float32))
  rank = torch.argsort(torch.argsort(keys, dim=1, stable=True), dim=1, stable=True)
  item_chosen = selectable & (rank < n_sel[:, None])
  tok_chosen = torch.gather(item_chosen, 1, item) & valid
  u = torch.gather(value_u.to(torch.float32), 1, item)
  to_mask = u < mask_token_rate
  to_rand = ~to_mask & (u < mask_token_rate + random_token_rate)
  new_tok = torch.where(to_mask, torch.full_like(token_ids, mask_token_id), torch.where(to_rand, random_ids.to(token_ids.dtype), token_ids))
  masked = torch.where(tok_chosen, new_tok, token_ids)
  order = torch.argsort((~tok_chosen).to(torch.int8), dim=1, stable=True)      # chosen positions first, ascending
  n_masked = tok_chosen.sum(1)
  live = pos < n_masked[:, None]
  positions = torch.where(live, order, torch.zeros_like(order)).to(torch.int32)
  labels = torch.where(live, torch.gather(token_ids, 1, order), torch.zeros_like(token_ids))
  return masked, positions, n_masked, labels


_INT32_MIN, _INT32_MAX = -(1 << 31), (1 << 31) - 1


def _item_masking_kernel_serves(token_ids, n_tokens, unselectable_ids, mask_token_id, item_keys, value_u, random_ids, word_start) -> bool:
  """What `kernel=None` sends to `mmt_item_masking`: int32 ids inside the library's limits and every other input in the
  plain form -- [B] lengths, [B,T] draws, a bool [B,T] `word_start` or none.  Anything the torch ops would broadcast or
  convert (other shapes, an integer `word_start`, an id that is no int32 value) stays with the torch ops."""
  from . import _lib
  if not (token_ids.dim() == 2 and token_ids.dtype == torch.int32 and 1 <= token_ids.shape[1] <= _lib.MMT_MASK_MAX_TOKENS and
          1 <= token_ids.shape[0] and token_ids.numel() < (1 << 31) and len(unselectable_ids) <= _lib.MMT_MASK_MAX_UNSELECTABLE):
    return False
  shape = token_ids.shape
  if n_tokens.shape != shape[:1] or n_tokens.is_floating_point() or not _INT32_MIN <= int(mask_token_id) <= _INT32_MAX:
    return False
  if any(t.shape != shape for t in (item_keys, value_u, random_ids)):
    return False
  return word_start is None or (word_start.dtype == torch.bool and word_start.shape == shape)


def _random_item_masking_kernel(token_ids, n_tokens, selection_rate, max_selections, unselectable_ids, mask_token_id, item_keys,
                                value_u, random_ids, word_start, mask_token_rate, random_token_rate):
  """`mmt_item_masking` (GPU tensors, the current stream, fresh outputs, no host wait) or `mmt_item_masking_host`."""
  from . import _lib
  if token_ids.dim() != 2 or token_ids.dtype != torch.int32:
    raise ValueError('random_item_masking(kernel=True) expects token_ids int32 [B,T]')
  if not _INT32_MIN <= int(mask_token_id) <= _INT32_MAX:
    raise ValueError(f'mask_token_id {mask_token_id} is no int32 value')
  dev = token_ids.device
  B, T = token_ids.shape
  same = lambda t, dtype: t.to(device=dev, dtype=dtype).contiguous()
  token_ids = token_ids.contiguous()
  if n_tokens.dtype not in (torch.int32, torch.int64):
    n_tokens = n_tokens.to(torch.int64)
  n_tokens = same(n_tokens, n_tokens.dtype)
  if n_tokens.shape != (B,):
    raise ValueError('random_item_masking expects n_tokens [B]')
  item_keys, value_u, random_ids = same(item_keys, torch.float32), same(value_u, torch.float32), same(random_ids, torch.int32)
  if word_start is not None:
    word_start = same(word_start, torch.bool).view(torch.uint8)
  for t in (item_keys, value_u, random_ids, word_start):
    if t is not None and t.shape != (B, T):
      raise ValueError('random_item_masking expects item_keys, value_u, random_ids and word_start [B,T]')
  d = _lib.ItemMaskingDesc()
  d.B, d.T = B, T
  d.max_selections = min(max(int(max_selections), _INT32_MIN), _INT32_MAX)
  d.mask_token_id = int(mask_token_id)
  ids = [u for u in unselectable_ids if _INT32_MIN <= u <= _INT32_MAX]          # (no int32 token equals any other)
  d.n_unselectable = len(ids)
  for k, u in enumerate(ids[:_lib.MMT_MASK_MAX_UNSELECTABLE]):
    d.unselectable[k] = u
  d.n_tokens_i64 = int(n_tokens.dtype == torch.int64)
  # torch compares a float32 tensor with a Python number in float32: each threshold is the Python value rounded once
  d.selection_rate, d.mask_threshold = float(selection_rate), float(mask_token_rate)
  d.random_threshold = float(mask_token_rate + random_token_rate)
  masked, positions, labels = (torch.empty((B, T), dtype=torch.int32, device=dev) for _ in range(3))
  n_masked = torch.empty((B,), dtype=torch.int64, device=dev)
  args = (d, token_ids.data_ptr(), n_tokens.data_ptr(), None if word_start is None else word_start.data_ptr(), item_keys.data_ptr(),
          value_u.data_ptr(), random_ids.data_ptr(), masked.data_ptr(), positions.data_ptr(), n_masked.data_ptr(), labels.data_ptr())
  if dev.type == 'cuda':
    with torch.cuda.device(dev):
      _lib.check(_lib.lib().mmt_item_masking(*args, torch.cuda.current_stream(dev).cuda_stream))
  else:
    _lib.check(_lib.lib().mmt_item_masking_host(*args))
  return masked, positions, n_masked, labels


def _pad_or_fail(x: torch.Tensor, n_live: torch.Tensor, width: int, what: str) -> torch.Tensor:
  """tensor_utils.pad_to_max_seq_len on the compacted [B,T] rows: tf.pad cannot shorten, so more live entries
  than `width` is an error in the reference as well."""
  if x.shape[1] >= width:
    if int(n_live.max()) > width:
      raise ValueError(f'{what}: more masked positions than max selections ({int(n_live.max())} > {width})')
    return x[:, :width]
  return torch.nn.functional.pad(x, (0, width - x.shape[1]))


def make_mlm_and_mpp_features(features: Dict[str, torch.Tensor], randoms: Dict[str, torch.Tensor], *,
                              max_seq_len: int, num_patches: int, patch_size: int, vocab_size: int,
                              mask_token_id: int, unselectable_ids, mlm_fraction_to_mask: float = 0.15,
                              mpp_fraction_to_mask: float = 0.5, mlm_max_selections_per_seq: int = 256,
                              mpp_max_selections_per_seq: int = 98, patch_mask_token_id: int = None,
                              channels: int = 3, output_channel_bits: int = 3, max_pixel_val: int = 256,
                              masking_kernel: bool = None):
  """`make_mlm_and_mpp_features` (data_utils.py:507-637) + `make_word_ids_features` (:728-741), batched.

  features: patch_token_ids [B, 2+P] ([CLS] [PATCH] patch tokens), text_token_ids [B,T] + num_text_wordpieces
  [B] (+ optional text_word_start [B,T] for whole-word masking), patch_embeddings [B,P,E],
  unnormalized_patch_embeddings [B,P,E].  randoms: {mlm,mpp}_{item_keys,value_u,random_ids}.
  Returns the new features: word_ids [B,S], patch_token_ids, text_token_ids [B, S-2-P], patch_embeddings (rows
  of [MASK]ed patches zeroed), mlm_/mpp_ positions, label_ids, label_weights.  masking_kernel: the `kernel` switch of
  the two `random_item_masking` calls (None: one launch each for GPU tensors)."""
  out = dict(features)
  B = features['patch_token_ids'].shape[0]
  dev = features['patch_token_ids'].device
  pm = mask_token_id if patch_mask_token_id is None else patch_mask_token_id
  mlm_max = min(mlm_max_selections_per_seq, max_seq_len)
  # ---- patches (:521-588)
  ptok = features['patch_token_ids']
  n_ptok = torch.full((B,), ptok.shape[1], device=dev, dtype=torch.int64)
  mpp_tok, mpp_pos, n_mpp, _ = random_item_masking(
      ptok, n_ptok, selection_rate=mpp_fraction_to_mask, max_selections=mpp_max_selections_per_seq,
      unselectable_ids=unselectable_ids, mask_token_id=pm, item_keys=randoms['mpp_item_keys'],
      value_u=randoms['mpp_value_u'], random_ids=randoms['mpp_random_ids'], kernel=masking_kernel)
  mpp_pos = _pad_or_fail(mpp_pos, n_mpp, mpp_max_selections_per_seq, 'mpp')
  live = torch.arange(mpp_max_selections_per_seq, device=dev)[None] < n_mpp[:, None]
  shifted = (mpp_pos.to(torch.int64) - 2).clamp_(min=0)                                  # -2: [CLS] and [PATCH]
  unnorm = features['unnormalized_patch_embeddings']
  emb = torch.gather(unnorm, 1, shifted[..., None].expand(-1, -1, unnorm.shape[-1]))
  lab = make_mpp_label_ids(emb, patch_size, channels, output_channel_bits, max_pixel_val)
  out['mpp_label_ids'] = torch.where(live, lab, torch.zeros_like(lab))
  num_real = (mpp_tok == pm).sum(1)                                                       # get_masked_weights (:483-505)
  idx = torch.arange(mpp_max_selections_per_seq, device=dev)[None]
  out['mpp_label_weights'] = ((idx < num_real[:, None]) & live).to(torch.float32)
  out['mpp_positions'] = mpp_pos
  keep = (mpp_tok[:, 2:2 + num_patches] != pm).to(features['patch_embeddings'].dtype)   # zero the masked patches (:577-585)
  out['patch_embeddings'] = features['patch_embeddings'] * keep[..., None]
  out['patch_token_ids'] = mpp_tok
  # ---- text (:590-636)
  ttok = features['text_token_ids']
  mlm_tok, mlm_pos, n_mlm, mlm_lab = random_item_masking(
      ttok, features['num_text_wordpieces'].to(torch.int64), selection_rate=mlm_fraction_to_mask,
      max_selections=mlm_max, unselectable_ids=unselectable_ids, mask_token_id=mask_token_id,
      item_keys=randoms['mlm_item_keys'], value_u=randoms['mlm_value_u'], random_ids=randoms['mlm_random_ids'],
      word_start=features.get('text_word_start'), kernel=masking_kernel)
  tlive = torch.arange(ttok.shape[1], device=dev)[None] < n_mlm[:, None]
  mlm_pos = torch.where(tlive, mlm_pos + (2 + num_patches), torch.zeros_like(mlm_pos))     # offset before the padding
  out['mlm_positions'] = _pad_or_fail(mlm_pos, n_mlm, mlm_max, 'mlm')
  out['mlm_label_ids'] = _pad_or_fail(mlm_lab, n_mlm, mlm_max, 'mlm')
  valid_t = torch.arange(ttok.shape[1], device=dev)[None] < features['num_text_wordpieces'][:, None]
  num_real_t = ((mlm_tok == mask_token_id) & valid_t).sum(1)
  out['mlm_label_weights'] = (torch.arange(mlm_max, device=dev)[None] < num_real_t[:, None]).to(torch.float32)
  max_remaining = max_seq_len - num_patches - 2
  text = torch.where(valid_t, mlm_tok, torch.zeros_like(mlm_tok))
  text = text[:, :max_remaining] if text.shape[1] >= max_remaining else torch.nn.functional.pad(text, (0, max_remaining - text.shape[1]))
  out['text_token_ids'] = text
  out['word_ids'] = torch.cat([mpp_tok, text], dim=1)                                        # make_word_ids_features
  return out
