"""ctypes binding of the C ABI declared in include/mmt_attn.h.

The shared library is built in-tree (csrc/Makefile -> mmt_amd/libmmt_attn.so).  There is
no CPU fallback: if the library is missing, loading fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), 'csrc')
LIB_PATH = os.path.join(_HERE, 'libmmt_attn.so')

MMT_ABI_VERSION = 4
MMT_F32, MMT_BF16 = 0, 1
MMT_IDS_NONE, MMT_IDS_1D, MMT_IDS_2D = 0, 1, 2
MMT_IDS_2D_IMAGE = 3          # MMT_IDS_2D with the image at [g, g + P*P), g = the first-image-position field of image_grid
MMT_FLAG_SCALE_BEFORE_ADD = 1
MMT_FLAG_ACCUM_REL_GRADS = 2
MMT_FLAG_EXAMPLE_IDS = 4      # mask.valid_len names int32 [B,S] example ids (packed rows) instead of [B] lengths
MMT_FLAG_EXAMPLE_STARTS = 8   # with EXAMPLE_IDS: mask.valid_len names int32 [B,2,S], ids and each position's example start
MMT_FLAG_EXAMPLE_GLOBALS = 16  # with EXAMPLE_IDS | EXAMPLE_STARTS: the global range is read at local positions (per-example global tokens)


def image_grid(radius: int, start: int) -> int:
  """`MMT_IMAGE_GRID(a, g)` of include/mmt_attn.h: the `mmt_mask_desc.image_grid` word (0 = no grid term)."""
  return (int(radius) & 0xFF) | ((int(start) & 0x7FFFFF) << 8)

# mmt_attn_desc.tuning (include/mmt_attn.h): kernel-selection switches; 0 = the library's defaults
MMT_TUNE_FWD_WALK = 0x01
MMT_TUNE_FWD_PWIN = 0x100
MMT_TUNE_FWD_ROWS_ONE_WG = 0x200
MMT_TUNE_FWD_NO_WIN = 0x02
MMT_TUNE_FWD_FORCE_WIN = 0x04
MMT_TUNE_BWD_NO_HANDOVER = 0x08
MMT_TUNE_BWD_HO_PER_WAVE = 0x10
MMT_TUNE_BWD_NO_PEEL_DQ = 0x20
MMT_TUNE_BWD_NO_PEEL_DKV = 0x40
MMT_TUNE_BWD_DQ_PLANE_MAJOR = 0x80

EXPORTS = ('mmt_abi_version', 'mmt_last_error', 'mmt_write_step_scalars', 'mmt_workspace_bytes', 'mmt_attn_fwd',
           'mmt_attn_bwd', 'mmt_side_inputs',
           # include/mmt_layer.h
           'mmt_layer_workspace_bytes', 'mmt_ln_fwd', 'mmt_ln_bwd', 'mmt_residual_block_fwd',
           'mmt_residual_block_bwd', 'mmt_bias_gelu_fwd', 'mmt_bias_gelu_bwd', 'mmt_colsum_reduce', 'mmt_colsum_reduce_batch', 'mmt_accumulate_grad', 'mmt_grad_clip_scale', 'mmt_adamw_step', 'mmt_wgrad_accumulate',
           'mmt_wgrad_bias_accumulate', 'mmt_wgrad_grouped', 'mmt_wgrad_group_workspace_bytes', 'mmt_wgrad_workspace_bytes', 'mmt_wgrad_set_cu_budget', 'mmt_embed_fwd', 'mmt_embed_bwd', 'mmt_embed_fwd_packed', 'mmt_embed_bwd_packed', 'mmt_embed_fwd_pairs',
           'mmt_embed_workspace_bytes', 'mmt_xent_fwd', 'mmt_xent_fwd_argmax', 'mmt_xent_bwd', 'mmt_xent_bwd_scaled', 'mmt_weighted_loss', 'mmt_colsum', 'mmt_colsum_workspace_bytes', 'mmt_ln_bwd_add', 'mmt_ffn_gelu_gemm', 'mmt_ffn_dgelu_gemm', 'mmt_ffn_set_cu_budget',
           'mmt_image_patches', 'mmt_rand_augment_workspace_bytes', 'mmt_rand_augment',
           'mmt_wordpiece_vocab_bytes', 'mmt_wordpiece_vocab_build', 'mmt_text_tokens_workspace_bytes', 'mmt_text_tokens',
           'mmt_jpeg_info', 'mmt_jpeg_coefficients', 'mmt_jpeg_workspace_bytes', 'mmt_jpeg_pixels', 'mmt_jpeg_pixels_host',
           'mmt_jpeg_scan_plan', 'mmt_jpeg_entropy_workspace_bytes', 'mmt_jpeg_entropy', 'mmt_jpeg_entropy_host',
           'mmt_records_scan', 'mmt_example_fields', 'mmt_records_crc_workspace_bytes', 'mmt_records_crc', 'mmt_records_crc_host',
           'mmt_png_info', 'mmt_png_inflate', 'mmt_png_workspace_bytes', 'mmt_png_pixels', 'mmt_png_pixels_host',
           'mmt_png_gather', 'mmt_png_scanlines_workspace_bytes', 'mmt_png_scanlines', 'mmt_png_scanlines_host',
           'mmt_lamb_workspace_bytes', 'mmt_lamb_step', 'mmt_lamb_step_host',
           'mmt_pack_rows_workspace_bytes', 'mmt_pack_rows', 'mmt_pack_rows_host',
           'mmt_ema_step', 'mmt_ema_step_host', 'mmt_ema_swap', 'mmt_ema_swap_host',
           'mmt_item_masking', 'mmt_item_masking_host')


class EmbedDesc(ctypes.Structure):
  _fields_ = [('rows', ctypes.c_int64), ('S', ctypes.c_int32), ('H', ctypes.c_int32), ('dtype', ctypes.c_int32),
              ('vocab', ctypes.c_int32), ('seg_vocab', ctypes.c_int32), ('patch_start', ctypes.c_int32),
              ('n_patch', ctypes.c_int32), ('eps', ctypes.c_float), ('dropout_p', ctypes.c_float),
              ('accumulate', ctypes.c_int32), ('dropout_seed', ctypes.c_uint64), ('dropout_epoch', ctypes.c_void_p)]


class RowsDesc(ctypes.Structure):
  _fields_ = [('rows', ctypes.c_int64), ('H', ctypes.c_int32), ('dtype', ctypes.c_int32),
              ('eps', ctypes.c_float), ('dropout_p', ctypes.c_float),
              ('dropout_seed', ctypes.c_uint64), ('accumulate', ctypes.c_int32),
              ('defer_reduce', ctypes.c_int32), ('dropout_epoch', ctypes.c_void_p)]


class MaskDesc(ctypes.Structure):
  _fields_ = [('valid_len', ctypes.c_void_p), ('local_radius', ctypes.c_int32),
              ('global_start', ctypes.c_int32), ('n_global', ctypes.c_int32),
              ('id_mode', ctypes.c_int32), ('max_dist', ctypes.c_int32),
              ('patches_per_row', ctypes.c_int32), ('core_layers', ctypes.c_int32),
              ('image_grid', ctypes.c_int32), ('global_index', ctypes.c_void_p)]


class AttnDesc(ctypes.Structure):
  _fields_ = [('B', ctypes.c_int32), ('S', ctypes.c_int32), ('N', ctypes.c_int32),
              ('D', ctypes.c_int32), ('R', ctypes.c_int32), ('dtype', ctypes.c_int32),
              ('q_stride', ctypes.c_int64 * 3), ('k_stride', ctypes.c_int64 * 3),
              ('v_stride', ctypes.c_int64 * 3), ('o_stride', ctypes.c_int64 * 3),
              ('scale', ctypes.c_float), ('mask_value', ctypes.c_float),
              ('flags', ctypes.c_uint32), ('dropout_p', ctypes.c_float),
              ('dropout_seed', ctypes.c_uint64), ('mask', MaskDesc),
              ('dropout_epoch', ctypes.c_void_p), ('tuning', ctypes.c_uint32), ('sync_words', ctypes.c_uint32),
              ('sync', ctypes.c_void_p)]


class AdamwDesc(ctypes.Structure):
  _fields_ = [('n', ctypes.c_int64), ('lr', ctypes.c_float), ('beta1', ctypes.c_float),
              ('beta2', ctypes.c_float), ('eps', ctypes.c_float), ('bias_correction1', ctypes.c_float),
              ('bias_correction2', ctypes.c_float), ('zero_grad', ctypes.c_int32),
              ('reserved', ctypes.c_int32), ('hyper', ctypes.c_void_p)]


class LambDesc(ctypes.Structure):       # mmt_adamw_desc with the slab's parameter-segment count in the reserved word
  _fields_ = [('n', ctypes.c_int64), ('lr', ctypes.c_float), ('beta1', ctypes.c_float),
              ('beta2', ctypes.c_float), ('eps', ctypes.c_float), ('bias_correction1', ctypes.c_float),
              ('bias_correction2', ctypes.c_float), ('zero_grad', ctypes.c_int32),
              ('n_segments', ctypes.c_int32), ('hyper', ctypes.c_void_p)]


class EmaDesc(ctypes.Structure):
  _fields_ = [('n', ctypes.c_int64), ('one_minus_decay', ctypes.c_float), ('reserved', ctypes.c_int32),
              ('one_minus_decay_dev', ctypes.c_void_p)]


MMT_PACK_MAX_EXAMPLES = 4096             # examples (and example slots) of one mmt_pack_rows call: its plan lives in LDS


class PackDesc(ctypes.Structure):
  _fields_ = [('E', ctypes.c_int32), ('S', ctypes.c_int32), ('R', ctypes.c_int32), ('S_row', ctypes.c_int32),
              ('E_max', ctypes.c_int32), ('n_mlm', ctypes.c_int32), ('n_mpp', ctypes.c_int32), ('reserved', ctypes.c_int32)]


MMT_MASK_MAX_TOKENS = 8192               # positions of a row of one mmt_item_masking call: the row lives in LDS
MMT_MASK_MAX_UNSELECTABLE = 8


class ItemMaskingDesc(ctypes.Structure):
  _fields_ = [('B', ctypes.c_int32), ('T', ctypes.c_int32), ('max_selections', ctypes.c_int32), ('mask_token_id', ctypes.c_int32),
              ('n_unselectable', ctypes.c_int32), ('unselectable', ctypes.c_int32 * MMT_MASK_MAX_UNSELECTABLE),
              ('n_tokens_i64', ctypes.c_int32), ('selection_rate', ctypes.c_float), ('mask_threshold', ctypes.c_float),
              ('random_threshold', ctypes.c_float), ('reserved', ctypes.c_int32)]


class ImageDesc(ctypes.Structure):
  _fields_ = [('B', ctypes.c_int32), ('image_size', ctypes.c_int32), ('patch_size', ctypes.c_int32),
              ('out_dtype', ctypes.c_int32), ('channel_bits', ctypes.c_int32), ('mean', ctypes.c_float * 3)]


class JpegImage(ctypes.Structure):
  _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('components', ctypes.c_int32),
              ('h_samp', ctypes.c_int32 * 3), ('v_samp', ctypes.c_int32 * 3), ('blocks_w', ctypes.c_int32 * 3),
              ('blocks_h', ctypes.c_int32 * 3), ('coef_offset', ctypes.c_int64 * 3), ('coef_elems', ctypes.c_int64),
              ('pixel_offset', ctypes.c_int64)]


MMT_JPEG_HUFF_WORDS = 336      # uint32 words of one Huffman table in the device form; 6 tables per image
MMT_JPEG_ST_OK, MMT_JPEG_ST_BAD_CODE, MMT_JPEG_ST_RUN, MMT_JPEG_ST_OVERRUN, MMT_JPEG_ST_BLOCKS = 0, 1, 2, 3, 4
MMT_JPEG_ST_NOT_CONVERGED = 16


class JpegScan(ctypes.Structure):
  _fields_ = [('byte_offset', ctypes.c_int64), ('byte_count', ctypes.c_int64), ('segment_offset', ctypes.c_int64),
              ('subseq_offset', ctypes.c_int64), ('n_segments', ctypes.c_int32), ('n_subseq', ctypes.c_int32),
              ('max_segment_subseq', ctypes.c_int32), ('components', ctypes.c_int32), ('dc_table', ctypes.c_int32 * 3),
              ('ac_table', ctypes.c_int32 * 3), ('restart_interval', ctypes.c_int32), ('mcus', ctypes.c_int32),
              ('subseq_bytes', ctypes.c_int32), ('uniform_tables', ctypes.c_int32)]


class PngStream(ctypes.Structure):
  _fields_ = [('comp_offset', ctypes.c_int64), ('comp_bytes', ctypes.c_int64)]


# status words of mmt_png_scanlines (include/mmt_layer.h, MMT_PNG_ST_*)
PNG_ST_NAMES = ('ok', 'truncated', 'block type', 'stored length', 'code lengths', 'bad code', 'distance', 'too long', 'too short',
                'adler', 'filter byte', 'no progress')


class PngImage(ctypes.Structure):
  _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32), ('bit_depth', ctypes.c_int32), ('color_type', ctypes.c_int32),
              ('interlace', ctypes.c_int32), ('palette_entries', ctypes.c_int32), ('raw_offset', ctypes.c_int64),
              ('raw_bytes', ctypes.c_int64), ('pixel_offset', ctypes.c_int64)]


MMT_FIELD_MISSING, MMT_FIELD_BYTES, MMT_FIELD_INT64, MMT_FIELD_FLOAT = 0, 1, 2, 3
MMT_RECORDS_PIECE = 128                  # bytes a lane of mmt_records_crc takes
MMT_RECORDS_PART = 256 * MMT_RECORDS_PIECE   # bytes of pieces a workgroup takes


class Record(ctypes.Structure):
  _fields_ = [('offset', ctypes.c_int64), ('length', ctypes.c_int64), ('crc', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


class ExampleField(ctypes.Structure):
  _fields_ = [('kind', ctypes.c_int32), ('float_value', ctypes.c_float), ('count', ctypes.c_int64), ('offset', ctypes.c_int64),
              ('length', ctypes.c_int64), ('int_value', ctypes.c_int64)]


class WgradProblem(ctypes.Structure):
  _fields_ = [('dw', ctypes.c_void_p), ('ldw', ctypes.c_int64), ('dbias', ctypes.c_void_p), ('dy', ctypes.c_void_p),
              ('ldy', ctypes.c_int64), ('x', ctypes.c_void_p), ('ldx', ctypes.c_int64), ('M', ctypes.c_int32),
              ('N', ctypes.c_int32)]


class ColsumItem(ctypes.Structure):
  _fields_ = [('workspace', ctypes.c_void_p), ('o0', ctypes.c_void_p), ('o1', ctypes.c_void_p), ('o2', ctypes.c_void_p),
              ('rows', ctypes.c_int64), ('H', ctypes.c_int32), ('kind', ctypes.c_int32), ('accumulate', ctypes.c_int32),
              ('reserved', ctypes.c_int32)]


class MmtError(RuntimeError):
  """Raised when an entry point of libmmt_attn returns a negative code."""

  def __init__(self, code: int, message: str):
    super().__init__(f'libmmt_attn error {code}: {message}')
    self.code = code


def build(force: bool = False) -> str:
  """Compiles the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
  srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(('.hip', '.h'))]
  srcs.append(os.path.join(os.path.dirname(os.path.dirname(_HERE)), 'include', 'mmt_attn.h'))
  stale = (not os.path.exists(LIB_PATH) or
           any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs))
  if force or stale:
    subprocess.check_call(['make', '-s', '-j4', '-C', _CSRC])
  return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise ImportError(
        f'{LIB_PATH} is missing: the HIP extension has not been built '
        '(run `python -c "import __graft_entry__ as g; g.build()"` or `make -C csrc`). '
        'There is no CPU fallback for the hot path.')
  L = ctypes.CDLL(LIB_PATH)
  vp, i32p = ctypes.c_void_p, ctypes.c_void_p
  L.mmt_abi_version.restype = ctypes.c_int
  L.mmt_abi_version.argtypes = []
  L.mmt_last_error.restype = ctypes.c_char_p
  L.mmt_last_error.argtypes = []
  L.mmt_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_workspace_bytes.argtypes = [ctypes.POINTER(AttnDesc)]
  L.mmt_attn_fwd.restype = ctypes.c_int
  L.mmt_attn_fwd.argtypes = [ctypes.POINTER(AttnDesc), vp, vp, vp, vp, vp, i32p, i32p, vp, vp,
                             vp, ctypes.c_size_t, vp]
  L.mmt_attn_bwd.restype = ctypes.c_int
  L.mmt_attn_bwd.argtypes = [ctypes.POINTER(AttnDesc), vp, vp, vp, vp, vp, i32p, i32p, vp, vp, vp,
                             vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
  L.mmt_side_inputs.restype = ctypes.c_int
  L.mmt_side_inputs.argtypes = [ctypes.POINTER(MaskDesc), ctypes.c_int32, ctypes.c_int32, i32p,
                                i32p, ctypes.c_int32, i32p, i32p, i32p, vp]
  rd = ctypes.POINTER(RowsDesc)
  L.mmt_layer_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_layer_workspace_bytes.argtypes = [rd]
  for name, nargs in (('mmt_ln_fwd', 7), ('mmt_ln_bwd', 11), ('mmt_residual_block_fwd', 10),
                      ('mmt_residual_block_bwd', 14), ('mmt_bias_gelu_fwd', 4), ('mmt_bias_gelu_bwd', 8)):
    fn = getattr(L, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [rd] + [vp] * nargs
  L.mmt_ln_bwd.argtypes = [rd] + [vp] * 9 + [ctypes.c_size_t, vp]
  L.mmt_ln_bwd_add.restype = ctypes.c_int
  L.mmt_ln_bwd_add.argtypes = [rd] + [vp] * 10 + [ctypes.c_size_t, vp]
  L.mmt_residual_block_bwd.argtypes = [rd] + [vp] * 12 + [ctypes.c_size_t, vp]
  L.mmt_bias_gelu_bwd.argtypes = [rd] + [vp] * 6 + [ctypes.c_size_t, vp]
  L.mmt_colsum_reduce.restype = ctypes.c_int
  L.mmt_colsum_reduce.argtypes = [rd, ctypes.c_int32, vp, vp, vp, vp, vp]
  L.mmt_colsum_reduce_batch.restype = ctypes.c_int
  L.mmt_colsum_reduce_batch.argtypes = [ctypes.c_int32, ctypes.POINTER(ColsumItem), vp]
  L.mmt_wgrad_accumulate.restype = ctypes.c_int
  L.mmt_wgrad_accumulate.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_int64, vp, ctypes.c_size_t, vp]
  L.mmt_wgrad_bias_accumulate.restype = ctypes.c_int
  L.mmt_wgrad_bias_accumulate.argtypes = [vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int64, vp, ctypes.c_size_t, vp]
  wp = ctypes.POINTER(WgradProblem)
  L.mmt_wgrad_group_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_wgrad_group_workspace_bytes.argtypes = [ctypes.c_int32, wp, ctypes.c_int64]
  L.mmt_wgrad_grouped.restype = ctypes.c_int
  L.mmt_wgrad_grouped.argtypes = [ctypes.c_int32, wp, ctypes.c_int64, vp, ctypes.c_size_t, vp]
  ed = ctypes.POINTER(EmbedDesc)
  L.mmt_embed_fwd.restype = ctypes.c_int
  L.mmt_embed_fwd.argtypes = [ed] + [vp] * 13
  L.mmt_embed_bwd.restype = ctypes.c_int
  L.mmt_embed_bwd.argtypes = [ed] + [vp] * 12 + [ctypes.c_size_t, vp]
  L.mmt_embed_fwd_packed.restype = ctypes.c_int
  L.mmt_embed_fwd_packed.argtypes = [ed] + [vp] * 5 + [ctypes.c_int32] + [vp] * 6 + [ctypes.c_int32] + [vp] * 4
  L.mmt_embed_bwd_packed.restype = ctypes.c_int
  L.mmt_embed_bwd_packed.argtypes = [ed] + [vp] * 13 + [ctypes.c_int32, vp, ctypes.c_size_t, vp]
  L.mmt_embed_fwd_pairs.restype = ctypes.c_int
  L.mmt_embed_fwd_pairs.argtypes = [ed] + [vp] * 5 + [ctypes.c_int32] * 2 + [vp] * 10
  L.mmt_embed_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_embed_workspace_bytes.argtypes = [ed]
  L.mmt_xent_fwd_argmax.restype = ctypes.c_int
  L.mmt_xent_fwd_argmax.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int64, vp, vp, vp, vp, vp]
  L.mmt_xent_fwd.restype = ctypes.c_int
  L.mmt_xent_fwd.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int64, vp, vp, vp, vp]
  L.mmt_colsum_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_colsum_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32]
  L.mmt_colsum.restype = ctypes.c_int
  L.mmt_colsum.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int64, vp, ctypes.c_int32, vp,
                           ctypes.c_size_t, vp]
  L.mmt_xent_bwd_scaled.restype = ctypes.c_int
  L.mmt_xent_bwd_scaled.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int64, vp, vp, vp, vp,
                                    vp, ctypes.c_int64, vp]
  L.mmt_weighted_loss.restype = ctypes.c_int
  L.mmt_weighted_loss.argtypes = [ctypes.c_int64, vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp]
  L.mmt_xent_bwd.restype = ctypes.c_int
  L.mmt_xent_bwd.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int64, vp, vp, vp, vp,
                             ctypes.c_int64, vp]
  i64 = ctypes.c_int64
  L.mmt_ffn_gelu_gemm.restype = ctypes.c_int
  L.mmt_ffn_gelu_gemm.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, vp]
  L.mmt_ffn_dgelu_gemm.restype = ctypes.c_int
  L.mmt_ffn_dgelu_gemm.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i64, i64, i64, i64, vp]
  L.mmt_ffn_set_cu_budget.restype = None
  L.mmt_ffn_set_cu_budget.argtypes = [ctypes.c_int32]
  L.mmt_wgrad_set_cu_budget.restype = None
  L.mmt_wgrad_set_cu_budget.argtypes = [ctypes.c_int32]
  L.mmt_wgrad_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_wgrad_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
  L.mmt_adamw_step.restype = ctypes.c_int
  L.mmt_adamw_step.argtypes = [ctypes.POINTER(AdamwDesc)] + [vp] * 8
  L.mmt_lamb_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_lamb_workspace_bytes.argtypes = [ctypes.c_int64]
  L.mmt_lamb_step.restype = ctypes.c_int
  L.mmt_lamb_step.argtypes = [ctypes.POINTER(LambDesc)] + [vp] * 10 + [ctypes.c_size_t, vp]
  L.mmt_lamb_step_host.restype = ctypes.c_int
  L.mmt_lamb_step_host.argtypes = [ctypes.POINTER(LambDesc)] + [vp] * 10 + [ctypes.c_size_t]
  L.mmt_pack_rows_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_pack_rows_workspace_bytes.argtypes = [ctypes.POINTER(PackDesc)]
  L.mmt_pack_rows.restype = ctypes.c_int
  L.mmt_pack_rows.argtypes = [ctypes.POINTER(PackDesc)] + [vp] * 16 + [ctypes.c_size_t, vp]
  L.mmt_pack_rows_host.restype = ctypes.c_int
  L.mmt_pack_rows_host.argtypes = [ctypes.POINTER(PackDesc)] + [vp] * 16 + [ctypes.c_size_t]
  L.mmt_ema_step.restype = ctypes.c_int
  L.mmt_ema_step.argtypes = [ctypes.POINTER(EmaDesc), vp, vp, vp]
  L.mmt_ema_step_host.restype = ctypes.c_int
  L.mmt_ema_step_host.argtypes = [ctypes.POINTER(EmaDesc), vp, vp]
  L.mmt_ema_swap.restype = ctypes.c_int
  L.mmt_ema_swap.argtypes = [ctypes.c_int64, vp, vp, vp, vp]
  L.mmt_ema_swap_host.restype = ctypes.c_int
  L.mmt_ema_swap_host.argtypes = [ctypes.c_int64, vp, vp, vp]
  L.mmt_item_masking.restype = ctypes.c_int
  L.mmt_item_masking.argtypes = [ctypes.POINTER(ItemMaskingDesc)] + [vp] * 11
  L.mmt_item_masking_host.restype = ctypes.c_int
  L.mmt_item_masking_host.argtypes = [ctypes.POINTER(ItemMaskingDesc)] + [vp] * 10
  L.mmt_grad_clip_scale.restype = ctypes.c_int
  L.mmt_grad_clip_scale.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.c_float,
                                    ctypes.c_float, vp, vp, vp, ctypes.c_size_t, vp]
  L.mmt_accumulate_grad.restype = ctypes.c_int
  L.mmt_accumulate_grad.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int64, vp]
  L.mmt_image_patches.restype = ctypes.c_int
  L.mmt_image_patches.argtypes = [ctypes.POINTER(ImageDesc), vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
  L.mmt_rand_augment_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_rand_augment_workspace_bytes.argtypes = [ctypes.c_int32]
  L.mmt_rand_augment.restype = ctypes.c_int
  L.mmt_rand_augment.argtypes = [ctypes.c_int32, vp, i64, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
  L.mmt_wordpiece_vocab_bytes.restype = ctypes.c_size_t
  L.mmt_wordpiece_vocab_bytes.argtypes = [i64, i64]
  L.mmt_wordpiece_vocab_build.restype = ctypes.c_int
  L.mmt_wordpiece_vocab_build.argtypes = [i64, vp, vp, vp, ctypes.c_size_t]
  L.mmt_text_tokens_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_text_tokens_workspace_bytes.argtypes = [ctypes.c_int32] * 3
  L.mmt_text_tokens.restype = ctypes.c_int
  L.mmt_text_tokens.argtypes = ([ctypes.c_int32] * 2 + [vp, i64, vp, vp, vp, ctypes.c_size_t, vp, i64, vp] + [ctypes.c_int32] * 4 +
                                [vp, vp, vp, vp, ctypes.c_size_t, vp])
  jp = ctypes.POINTER(JpegImage)
  L.mmt_jpeg_info.restype = ctypes.c_int
  L.mmt_jpeg_info.argtypes = [vp, i64, jp]
  L.mmt_jpeg_coefficients.restype = ctypes.c_int
  L.mmt_jpeg_coefficients.argtypes = [vp, i64, jp, vp, i64, vp]
  L.mmt_jpeg_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_jpeg_workspace_bytes.argtypes = [i64]
  L.mmt_jpeg_pixels.restype = ctypes.c_int
  L.mmt_jpeg_pixels.argtypes = [ctypes.c_int32, vp, vp, i64, vp, vp, i64, vp, ctypes.c_size_t, vp]
  L.mmt_jpeg_pixels_host.restype = ctypes.c_int
  L.mmt_jpeg_pixels_host.argtypes = [ctypes.c_int32, vp, vp, i64, vp, vp, i64, vp, ctypes.c_size_t]
  L.mmt_jpeg_scan_plan.restype = ctypes.c_int
  L.mmt_jpeg_scan_plan.argtypes = [vp, i64, jp, ctypes.c_int32, ctypes.POINTER(JpegScan), vp, vp, vp, i64, vp, i64]
  L.mmt_jpeg_entropy_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_jpeg_entropy_workspace_bytes.argtypes = [ctypes.c_int32, i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
  entropy_args = ([ctypes.c_int32, vp, i64, vp, vp, vp, vp, i64, vp, i64] + [ctypes.c_int32] * 3 + [vp, i64, vp, vp, ctypes.c_size_t])
  L.mmt_jpeg_entropy.restype = ctypes.c_int
  L.mmt_jpeg_entropy.argtypes = entropy_args + [vp]
  L.mmt_jpeg_entropy_host.restype = ctypes.c_int
  L.mmt_jpeg_entropy_host.argtypes = entropy_args
  L.mmt_records_scan.restype = ctypes.c_int
  L.mmt_records_scan.argtypes = [vp, i64, vp, i64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
  L.mmt_example_fields.restype = ctypes.c_int
  L.mmt_example_fields.argtypes = [vp, i64, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ExampleField)]
  L.mmt_records_crc_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_records_crc_workspace_bytes.argtypes = [i64]
  L.mmt_records_crc.restype = ctypes.c_int
  L.mmt_records_crc.argtypes = [vp, i64, i64, vp, vp, vp, vp, ctypes.c_size_t, vp]
  L.mmt_records_crc_host.restype = ctypes.c_int
  L.mmt_records_crc_host.argtypes = [vp, i64, i64, vp, vp, vp, vp, ctypes.c_size_t]
  pp = ctypes.POINTER(PngImage)
  L.mmt_png_info.restype = ctypes.c_int
  L.mmt_png_info.argtypes = [vp, i64, pp]
  L.mmt_png_inflate.restype = ctypes.c_int
  L.mmt_png_inflate.argtypes = [vp, i64, pp, vp, i64, vp]
  L.mmt_png_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_png_workspace_bytes.argtypes = [i64]
  L.mmt_png_pixels.restype = ctypes.c_int
  L.mmt_png_pixels.argtypes = [ctypes.c_int32, vp, vp, i64, vp, vp, i64, vp, ctypes.c_size_t, vp]
  L.mmt_png_pixels_host.restype = ctypes.c_int
  L.mmt_png_pixels_host.argtypes = [ctypes.c_int32, vp, vp, i64, vp, vp, i64, vp, ctypes.c_size_t]
  L.mmt_png_gather.restype = ctypes.c_int
  L.mmt_png_gather.argtypes = [vp, i64, pp, vp, i64, ctypes.POINTER(PngStream), vp]
  L.mmt_png_scanlines_workspace_bytes.restype = ctypes.c_size_t
  L.mmt_png_scanlines_workspace_bytes.argtypes = [ctypes.c_int32]
  L.mmt_png_scanlines.restype = ctypes.c_int
  L.mmt_png_scanlines.argtypes = [ctypes.c_int32, vp, vp, vp, i64, vp, i64, vp, ctypes.c_int32, vp, ctypes.c_size_t, vp]
  L.mmt_png_scanlines_host.restype = ctypes.c_int
  L.mmt_png_scanlines_host.argtypes = [ctypes.c_int32, vp, vp, vp, i64, vp, i64, vp, ctypes.c_int32, vp, ctypes.c_size_t]
  L.mmt_write_step_scalars.restype = ctypes.c_int
  L.mmt_write_step_scalars.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp]
  if L.mmt_abi_version() != MMT_ABI_VERSION:
    raise ImportError('libmmt_attn ABI version mismatch')
  _lib = L
  return L


def check(rc: int) -> None:
  if rc != 0:
    raise MmtError(rc, lib().mmt_last_error().decode())
