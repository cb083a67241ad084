"""Shards for the fine-tuning and retrieval loaders (tests/test_finetune_records_host.py, tests/test_gpu_finetune_records.py,
tests/test_gpu_retrieval_records.py), written at test time with the writer of tests/_record_cases.py from the committed
JPEG and PNG fixtures and the text corpus.  No code of mmt_amd is used here."""
import functools
import os

from tests import _jpeg_cases as JC
from tests import _png_cases as PC
from tests import _record_cases as R
from tests import _text_cases as TC

IMAGE, PATCH, SEQ, BATCH = 32, 16, 32, 8          # the smallest shapes of tests/test_gpu_records.py
N_PATCH = (IMAGE // PATCH) ** 2
N_IMG = 2 + N_PATCH

PNG_NAME = '9x17_rgb8_fcycle_i1_fixed'      # a committed PNG fixture: interlaced RGB, every filter type


def image_bytes(name) -> bytes:
  return PC.data(name[4:]) if name.startswith('png:') else JC.data(name)


def image_pixels(name):
  """The committed decode of a fixture, uint8 [h, w, 3]."""
  return PC.expected(name[4:]) if name.startswith('png:') else JC.expected(name)


def write_file(path, payloads) -> str:
  with open(str(path), 'wb') as f:
    for p in payloads:
      f.write(R.frame(p))
  return str(path)


def _texts(rec):
  feats = [('caption', 'bytes', [rec['caption'].encode('utf-8')])]
  if rec['alt_text'] != '':                                      # a missing text field is '' (FixedLenFeature default)
    feats.append(('alt_text', 'bytes', [rec['alt_text'].encode('utf-8')]))
  return feats


def image_payload(image, image_index, alias=False) -> bytes:
  """An image record of a separate set; with alias the id is stored under `index`."""
  return R.example([('image_data', 'bytes', [image_bytes(image)]), ('index' if alias else 'image_index', 'int64', [image_index]),
                    ('other', 'float', [1.5])])


def text_payload(rec) -> bytes:
  """A text record of a separate set: rec has text_index, gt_image_index, caption, alt_text."""
  return R.example([('gt_image_index', 'int64', [rec['gt_image_index']])] + _texts(rec) + [('text_index', 'int64', [rec['text_index']])])


def pair_payload(image, image_index, rec) -> bytes:
  return R.example([('text_index', 'int64', [rec['text_index']]), ('image_data', 'bytes', [image_bytes(image)])] + _texts(rec) +
                   [('image_index', 'int64', [image_index]), ('gt_image_index', 'int64', [rec['gt_image_index']])])


# ---- the retrieval fixture: 5 images (one PNG) and 7 texts, ids unsorted and not contiguous ----------------------------
IMAGE_IDS = (40, 7, 1000003, 12, 0)
TEXT_IDS = (900, 15, 16, 3, 77777, 42, 8)
GT_OF_TEXT = (7, 40, 0, 12, 7, 1000003, 5)        # the last text's image is in no set


@functools.lru_cache(maxsize=None)
def retrieval_images():
  names = R.image_names()
  return (names[8], names[11], 'png:' + PNG_NAME, names[5], names[10])


@functools.lru_cache(maxsize=None)
def retrieval_texts():
  recs = R.loader_records(7)
  return tuple({'text_index': TEXT_IDS[i], 'gt_image_index': GT_OF_TEXT[i], 'caption': r['caption'], 'alt_text': r['alt_text']}
               for i, r in enumerate(recs))


def write_separate_sets(directory):
  """image-*.tfrecord (2 files: 3 + 2 records, the second file's ids under `index`) and text.tfrecord.  Returns
  (image pattern, text pattern, image ids in read order, text records in read order)."""
  d = str(directory)
  ims, ids = retrieval_images(), IMAGE_IDS
  write_file(os.path.join(d, 'image-0.tfrecord'), [image_payload(ims[i], ids[i]) for i in (0, 1, 2)])
  write_file(os.path.join(d, 'image-1.tfrecord'), [image_payload(ims[i], ids[i], alias=True) for i in (3, 4)])
  write_file(os.path.join(d, 'text.tfrecord'), [text_payload(r) for r in retrieval_texts()])
  order = (0, 3, 1, 4, 2)                                        # two files interleaved record by record
  return (os.path.join(d, 'image-*.tfrecord'), os.path.join(d, 'text.tfrecord'), [(ims[i], ids[i]) for i in order],
          list(retrieval_texts()))


def pair_list():
  """21 listed pairs: each of the 7 texts with 3 of the 5 images, as (image place, text place)."""
  return [((t + k * 2) % 5, t) for t in range(7) for k in range(3)]


def write_pair_records(directory):
  """One file of 21 records.  Returns (pattern, the (image place, text place) list in record order)."""
  listed = pair_list()
  ims, texts = retrieval_images(), retrieval_texts()
  path = write_file(os.path.join(str(directory), 'pairs.tfrecord'),
                    [pair_payload(ims[i], IMAGE_IDS[i], texts[t]) for i, t in listed])
  return path, listed


def vocab_size():
  return len(TC.vocab_tokens()) + 1
