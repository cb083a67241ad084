"""TFRecord shards for the data layer ("Records"): the chunked shard reader and the assembly of a
group of records into one blob that is uploaded once.

  read_shard        a file -> (payload bytes, stored masked CRC) per record; frames are walked by mmt_records_scan on a
                    reused (pinned, when there is a GPU) buffer, the partial tail is carried into the next chunk
  pack_records      payloads -> one (pinned) blob, the mmt_record array over it and every named feature's place in it
                    (mmt_example_fields per payload)
  example_fields    one payload -> its named features where it lies, for reading ids before anything is copied or uploaded
  payload_checksums the blob on its device -> bad flags, one mmt_records_crc call (mmt_records_crc_host for CPU tensors)

Compressed shards (TFRecordOptions GZIP / ZLIB) are refused."""
from __future__ import annotations

import ctypes
from typing import Iterator, List, Sequence, Tuple

import numpy as np
import torch

SCAN_CAPACITY = 4096          # records one mmt_records_scan call returns at the most


def _buffer(n: int) -> torch.Tensor:
  return torch.empty(n, dtype=torch.uint8, pin_memory=torch.cuda.is_available())


def _looks_compressed(head: bytes) -> bool:
  if head[:2] == b'\x1f\x8b':
    return True                                                  # gzip
  return len(head) >= 2 and head[0] & 0x0F == 8 and head[0] >> 4 <= 7 and ((head[0] << 8) | head[1]) % 31 == 0   # zlib


def read_shard(path: str, chunk_bytes: int = 1 << 22) -> Iterator[Tuple[bytes, int]]:
  """Yields (payload, stored masked CRC-32C of the payload) for every record of the file, in order.  The length
  checksums are verified here (ValueError naming file and byte offset); the payload checksum is the caller's to verify
  (`payload_checksums`).  A file that ends inside a frame is a truncated shard: ValueError."""
  from . import _lib
  L = _lib.lib()
  buf = _buffer(max(int(chunk_bytes), 16))
  view = buf.numpy()
  recs = (_lib.Record * SCAN_CAPACITY)()
  n, used = ctypes.c_int64(), ctypes.c_int64()
  have, base = 0, 0                                              # valid bytes in the buffer; file offset of its first byte
  with open(path, 'rb') as f:
    while True:
      got = f.readinto(memoryview(view)[have:])
      have += got
      pos = 0
      while True:
        rc = L.mmt_records_scan(view.ctypes.data + pos, have - pos, ctypes.addressof(recs), SCAN_CAPACITY, ctypes.byref(n), ctypes.byref(used))
        if rc != 0:
          msg = L.mmt_last_error().decode()
          if base + pos == 0 and _looks_compressed(bytes(view[:2])):
            raise ValueError(f'{path}: a compressed shard (gzip / zlib magic at byte 0); TFRecordOptions compression is not supported')
          raise ValueError(f'{path}: {msg} (the chunk starts at byte {base + pos} of the file)')
        for i in range(n.value):
          o = pos + recs[i].offset
          yield view[o:o + recs[i].length].tobytes(), int(recs[i].crc)
        pos += used.value
        if n.value < SCAN_CAPACITY:
          break
      if pos < have and pos > 0:
        view[:have - pos] = view[pos:have].copy()
      have -= pos
      base += pos
      if got == 0:
        if have:
          raise ValueError(f'{path}: truncated shard: {have} bytes behind the last whole record at byte {base}')
        return
      if have == view.size:                                      # a record larger than the buffer: grow
        bigger = _buffer(2 * view.size)
        bigger.numpy()[:have] = view[:have]
        buf, view = bigger, bigger.numpy()


def pack_records(payloads: Sequence[bytes], stored: Sequence[int], names: Sequence[str]):
  """Copies the payloads back to back into one blob (pinned when there is a GPU; padded to 16 bytes) and looks the named
  features up in each.  Returns (blob uint8 tensor, the mmt_record ctypes array over the blob, fields): fields[i][j] is
  the `ExampleField` of names[j] in record i with `offset` rebased into the blob.  A payload that is no well-formed
  Example raises ValueError naming its position in `payloads`."""
  from . import _lib
  L = _lib.lib()
  n = len(payloads)
  total = sum(len(p) for p in payloads)
  blob = _buffer(max((total + 15) & ~15, 16))
  view = blob.numpy()
  view[total:] = 0
  recs = (_lib.Record * max(n, 1))()
  c_names = (ctypes.c_char_p * len(names))(*[s.encode() for s in names])
  fields: List = []
  at = 0
  for i, p in enumerate(payloads):
    view[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
    recs[i].offset, recs[i].length, recs[i].crc = at, len(p), int(stored[i])
    out = (_lib.ExampleField * len(names))()
    if L.mmt_example_fields(view.ctypes.data + at, len(p), len(names), c_names, out) != 0:
      raise ValueError(f'record {i} is no tf.train.Example: {L.mmt_last_error().decode()}')
    for f in out:
      f.offset += at
    fields.append(out)
    at += len(p)
  return blob, recs, fields


def example_fields(payload: bytes, names: Sequence[str]):
  """The named features of one payload, looked up where it lies (no copy, nothing uploaded): the `ExampleField` array of
  `names`, offsets relative to the payload.  For reading a record's ids before deciding whether it is decoded at all.
  A payload that is no well-formed Example raises ValueError."""
  from . import _lib
  L = _lib.lib()
  view = np.frombuffer(payload, dtype=np.uint8) if len(payload) else np.zeros(1, dtype=np.uint8)
  c_names = (ctypes.c_char_p * len(names))(*[s.encode() for s in names])
  out = (_lib.ExampleField * len(names))()
  if L.mmt_example_fields(view.ctypes.data, len(payload), len(names), c_names, out) != 0:
    raise ValueError(f'no tf.train.Example: {L.mmt_last_error().decode()}')
  return out


def payload_checksums(blob_d: torch.Tensor, recs, n: int) -> torch.Tensor:
  """int32 [n] on the blob's device: 1 where the payload's CRC-32C does not give the stored checksum.  One
  mmt_records_crc call on the current stream for a GPU tensor; nothing is read back here."""
  from . import _lib
  L = _lib.lib()
  dev = blob_d.device
  meta = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)
  need = L.mmt_records_crc_workspace_bytes(n)
  if dev.type == 'cuda':
    with torch.cuda.device(dev):
      meta_d = meta.pin_memory().to(dev, non_blocking=True)
      crc = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
      bad = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
      work = torch.empty(need, dtype=torch.uint8, device=dev)
      _lib.check(L.mmt_records_crc(blob_d.data_ptr(), blob_d.numel(), n, meta_d.data_ptr(), crc.data_ptr(), bad.data_ptr(),
                                   work.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream))
  else:
    crc = torch.empty(max(n, 1), dtype=torch.int32)
    bad = torch.empty(max(n, 1), dtype=torch.int32)
    work = torch.empty(need + 16, dtype=torch.uint8)
    ws = (work.data_ptr() + 15) & ~15
    _lib.check(L.mmt_records_crc_host(blob_d.data_ptr(), blob_d.numel(), n, meta.data_ptr(), crc.data_ptr(), bad.data_ptr(), ws, need))
  return bad[:n]
