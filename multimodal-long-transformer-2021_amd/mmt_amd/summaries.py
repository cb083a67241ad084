"""TensorBoard event files without TensorFlow: `EventFileWriter` writes scalar summaries, `read_scalars` reads them
back.  DESIGN.md section 4, "Trainer loop, summaries, recovery".

A file is a sequence of TFRecord frames, exactly the frames `include/mmt_layer.h` describes for the record reader:
  uint64 length (little endian) | uint32 masked_crc32c(the 8 length bytes) | payload | uint32 masked_crc32c(payload)
and every payload is one `Event` message in protobuf wire format, written and read here by hand:
  Event          wall_time = 1 (double), step = 2 (int64 varint), file_version = 3 (string), summary = 5 (message)
  Summary        value = 1 (repeated message)
  Summary.Value  tag = 1 (string), simple_value = 2 (float32)
The first frame of a file carries `file_version = "brain.Event:2"`.  Events are about a hundred bytes and a run writes
one per `trainer.summary_interval` steps, so the CRC-32C is a 256-entry table in Python."""
from __future__ import annotations

import os
import socket
import struct
import threading
import time
from typing import Dict, Iterator, List, Mapping, Tuple

import numpy as np

FILE_VERSION = 'brain.Event:2'
_PREFIX = 'events.out.tfevents.'

_VARINT, _FIXED64, _BYTES, _FIXED32 = 0, 1, 2, 5                 # protobuf wire types


def _make_table() -> List[int]:
  table = []
  for i in range(256):
    c = i
    for _ in range(8):
      c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    table.append(c)
  return table


_TABLE = _make_table()


def crc32c(data: bytes) -> int:
  """CRC-32C (Castagnoli, reflected 0x82F63B78, init and final xor 0xFFFFFFFF)."""
  c = 0xFFFFFFFF
  table = _TABLE
  for b in data:
    c = table[(c ^ b) & 0xFF] ^ (c >> 8)
  return c ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
  c = crc32c(data)
  return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def frame(payload: bytes) -> bytes:
  """One TFRecord frame round `payload`."""
  head = struct.pack('<Q', len(payload))
  return head + struct.pack('<I', masked_crc32c(head)) + payload + struct.pack('<I', masked_crc32c(payload))


# ---- the wire format, as far as an Event of scalars needs it ---------------------------------------------------------------
def _varint(n: int) -> bytes:
  n &= (1 << 64) - 1                                             # int64: a negative value is its two's complement, ten bytes
  out = bytearray()
  while n > 0x7F:
    out.append((n & 0x7F) | 0x80)
    n >>= 7
  out.append(n)
  return bytes(out)


def _key(field: int, wire_type: int) -> bytes:
  return _varint((field << 3) | wire_type)


def _delimited(field: int, body: bytes) -> bytes:
  return _key(field, _BYTES) + _varint(len(body)) + body


def _float32_bytes(value) -> bytes:
  """`value` rounded to float32 (to nearest even; beyond its range to an infinity; NaN stays NaN), little endian."""
  with np.errstate(over='ignore'):
    return np.asarray(value, dtype=np.float64).astype('<f4').tobytes()


def encode_event(wall_time: float, step: int = 0, file_version: str = None, scalars: Mapping[str, float] = None) -> bytes:
  out = _key(1, _FIXED64) + struct.pack('<d', float(wall_time)) + _key(2, _VARINT) + _varint(int(step))
  if file_version is not None:
    out += _delimited(3, file_version.encode('utf-8'))
  if scalars is not None:
    summary = b''.join(_delimited(1, _delimited(1, str(tag).encode('utf-8')) + _key(2, _FIXED32) + _float32_bytes(value))
                       for tag, value in scalars.items())
    out += _delimited(5, summary)
  return out


def _read_varint(buf: bytes, pos: int) -> Tuple[int, int]:
  value, shift = 0, 0
  while True:
    if pos >= len(buf) or shift > 63:
      raise ValueError('malformed varint')
    b = buf[pos]
    pos += 1
    value |= (b & 0x7F) << shift
    if not b & 0x80:
      return value, pos
    shift += 7


def _fields(buf: bytes) -> Iterator[Tuple[int, int, object]]:
  """(field number, wire type, value) of every field of a message: an int for a varint, the raw bytes otherwise."""
  pos = 0
  while pos < len(buf):
    key, pos = _read_varint(buf, pos)
    field, wire_type = key >> 3, key & 7
    if wire_type == _VARINT:
      value, pos = _read_varint(buf, pos)
    elif wire_type in (_FIXED64, _FIXED32):
      n = 8 if wire_type == _FIXED64 else 4
      value, pos = buf[pos:pos + n], pos + n
    elif wire_type == _BYTES:
      n, pos = _read_varint(buf, pos)
      value, pos = buf[pos:pos + n], pos + n
    else:
      raise ValueError(f'wire type {wire_type} (field {field}) is not read here')
    if pos > len(buf):
      raise ValueError(f'field {field} runs past the end of its message')
    yield field, wire_type, value


def decode_event(payload: bytes) -> Dict:
  """{'wall_time', 'step', 'file_version' (None when absent), 'scalars': [(tag, value), ...]}; unknown fields, and
  summary values that are no `simple_value`, are skipped."""
  event = {'wall_time': 0.0, 'step': 0, 'file_version': None, 'scalars': []}
  for field, wire_type, value in _fields(payload):
    if field == 1 and wire_type == _FIXED64:
      event['wall_time'] = struct.unpack('<d', value)[0]
    elif field == 2 and wire_type == _VARINT:
      event['step'] = value - (1 << 64) if value >> 63 else value
    elif field == 3 and wire_type == _BYTES:
      event['file_version'] = value.decode('utf-8')
    elif field == 5 and wire_type == _BYTES:
      for f, w, item in _fields(value):
        if f != 1 or w != _BYTES:
          continue
        tag, number = '', None
        for vf, vw, v in _fields(item):
          if vf == 1 and vw == _BYTES:
            tag = v.decode('utf-8')
          elif vf == 2 and vw == _FIXED32:
            number = float(np.frombuffer(v, dtype='<f4')[0])
        if number is not None:
          event['scalars'].append((tag, number))
  return event


# ---- files ----------------------------------------------------------------------------------------------------------------
_writers = 0
_writers_lock = threading.Lock()


class EventFileWriter:
  """One event file `events.out.tfevents.<10-digit seconds>.<hostname>.<pid>.<n>` in `logdir` (created); `<n>` counts the
  writers of this process, so two writers started in the same second never share a name."""

  def __init__(self, logdir: str):
    global _writers
    os.makedirs(logdir, exist_ok=True)
    with _writers_lock:
      n, _writers = _writers, _writers + 1
    now = time.time()
    self.path = os.path.join(logdir, f'{_PREFIX}{int(now):010d}.{socket.gethostname()}.{os.getpid()}.{n}')
    self._file = open(self.path, 'wb')
    self._file.write(frame(encode_event(now, 0, file_version=FILE_VERSION)))

  def scalars(self, step: int, values: Mapping[str, float]) -> None:
    """ONE event at `step` with one value per tag, in the mapping's order, each rounded to float32; NaN and infinities
    are written as they are."""
    if self._file is None:
      raise ValueError(f'write to a closed EventFileWriter ({self.path})')
    self._file.write(frame(encode_event(time.time(), step, scalars=values)))

  def flush(self) -> None:
    if self._file is not None:
      self._file.flush()

  def close(self) -> None:
    if self._file is not None:
      self._file.close()
      self._file = None


def _name_order(name: str):
  """Name order, with the writer count behind the last dot taken as a number (`.10` behind `.9`)."""
  stem, _, n = name.rpartition('.')
  return (stem, int(n)) if n.isdigit() else (name, -1)


def event_files(logdir: str) -> List[str]:
  return [os.path.join(logdir, f) for f in sorted((f for f in os.listdir(logdir) if f.startswith(_PREFIX)), key=_name_order)]


def read_events(path: str) -> Iterator[Dict]:
  """Every event of one file.  Both checksums of every frame are verified (ValueError naming file and byte offset); a
  file that ends inside a frame -- its writer is still running, or was killed -- ends the walk without an error."""
  with open(path, 'rb') as f:
    data = f.read()
  pos = 0
  while pos + 12 <= len(data):
    head = data[pos:pos + 8]
    if struct.unpack_from('<I', data, pos + 8)[0] != masked_crc32c(head):
      raise ValueError(f'{path}: bad length checksum in the frame at byte {pos}')
    n = struct.unpack('<Q', head)[0]
    if pos + 12 + n + 4 > len(data):
      return
    payload = data[pos + 12:pos + 12 + n]
    if struct.unpack_from('<I', data, pos + 12 + n)[0] != masked_crc32c(payload):
      raise ValueError(f'{path}: bad payload checksum in the frame at byte {pos}')
    yield decode_event(payload)
    pos += 12 + n + 4


def read_scalars(logdir: str) -> Dict[str, List[Tuple[int, float]]]:
  """tag -> [(step, value), ...] over every event file of `logdir`, files in name order, events in file order."""
  out: Dict[str, List[Tuple[int, float]]] = {}
  for path in event_files(logdir):
    for event in read_events(path):
      for tag, value in event['scalars']:
        out.setdefault(tag, []).append((event['step'], value))
  return out
