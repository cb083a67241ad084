"""TensorBoard event files without TensorFlow (mmt_amd/summaries.py) and the host-side rules of the trainer's loop mode
(`evaluation.loop_end_due`, `evaluation.check_loop_startup`, `train.Recovery`), on the CPU.

The Python writer is checked by two implementations it shares no code with: the project's C++ record reader
(`records.read_shard` walks the frames, `mmt_records_crc_host` verifies the payload checksums) and the protobuf runtime
(`google.protobuf`, message types built from a descriptor declared here with the field numbers of TensorFlow's
`event.proto` / `summary.proto`)."""
import ctypes
import math
import os
import struct
import types

import numpy as np
import pytest

import __graft_entry__  # noqa: F401  (sets sys.path)

# what the writer is asked to write: NaN, infinities, -0.0, a float32 denormal, a value beyond float32, a long tag
LONG_TAG = 't' * 200
WRITES = [
    (1, {'training_loss': 2.5, 'learning_rate': 1e-4}),
    (2, {'nan': float('nan'), 'inf': float('inf'), 'minus_inf': float('-inf'), 'minus_zero': -0.0, 'denormal': 1e-45,
         'a_third': 1.0 / 3.0, 'too_large': 1e39}),
    (2 ** 40, {LONG_TAG: 7.0, 'mlm_accuracy': 0.123456789}),
    (0, {}),
]


@pytest.fixture(scope='module')
def lib():
  from mmt_amd import _lib
  _lib.build()
  return _lib


@pytest.fixture()
def written(tmp_path):
  from mmt_amd import summaries
  w = summaries.EventFileWriter(str(tmp_path / 'logs'))
  for step, values in WRITES:
    w.scalars(step, values)
  w.flush()
  w.close()
  return w.path


def f32(v):
  with np.errstate(over='ignore'):
    return np.float32(v)


def same_float(a, b):
  """Equal as float32 bit patterns, any NaN equal to any NaN."""
  a, b = f32(a), f32(b)
  return bool(np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


# ---- checksum ---------------------------------------------------------------------------------------------------------------
def test_crc32c_and_its_mask():
  from mmt_amd import summaries
  assert summaries.crc32c(b'123456789') == 0xE3069283
  assert summaries.crc32c(b'') == 0
  for data in (b'123456789', b'', bytes(range(256)) * 3):
    c = summaries.crc32c(data)
    assert summaries.masked_crc32c(data) == ((c >> 15 | c << 17) + 0xa282ead8) % 2 ** 32


# ---- framing, through the project's own reader ---------------------------------------------------------------------------------
def test_the_record_reader_walks_every_frame_and_finds_no_bad_payload(lib, written):
  from mmt_amd import records, summaries
  frames = list(records.read_shard(written, chunk_bytes=64))     # small chunks: frames straddle them
  assert len(frames) == 1 + len(WRITES)
  payloads = [p for p, _ in frames]
  assert b''.join(summaries.frame(p) for p in payloads) == open(written, 'rb').read()
  # the C++ checksum over the payloads laid back to back, against the checksums the Python writer stored
  L = lib.lib()
  n = len(frames)
  blob = np.frombuffer(b''.join(payloads), dtype=np.uint8).copy()
  recs = (lib.Record * n)()
  at = 0
  for i, (p, stored) in enumerate(frames):
    recs[i].offset, recs[i].length, recs[i].crc = at, len(p), stored
    at += len(p)
  crc, bad = np.zeros(n, dtype=np.uint32), np.full(n, -7, dtype=np.int32)
  need = L.mmt_records_crc_workspace_bytes(n)
  ws = np.zeros(need // 8 + 2, dtype=np.int64)
  lib.check(L.mmt_records_crc_host(blob.ctypes.data, blob.size, n, ctypes.addressof(recs), crc.ctypes.data, bad.ctypes.data,
                                   (ws.ctypes.data + 15) & ~15, need))
  assert bad.tolist() == [0] * n
  assert crc.tolist() == [summaries.crc32c(p) for p in payloads]
  # ... and it does see a payload the writer did not checksum
  recs[1].crc ^= 1
  lib.check(L.mmt_records_crc_host(blob.ctypes.data, blob.size, n, ctypes.addressof(recs), crc.ctypes.data, bad.ctypes.data,
                                   (ws.ctypes.data + 15) & ~15, need))
  assert bad.tolist() == [0, 1] + [0] * (n - 2)


# ---- decoding, by the protobuf runtime ------------------------------------------------------------------------------------------
def event_classes():
  pytest.importorskip('google.protobuf')
  from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
  F = descriptor_pb2.FieldDescriptorProto
  fd = descriptor_pb2.FileDescriptorProto(name='mmt_test_event.proto', package='mmt_test', syntax='proto3')

  def message(parent, name, fields):
    m = parent.add()
    m.name = name
    for fname, number, ftype, label, type_name in fields:
      f = m.field.add()
      f.name, f.number, f.type, f.label = fname, number, ftype, label
      if type_name:
        f.type_name = type_name
    return m

  summary = message(fd.message_type, 'Summary', [('value', 1, F.TYPE_MESSAGE, F.LABEL_REPEATED, '.mmt_test.Summary.Value')])
  message(summary.nested_type, 'Value', [('tag', 1, F.TYPE_STRING, F.LABEL_OPTIONAL, ''),
                                         ('simple_value', 2, F.TYPE_FLOAT, F.LABEL_OPTIONAL, '')])
  message(fd.message_type, 'Event', [('wall_time', 1, F.TYPE_DOUBLE, F.LABEL_OPTIONAL, ''),
                                     ('step', 2, F.TYPE_INT64, F.LABEL_OPTIONAL, ''),
                                     ('file_version', 3, F.TYPE_STRING, F.LABEL_OPTIONAL, ''),
                                     ('summary', 5, F.TYPE_MESSAGE, F.LABEL_OPTIONAL, '.mmt_test.Summary')])
  pool = descriptor_pool.DescriptorPool()
  pool.Add(fd)
  return message_factory.GetMessageClass(pool.FindMessageTypeByName('mmt_test.Event'))


def test_the_protobuf_runtime_parses_every_event(lib, written):
  from mmt_amd import records
  Event = event_classes()
  events = []
  for payload, _ in records.read_shard(written):
    e = Event()
    e.ParseFromString(payload)                                   # raises on anything that is no Event
    events.append(e)
  first = events[0]
  assert first.file_version == 'brain.Event:2' and first.step == 0 and len(first.summary.value) == 0
  born = os.path.getmtime(written)
  assert all(abs(e.wall_time - born) < 600 for e in events)
  assert len(events) == 1 + len(WRITES)
  for e, (step, values) in zip(events[1:], WRITES):
    assert e.step == step and e.file_version == ''
    assert [v.tag for v in e.summary.value] == list(values)       # one Value per tag, in the dict's order
    for v, (tag, want) in zip(e.summary.value, values.items()):
      assert same_float(v.simple_value, want), (tag, v.simple_value, want)
  by_tag = {v.tag: v.simple_value for v in events[2].summary.value}
  assert math.isnan(by_tag['nan']) and by_tag['inf'] == float('inf') and by_tag['minus_inf'] == float('-inf')
  assert by_tag['minus_zero'] == 0.0 and math.copysign(1.0, by_tag['minus_zero']) == -1.0
  assert by_tag['denormal'] == float(np.float32(1e-45)) > 0.0
  assert by_tag['too_large'] == float('inf')                     # rounded to float32
  assert by_tag['a_third'] == float(np.float32(1.0 / 3.0)) != 1.0 / 3.0
  assert events[3].step == 2 ** 40 and events[3].summary.value[0].tag == LONG_TAG


def test_the_reader_skips_what_it_does_not_know_and_reads_negative_steps():
  """An event as TensorFlow would write it -- with a source_metadata message (field 9), a Value with metadata (field 9)
  and a tensor (field 8) beside a simple_value, and one Value that holds an image (field 4) and no simple_value."""
  from mmt_amd import summaries
  Event = event_classes()
  assert summaries.decode_event(Event(wall_time=1.5, step=-3).SerializeToString()) == {
      'wall_time': 1.5, 'step': -3, 'file_version': None, 'scalars': []}
  S = summaries
  value = S._delimited(9, b'\x0a\x03abc') + S._delimited(1, b'loss') + S._delimited(8, b'\x08\x01') + S._key(2, 5) + struct.pack('<f', 0.25)
  image = S._delimited(1, b'picture') + S._delimited(4, b'\x08\x02\x10\x02')
  payload = (S._key(1, 1) + struct.pack('<d', 7.0) + S._delimited(9, b'\x0a\x02tf') + S._key(2, 0) + S._varint(12)
             + S._delimited(5, S._delimited(1, value) + S._delimited(1, image)) + S._key(20, 0) + S._varint(300) + S._key(21, 5) + b'\0' * 4)
  assert summaries.decode_event(payload) == {'wall_time': 7.0, 'step': 12, 'file_version': None, 'scalars': [('loss', 0.25)]}
  e = Event()
  e.ParseFromString(payload)                                     # the hand-made bytes are well formed
  assert e.step == 12 and [v.tag for v in e.summary.value] == ['loss', 'picture']


# ---- read_scalars -------------------------------------------------------------------------------------------------------------
def test_read_scalars_round_trip_over_two_files(tmp_path):
  from mmt_amd import summaries
  d = str(tmp_path / 'train')
  a = summaries.EventFileWriter(d)
  a.scalars(3, {'training_loss': 7.25, 'learning_rate': 1e-4})
  a.scalars(6, {'training_loss': float('nan'), 'learning_rate': 2e-4})
  a.close()
  b = summaries.EventFileWriter(d)
  b.scalars(9, {'training_loss': 1.0 / 3.0, 'extra': -0.0})
  b.scalars(2 ** 40, {'training_loss': float('inf')})
  b.flush()                                                      # read while the second writer is open
  got = summaries.read_scalars(d)
  b.close()
  assert [os.path.basename(p) for p in summaries.event_files(d)] == [os.path.basename(a.path), os.path.basename(b.path)]
  assert list(got) == ['training_loss', 'learning_rate', 'extra']
  steps, values = zip(*got['training_loss'])
  assert steps == (3, 6, 9, 2 ** 40)
  assert values[0] == 7.25 and math.isnan(values[1]) and values[2] == float(np.float32(1.0 / 3.0)) and values[3] == float('inf')
  assert got['learning_rate'] == [(3, float(np.float32(1e-4))), (6, float(np.float32(2e-4)))]
  assert got['extra'] == [(9, 0.0)] and math.copysign(1.0, got['extra'][0][1]) == -1.0
  assert summaries.read_scalars(d).keys() == got.keys()
  # a file that ends inside a frame (its writer was killed) is read up to there; a flipped payload byte is an error
  data = open(b.path, 'rb').read()
  open(b.path, 'wb').write(data[:-5])
  assert [s for s, _ in summaries.read_scalars(d)['training_loss']] == [3, 6, 9]
  broken = bytearray(data)
  broken[-6] ^= 0x40
  open(b.path, 'wb').write(bytes(broken))
  with pytest.raises(ValueError, match='payload checksum'):
    summaries.read_scalars(d)


# ---- writer life cycle --------------------------------------------------------------------------------------------------------
def test_writer_names_and_life_cycle(tmp_path, monkeypatch):
  import re
  import socket
  from mmt_amd import summaries
  monkeypatch.setattr(summaries.time, 'time', lambda: 1700000000.75)      # both writers start in the same second
  d = tmp_path / 'a' / 'b'                                       # created, parents included
  w1, w2 = summaries.EventFileWriter(str(d)), summaries.EventFileWriter(str(d))
  n1, n2 = os.path.basename(w1.path), os.path.basename(w2.path)
  assert n1 != n2 and sorted(os.listdir(d)) == sorted([n1, n2])
  host = re.escape(socket.gethostname())
  for name in (n1, n2):
    assert re.fullmatch(rf'events\.out\.tfevents\.1700000000\.{host}\.{os.getpid()}\.\d+', name), name
  assert int(n2.rsplit('.', 1)[1]) == int(n1.rsplit('.', 1)[1]) + 1
  w1.scalars(1, {'x': 1.0})
  w1.flush()
  w1.close()
  w1.close()                                                     # idempotent
  w1.flush()
  with pytest.raises(ValueError, match='closed'):
    w1.scalars(2, {'x': 2.0})
  w2.close()
  assert summaries.read_scalars(str(d)) == {'x': [(1, 1.0)]}
  # a timestamp below 10 digits is padded
  monkeypatch.setattr(summaries.time, 'time', lambda: 12345.0)
  w3 = summaries.EventFileWriter(str(d))
  w3.close()
  assert os.path.basename(w3.path).startswith('events.out.tfevents.0000012345.')


# ---- the loop's schedule and start-up checks ----------------------------------------------------------------------------------
@pytest.mark.parametrize('per_loop, train_steps, start, want', [
    (3, 7, 0, [3, 6, 7]),
    (1, 2, 0, [1, 2]),
    (100, 5, 0, [5]),
    (3, 7, 4, [6, 7]),                                           # resumed after step 4
    (3, 6, 0, [3, 6]),                                           # the last step is a multiple too: one loop end, not two
])
def test_loop_end_due(per_loop, train_steps, start, want):
  from mmt_amd import evaluation
  assert [s for s in range(start + 1, train_steps + 1) if evaluation.loop_end_due(s, per_loop, train_steps)] == want
  assert not evaluation.loop_end_due(0, per_loop, train_steps)


def test_loop_startup_checks():
  from mmt_amd import configs, evaluation
  cfg = configs.TrainerConfig()
  evaluation.check_loop_startup(cfg)                             # the defaults: 100 and 100
  for per_loop, interval in ((2, 4), (3, 3), (1, 7)):
    evaluation.check_loop_startup(types.SimpleNamespace(steps_per_loop=per_loop, summary_interval=interval))
  with pytest.raises(ValueError) as e:
    evaluation.check_loop_startup(types.SimpleNamespace(steps_per_loop=2, summary_interval=5))
  assert '5' in str(e.value) and '2' in str(e.value) and 'summary_interval' in str(e.value) and 'steps_per_loop' in str(e.value)
  for per_loop, interval in ((0, 100), (100, 0), (-3, 3), (3, -3), (0, 0)):
    with pytest.raises(ValueError) as e:
      evaluation.check_loop_startup(types.SimpleNamespace(steps_per_loop=per_loop, summary_interval=interval))
    assert str(per_loop) in str(e.value) and str(interval) in str(e.value)


def test_trainer_config_keys():
  from mmt_amd import configs
  cfg = configs.TrainerConfig()
  assert cfg.recovery_max_trials is None and cfg.recovery_begin_steps == 0 and cfg.loss_upper_bound == 1e6
  assert cfg.validation_summary_subdir == 'validation'
  exp = configs.get_exp_config('mmt/pretraining')
  exp.override({'trainer': {'recovery_max_trials': 3, 'recovery_begin_steps': 10, 'loss_upper_bound': 50.0,
                            'validation_summary_subdir': 'ev'}}, strict=True)
  t = exp.trainer
  assert (t.recovery_max_trials, t.recovery_begin_steps, t.loss_upper_bound, t.validation_summary_subdir) == (3, 10, 50.0, 'ev')
  assert exp.as_dict()['trainer']['recovery_max_trials'] == 3


# ---- recovery -----------------------------------------------------------------------------------------------------------------
def test_recovery_rule():
  from mmt_amd import configs, train
  assert train.Recovery.from_config(configs.TrainerConfig()) is None       # the default: no check
  r = train.Recovery(max_trials=5, begin_steps=10, loss_upper_bound=100.0)
  for step in (0, 1, 9, 10, 1000):
    for bad in (float('nan'), float('inf'), float('-inf')):
      assert r.should_recover(step, bad), (step, bad)
  for step, loss, want in ((9, 1e30, False), (10, 1e30, True), (11, 100.5, True), (10, 100.0, False), (10 ** 6, 100.0, False),
                           (10, 99.0, False), (10, -1e30, False), (0, 100.5, False)):
    assert r.should_recover(step, loss) is want, (step, loss)
  assert r.trials == 0                                           # asking counts nothing
  cfg = configs.TrainerConfig()
  cfg.override({'recovery_max_trials': 1, 'recovery_begin_steps': 4, 'loss_upper_bound': 1e-9}, strict=True)
  c = train.Recovery.from_config(cfg)
  assert (c.max_trials, c.begin_steps, c.loss_upper_bound) == (1, 4, 1e-9)


@pytest.mark.parametrize('limit', [0, 1, 2])
def test_recovery_counter_and_its_end(limit):
  from mmt_amd import train
  r = train.Recovery(max_trials=limit, begin_steps=0, loss_upper_bound=10.0)
  assert r.check(5, 9.0) is None and r.check(5, 10.0) is None and r.trials == 0
  for k in range(1, limit + 1):
    assert r.check(10 * k, float('nan') if k % 2 else 11.0) == k and r.trials == k
    assert r.check(10 * k + 1, 1.0) is None and r.trials == k    # a healthy loop does not reset the counter
  with pytest.raises(RuntimeError) as e:
    r.check(77, 12.5)
  text = str(e.value)
  assert 'step 77' in text and '12.5' in text and f'trial {limit + 1} of {limit}' in text
  assert r.trials == limit + 1
