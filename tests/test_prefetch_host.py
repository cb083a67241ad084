"""`mmt_amd.prefetch.Prefetcher` on `device='cpu'` (thread and queue only) over plain Python iterators: order, how far the
worker runs ahead, errors, exhaustion, `close()` in every state of the worker, the capture gate, and the wiring of
`MmtDataConfig.prefetch_buffer_size` into `build_inputs`.  Every wait is bounded: the prefetchers have a `timeout`, the
test's own waits a deadline."""
import json
import threading
import time

import pytest
import torch

from tests import _record_cases as R

WAIT = 10.0


def until(cond, limit=WAIT):
  end = time.monotonic() + limit
  while not cond():
    assert time.monotonic() < end, 'the condition did not come true in time'
    time.sleep(0.005)


def batches(n):
  for i in range(n):
    yield {'x': torch.full((2,), i), 'nest': (torch.tensor([i]), [i])}, {'y': torch.tensor(i)}


class Counting:
  """An iterator that counts how often it was advanced; `hold` makes an item wait for the test inside `__next__`."""

  def __init__(self, n=10 ** 9, fail_at=None, hold=None):
    self.n, self.fail_at, self.hold = n, fail_at, hold
    self.advanced = 0
    self.inside = threading.Event()
    self.closed = False

  def __iter__(self):
    return self

  def __next__(self):
    i = self.advanced
    if i >= self.n:
      raise StopIteration
    if self.fail_at is not None and i == self.fail_at:
      raise KeyError(f'record {i} is broken')
    if self.hold is not None:
      self.inside.set()
      assert self.hold.wait(WAIT)
    self.advanced += 1
    return ({'i': torch.tensor(i)}, {})

  def close(self):
    self.closed = True


def workers():
  from mmt_amd import prefetch
  return [t for t in threading.enumerate() if t.name.startswith(prefetch.THREAD_PREFIX)]


@pytest.mark.parametrize('depth', [1, 3])
def test_same_sequence_as_the_wrapped_iterator(depth):
  from mmt_amd import prefetch
  with prefetch.Prefetcher(batches(7), device='cpu', depth=depth, timeout=WAIT) as p:
    got = list(p)
  assert len(got) == 7
  for (gi, gl), (wi, wl) in zip(got, batches(7)):
    assert torch.equal(gi['x'], wi['x']) and torch.equal(gi['nest'][0], wi['nest'][0]) and gi['nest'][1] == wi['nest'][1]
    assert torch.equal(gl['y'], wl['y'])
  for _ in range(3):                                           # exhaustion repeats
    with pytest.raises(StopIteration):
      next(p)
  until(lambda: not workers())


@pytest.mark.parametrize('depth', [1, 3])
def test_the_worker_is_never_more_than_depth_plus_one_ahead(depth):
  from mmt_amd import prefetch
  src = Counting()
  with prefetch.Prefetcher(src, device='cpu', depth=depth, timeout=WAIT) as p:
    for taken in range(1, 6):
      inputs, _ = next(p)
      assert int(inputs['i']) == taken - 1
      until(lambda: src.advanced == taken + depth + 1)         # it fills the queue and holds one more ...
      time.sleep(0.1)                                          # ... and the stalled consumer sees it go no further
      assert src.advanced == taken + depth + 1
  assert src.closed


def test_an_exception_arrives_at_its_place_with_type_and_message():
  from mmt_amd import prefetch
  k = 4
  p = prefetch.Prefetcher(Counting(fail_at=k), device='cpu', depth=2, timeout=WAIT)
  for i in range(k):
    assert int(next(p)[0]['i']) == i
  with pytest.raises(KeyError, match='record 4 is broken'):
    next(p)
  with pytest.raises(StopIteration):
    next(p)
  p.close()
  until(lambda: not workers())


def test_timeout_is_an_error_not_a_hang():
  from mmt_amd import prefetch
  hold = threading.Event()
  p = prefetch.Prefetcher(Counting(hold=hold), device='cpu', depth=1, timeout=0.3)
  with pytest.raises(TimeoutError):
    next(p)
  hold.set()
  p.close()


def closes_in_time(p):
  t0 = time.monotonic()
  p.close()
  p.close()                                                    # idempotent
  assert time.monotonic() - t0 < 7.0
  return time.monotonic() - t0


def test_close_while_blocked_on_a_full_queue():
  from mmt_amd import prefetch
  src = Counting()
  p = prefetch.Prefetcher(src, device='cpu', depth=2, timeout=WAIT)
  next(p)
  until(lambda: src.advanced == 4)                             # one taken, two queued, one waiting at the put
  assert closes_in_time(p) < 2.0
  n = src.advanced
  time.sleep(0.2)
  assert src.advanced == n == 4 and not p.alive and src.closed
  with pytest.raises(StopIteration):
    next(p)


def test_close_while_waiting_at_the_gate_and_the_gate_stops_the_iterator():
  from mmt_amd import prefetch
  src = Counting()
  p = prefetch.Prefetcher(src, device='cpu', depth=2, timeout=0.5)
  with prefetch.capture_gate:
    with pytest.raises(TimeoutError):                          # starts the worker, which waits at the gate
      next(p)
    assert src.advanced == 0                                   # while the gate is held the iterator is not advanced
    assert closes_in_time(p) < 2.0
  time.sleep(0.2)
  assert src.advanced == 0 and not p.alive and src.closed
  # a recorder waits for at most one batch: with the worker mid-item the gate is taken, and free again behind the item
  hold = threading.Event()
  src = Counting(hold=hold)
  p = prefetch.Prefetcher(src, device='cpu', depth=1, timeout=0.2)
  with pytest.raises(TimeoutError):
    next(p)
  assert src.inside.wait(WAIT) and not prefetch.capture_gate.acquire(timeout=0.1)
  hold.set()
  assert prefetch.capture_gate.acquire(timeout=WAIT)
  n = src.advanced
  time.sleep(0.2)
  assert src.advanced == n                                     # held by the test: the worker does not resume the iterator
  prefetch.capture_gate.release()
  p.close()


def test_close_in_the_middle_of_an_item():
  from mmt_amd import prefetch
  hold = threading.Event()
  src = Counting(hold=hold)
  p = prefetch.Prefetcher(src, device='cpu', depth=2, timeout=0.2)
  with pytest.raises(TimeoutError):
    next(p)
  assert src.inside.wait(WAIT)
  closer = threading.Thread(target=p.close)
  closer.start()
  time.sleep(0.1)
  hold.set()                                                   # the item ends; nothing follows it
  closer.join(WAIT)
  assert not closer.is_alive()
  until(lambda: not p.alive)
  assert src.advanced == 1 and src.closed
  with pytest.raises(StopIteration):
    next(p)
  time.sleep(0.1)
  assert src.advanced == 1


def test_an_unread_prefetcher_reads_nothing():
  from mmt_amd import prefetch
  src = Counting()
  p = prefetch.Prefetcher(src, device='cpu', depth=2)
  time.sleep(0.1)
  assert src.advanced == 0 and not workers()
  p.close()
  assert src.closed
  with pytest.raises(ValueError):
    prefetch.Prefetcher(Counting(), device='cpu', depth=0)


# ---- configuration and wiring ------------------------------------------------------------------------------------------------
IMAGE, PATCH, SEQ, BATCH = 32, 16, 32, 4


def task_of(kind, **data):
  import mmt_amd
  from mmt_amd import configs
  exp = configs.get_exp_config(f'mmt/{kind}')
  model = {'num_classes': 2, 'cls_heads': [{'inner_dim': 16, 'num_classes': 2, 'name': 'itm'}]} if kind == 'classification' else {}
  exp.override({'task': {'model': model,
                         'train_data': dict(dict(image_size=IMAGE, patch_size=PATCH, max_seq_len=SEQ, global_batch_size=BATCH,
                                                 text_special_token_field_dict=json.dumps(R.FIELD_DICT)), **data)}})
  return mmt_amd.tasks.get_task(exp.task), exp.task.train_data


ITM_FIELDS = dict(label_field='itm_label_ids', label_weights_field='itm_label_weights', pos_weights_field='itm_pos_weights')


@pytest.mark.parametrize('kind', ['pretraining', 'classification'])
def test_build_inputs_wraps_exactly_when_the_key_is_positive(kind, tmp_path):
  from mmt_amd import _lib, prefetch
  _lib.build()
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  R.write_shards(tmp_path, R.loader_records(4), 1)
  extra = ITM_FIELDS if kind == 'classification' else {'tasks': 'mlm'}
  for source, where in (('synthetic', {}), ('records', dict(input_path=str(tmp_path / '*.tfrecord'), vocab_filename=vocab))):
    for value, depth in ((None, 0), (0, 0), (1, 1), (3, 3)):
      task, d = task_of(kind, prefetch_buffer_size=value, **where, **extra)
      data = task.build_inputs(d, device='cpu')
      assert task.input_source == source
      if depth:
        assert isinstance(data, prefetch.Prefetcher) and task.input_prefetch is data and data.depth == depth
        data.close()
      else:
        assert not isinstance(data, prefetch.Prefetcher) and task.input_prefetch is None
    task, d = task_of(kind, prefetch_buffer_size=-1, **where, **extra)
    with pytest.raises(ValueError, match='prefetch_buffer_size must not be negative'):
      task.build_inputs(d, device='cpu')
  assert not workers()
  if kind == 'pretraining':                                      # the worker runs the stand-in: its refusal of the CPU arrives here
    task, d = task_of(kind, prefetch_buffer_size=2, tasks='mlm')
    data = task.build_inputs(d, device='cpu')
    data.timeout = 60
    with pytest.raises(RuntimeError, match='GPU only'):
      next(data)
    data.close()
    until(lambda: not workers())


def test_the_key_round_trips_and_a_negative_loader_value_raises(tmp_path):
  from mmt_amd import configs, pretrain_dataloader
  assert configs.MmtDataConfig().prefetch_buffer_size is None
  cfg = configs.parse_configuration('mmt/pretraining', params_override='task.train_data.prefetch_buffer_size=3')
  assert cfg.task.train_data.prefetch_buffer_size == 3 and cfg.task.validation_data.prefetch_buffer_size is None
  assert cfg.as_dict()['task']['train_data']['prefetch_buffer_size'] == 3
  path = tmp_path / 'p.yaml'
  path.write_text('task:\n  train_data:\n    prefetch_buffer_size: 2\n  validation_data:\n    prefetch_buffer_size: 1\n')
  cfg = configs.parse_configuration('mmt/pretraining', config_files=[str(path)])
  assert cfg.task.train_data.prefetch_buffer_size == 2 and cfg.task.validation_data.prefetch_buffer_size == 1
  bad = configs.MmtPretrainDataConfig(prefetch_buffer_size=-2, text_special_token_field_dict=json.dumps(R.FIELD_DICT))
  with pytest.raises(ValueError, match='prefetch_buffer_size must not be negative'):
    pretrain_dataloader.MmtPretrainDataLoader(bad, device='cpu')
