"""A loader that runs ahead of the step ("Records", "Prefetch on a side stream").

`Prefetcher(batches, device=..., depth=2)` wraps any iterator of `(inputs, labels)` -- nests of dicts, tuples, lists and
tensors, as the loaders and `input_utils.synthetic_batch` yield them.  One daemon thread runs the wrapped iterator: it
sets its device, runs the whole generator body under `torch.cuda.stream(side)`, a stream the prefetcher owns (the current
device and the current stream are per thread in torch, and every stage launches on the current stream), records an event
on `side` behind each batch and puts `(batch, event)` into a `queue.Queue(maxsize=depth)`.  `__next__` takes one, makes
the consumer's current stream wait for the event, calls `record_stream` on every tensor of the nest and returns the
batch: the consumer never waits on the host for the device, and the worker is never more than `depth` finished batches
plus the one in work ahead.  `device='cpu'` is thread and queue only.  The thread starts with the first `__next__`, so an
iterator that is built and dropped unread (`evaluation.validation_source`) reads nothing.

The capture gate.  `torch.cuda.graph` captures in global mode: while any thread is capturing, an allocation or a
synchronising call in another thread invalidates the capture and fails in that other thread, and the loaders make both
kinds of call (fresh tensors, the checksum and JPEG status read-backs, the pack's `int(consumed)`).  `capture_gate` is one
module-level lock: the worker holds it from resuming the generator until the batch's event is recorded and releases it
before the blocking `put`; the capture sites (`graphed.GraphedTrainStep._record`, `evaluation.GraphedEvalStep._record`,
`retrieval.PairScorer._record`) take it around their `with torch.cuda.graph(...)` block.  With no prefetcher alive the
lock is uncontended; a recorder waits for at most one batch; replays are not gated."""
from __future__ import annotations

import contextlib
import dataclasses
import itertools
import queue
import threading

import torch

capture_gate = threading.Lock()

THREAD_PREFIX = 'mmt-prefetch-'
_POLL = 0.05                     # seconds between looks at the stop flag while the worker or the consumer waits
_JOIN = 5.0                      # bound of close()'s join
_ids = itertools.count()
_OK, _END, _ERR = 0, 1, 2


def tensors(nest):
  """Every tensor of a nest of dicts, tuples, lists, tensors and dataclass instances (their attributes)."""
  if torch.is_tensor(nest):
    yield nest
  elif isinstance(nest, dict):
    for v in nest.values():
      yield from tensors(v)
  elif isinstance(nest, (tuple, list)):
    for v in nest:
      yield from tensors(v)
  elif dataclasses.is_dataclass(nest) and not isinstance(nest, type):
    for v in vars(nest).values():
      yield from tensors(v)


def check_buffer_size(value) -> int:
  """`prefetch_buffer_size` as a depth: None or 0 is off; a negative value is a ValueError."""
  depth = int(value or 0)
  if depth < 0:
    raise ValueError('prefetch_buffer_size must not be negative')
  return depth


class Prefetcher:
  """Iterator, `close()`, context manager.  The batches are the wrapped iterator's, in its order; an exception in the
  worker is re-raised by the `__next__` that would have returned the batch it interrupted, after all earlier batches;
  exhaustion is StopIteration, again on every later call; with `timeout` a `__next__` that waits longer raises
  TimeoutError."""

  def __init__(self, batches, *, device, depth: int = 2, timeout: float = None):
    if int(depth) < 1:
      raise ValueError('Prefetcher: depth must be at least 1')
    self._it = iter(batches)
    self.device = torch.device(device)
    self.depth, self.timeout = int(depth), timeout
    self._cuda = self.device.type == 'cuda'
    if self._cuda and self.device.index is None:       # the worker thread needs the index: its current device is its own
      self.device = torch.device('cuda', torch.cuda.current_device())
    self._side = torch.cuda.Stream(self.device) if self._cuda else None
    self._q = queue.Queue(maxsize=self.depth)
    self._stop = threading.Event()
    self._finished = self._closed = False
    self._thread = threading.Thread(target=self._work, name=f'{THREAD_PREFIX}{next(_ids)}', daemon=True)
    self._started = False

  # ---- the worker ------------------------------------------------------------------------------------------------------------
  def _produce(self):
    """One item, under the gate: (kind, batch or exception, event)."""
    while not capture_gate.acquire(timeout=_POLL):
      if self._stop.is_set():
        return None
    try:
      if self._stop.is_set():
        return None
      try:
        batch = next(self._it)
      except StopIteration:
        return (_END, None, None)
      except BaseException as e:      # handed to the consumer, whatever it is
        return (_ERR, e, None)
      event = None
      if self._cuda:
        event = torch.cuda.Event()
        event.record(self._side)
      return (_OK, batch, event)
    finally:
      capture_gate.release()

  def _work(self):
    try:
      if self._cuda:
        torch.cuda.set_device(self.device)
      with (torch.cuda.stream(self._side) if self._cuda else contextlib.nullcontext()):
        while not self._stop.is_set():
          item = self._produce()
          while item is not None:
            if self._stop.is_set():                    # a batch finished behind close() is dropped, not delivered
              item = None
              break
            try:
              self._q.put(item, timeout=_POLL)
              break
            except queue.Full:
              if self._stop.is_set():
                item = None
          if item is None or item[0] != _OK:
            return
    except BaseException as e:                         # outside the iterator (device, stream): the consumer hears of it too
      while not self._stop.is_set():
        try:
          self._q.put((_ERR, e, None), timeout=_POLL)
          break
        except queue.Full:
          pass
    finally:
      close = getattr(self._it, 'close', None)       # the wrapped generator ends in the thread that ran it
      if close is not None:
        try:
          close()
        except Exception:
          pass

  # ---- the consumer ----------------------------------------------------------------------------------------------------------
  def __iter__(self):
    return self

  def __next__(self):
    if self._finished or self._closed:
      raise StopIteration
    if not self._started:
      self._started = True
      self._thread.start()
    waited = 0.0
    while True:
      try:
        kind, payload, event = self._q.get(timeout=_POLL if self.timeout is None else min(_POLL, max(self.timeout - waited, 1e-3)))
        break
      except queue.Empty:
        waited += _POLL
        if self._closed:
          raise StopIteration from None
        if self.timeout is not None and waited >= self.timeout:
          raise TimeoutError(f'Prefetcher: no batch within {self.timeout} s') from None
    if kind == _END:
      self._finished = True
      raise StopIteration
    if kind == _ERR:
      self._finished = True
      raise payload
    if self._cuda:
      current = torch.cuda.current_stream(self.device)
      current.wait_event(event)
      for t in tensors(payload):
        if t.is_cuda:
          t.record_stream(current)
    return payload

  def close(self) -> None:
    """Idempotent; safe while the worker is blocked on a full queue, waiting at the gate or in the middle of a batch.
    Sets the stop flag, empties the queue, joins with a bound; the worker closes the wrapped generator.  After it
    returns the wrapped iterator is not advanced again."""
    self._closed = True
    self._stop.set()
    if not self._started:
      self._started = True                             # never starts; the generator is closed here, nothing ran it
      close = getattr(self._it, 'close', None)
      if close is not None:
        close()
      return
    self._drain()
    self._thread.join(_JOIN)
    self._drain()

  def _drain(self):
    try:
      while True:
        self._q.get_nowait()
    except queue.Empty:
      pass

  @property
  def alive(self) -> bool:
    return self._thread.is_alive()

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()
    return False

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass
