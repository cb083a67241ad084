"""Host-side state between a backward node and the launch that serves it: the queue of launches a backward pass puts
off until several can go together, and the one path by which a parameter whose gradient a kernel wrote itself is
reported ready.  Knows nothing of the kernels -- `fused.py` makes the two queues (weight-gradient products, column-sum
reduces) and hands each its launch function."""
from __future__ import annotations

import collections

import torch


def notify_grad_ready(param) -> None:
  """Kernels that add a gradient straight into `param.grad` return None to autograd and call this once the write is
  enqueued on the current stream (`_mmt_grad_ready_hooks`: the data-parallel bucket reducer)."""
  for hook in getattr(param, '_mmt_grad_ready_hooks', ()):
    hook(param)


# While `_mmt_grad_deferred` is set the parameter's gradient product is queued, not launched: the reducer ignores autograd's
# own post-accumulate notification for it, so a bucket's all-reduce can never be enqueued ahead of its last product.
def mark_grad_deferred(*params) -> None:
  for p in params:
    p._mmt_grad_deferred = True


def clear_grad_deferred(*params) -> None:
  for p in params:
    p._mmt_grad_deferred = False


# What the queues hold.  A column-sum reduce: the partial sums a *_bwd kernel left in `ws` (kept alive here), to be added
# to `outs`.  A weight-gradient product dw += dy^T x (dbias += column sums of dy); `notify`: the parameters to report
# ready.  `ranges`: `_byte_range` of every output.
Reduce = collections.namedtuple('Reduce', 'ws rows H kind outs ranges')
Product = collections.namedtuple('Product', 'dw dy x dbias notify ranges')


def _byte_range(t: torch.Tensor):
  """[lo, hi) addresses a row-strided 2-D (or contiguous 1-D) tensor spans, gaps between its rows included."""
  lo = t.data_ptr()
  n = t.numel() if t.dim() != 2 else (t.shape[0] - 1) * t.stride(0) + t.shape[1]
  return lo, lo + n * t.element_size()


def _ranges_overlap(a, b) -> bool:
  return any(x[0] < y[1] and y[0] < x[1] for x in a for y in b)


_GRAPH_TASK_ID = getattr(torch._C, '_current_graph_task_id', None)


def _graph_task_id():
  return _GRAPH_TASK_ID() if _GRAPH_TASK_ID is not None else -1


def grouping_is_safe() -> bool:
  """The queues tell a new backward pass from a stale one by autograd's graph-task id.  Without that symbol every pass
  would look alike and items left behind by a backward that raised would be launched (with dead operands) by the next
  one: fail closed -- nothing is queued, every product and reduce is launched on its own."""
  return _GRAPH_TASK_ID is not None


_QUEUES = []                  # every DeferredLaunches, in creation order


class DeferredLaunches:
  """Items of one kind waiting to go into one launch.  `entries`: (device, graph-task id) -> [items], ONE entry per
  backward pass and device, launched on the current stream of its device by the end-of-backward callback of ITS pass
  (the callback runs under that id) or sooner, when it is full.  A re-entrant pass (torch.utils.checkpoint(...,
  use_reentrant=True) runs one inside a node of the outer pass) has an id and an entry of its own.
  In one launch the items are added to their outputs by different workgroups with plain loads and stores, so an item
  whose output ranges overlap a queued one's (a parameter used twice in the pass, or a view into the same gradient
  buffer) makes the entry launch first; the two contributions then follow each other on the stream.
  What differs between the queues is handed in: `launch(items, device)`; `limit(items)`, the number of items at which the
  entry launches; `may_join(items, item)`, False for one more reason to launch first; `on_queued(item)`,
  `on_launched(items)` and `on_dropped(item)`, what else to do then."""

  def __init__(self, launch, limit, may_join=None, on_queued=None, on_launched=None, on_dropped=None):
    skip = lambda *_: True         # (a queue without the rule or the action: every item may join, nothing else to do)
    self.launch, self.limit, self.may_join = launch, limit, may_join or skip
    self.on_queued, self.on_launched, self.on_dropped = on_queued or skip, on_launched or skip, on_dropped or skip
    self.entries = {}
    _QUEUES.append(self)

  def __len__(self) -> int:
    return len(self.entries)

  def queued(self):
    """Every waiting item, of every pass and device."""
    return [item for items in self.entries.values() for item in items]

  def add(self, device, item) -> None:
    gid = _graph_task_id()
    key = (device, gid)
    forget_passes_after(gid)
    items = self.entries.get(key)
    if items and (not self.may_join(items, item) or any(_ranges_overlap(item.ranges, q.ranges) for q in items)):
      self.flush(key)
      items = None
    if items is None:
      items = self.entries[key] = []
      torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)
    self.on_queued(item)
    items.append(item)
    if len(items) >= self.limit(items):
      self.flush(key)              # (a later item opens a new entry and queues another callback: harmless)

  def flush(self, key) -> None:
    items = self.entries.pop(key, None)
    if items:
      self.launch(items, key[0])
      self.on_launched(items)

  def _end_of_backward(self) -> None:
    """The entries of the pass that is ending.  Every queue has a callback of its own, queued when its entry was opened:
    the launches at the end of a pass -- the nodes of a recorded step -- come in the order the queues were first used."""
    gid = _graph_task_id()
    for key in [k for k in self.entries if k[1] == gid]:
      self.flush(key)
    forget_passes_after(gid)

  def drop(self, keys) -> None:
    """Forgets entries without launching them."""
    for key in keys:
      for item in self.entries.pop(key):
        self.on_dropped(item)


def forget_passes_after(gid) -> None:
  """A pass whose id is larger than the running one's began after it, i.e. inside one of its nodes, and has returned: what
  it still has queued was left behind when it raised (its end-of-backward callback never ran) and is nobody's to launch."""
  for queue in _QUEUES:
    queue.drop([key for key in queue.entries if key[1] > gid])


def forget_stale_queues() -> None:
  """Called where a forward pass starts work (descriptors, the step's seed stream): OUTSIDE any backward pass every queued
  item was left behind by a pass that raised -- its operands belong to a step that is over -- and is dropped.  (Inside
  one -- a checkpointed segment recomputed by the outer pass -- the outer pass's items are alive and stay.)"""
  if any(queue.entries for queue in _QUEUES) and _graph_task_id() == -1 and grouping_is_safe():
    reset_host_queues()


def reset_host_queues() -> None:
  """Forgets every weight-gradient product and column-sum reduce a backward pass has queued but not launched.  For a step
  that was ABANDONED half-way (a graph capture that raised inside backward, `graphed.py`): its queued products point at
  activations of a step that never ran; the retry must not launch them."""
  for queue in _QUEUES:
    queue.drop(list(queue.entries))
