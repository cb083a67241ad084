"""Cases, oracle and guarded call of the row packing (`mmt_pack_rows` / `mmt_pack_rows_host`), shared by
tests/test_pack_rows_host.py and tests/test_gpu_pack_rows.py.

The oracle is the rule as the issue states it -- a ten-line next-fit in arrival order -- plus
`input_utils.packed_example_layout` for the three layout tensors: it knows nothing of prefix sums or searches.  The call
goes through ctypes with every output inside a buffer pre-filled with a sentinel and guarded by 16 sentinel elements on
both sides, so "every element written, nothing outside" is checked for every case."""
import ctypes
import functools

import numpy as np
import torch

GUARD = 16
SENTINEL = {torch.int32: -0x5A5A5A5A, torch.int64: -0x5A5A5A5A5A5A5A5A, torch.float32: -12345.5}


def _case(S, S_row, R, E_max, lengths, n_mlm=3, n_mpp=2):
  return dict(S=S, S_row=S_row, R=R, E_max=E_max, lengths=list(lengths), n_mlm=n_mlm, n_mpp=n_mpp)


def _many(E, S, seed):
  return [int(x) for x in np.random.default_rng(seed).integers(1, S + 1, E)]


CASES = {
    'all-fit-absent-slots': _case(8, 20, 3, 8, [5, 6, 7, 3, 8]),              # E_max > E: three absent slots
    'row-filled-exactly': _case(8, 16, 3, 5, [8, 8, 4, 6, 6, 2]),             # 8 + 8 == S_row; E_max < E stops before the last
    'one-over-opens-a-row': _case(8, 16, 3, 6, [8, 7, 2, 8, 8, 1]),           # 8 + 7 + 2 == 17
    'stop-at-row-R': _case(8, 16, 2, 9, [8, 7, 2, 8, 8, 1, 3, 3, 3]),         # consumed < E
    'stop-at-E-max': _case(8, 64, 2, 3, [5, 6, 7, 3, 8]),
    'one-example': _case(8, 11, 2, 1, [6]),
    'one-row': _case(8, 19, 1, 6, [4, 8, 7, 5]),                              # 4 + 8 + 7 == 19, the fourth would open row 1
    'length-equals-S-row': _case(12, 12, 4, 5, [12, 3, 12, 9, 3]),
    'lengths-clamped': _case(8, 16, 4, 7, [0, -5, 100, 3, 2 ** 31 - 1, -2 ** 31, 8]),
    'many-lanes': _case(24, 64, 400, 1100, _many(1000, 24, 3)),               # several lanes of the plan, a ragged last lane
    'limit-4096': _case(4, 8, 2100, 4096, _many(4096, 4, 4), n_mlm=1, n_mpp=1),   # E == E_max == the limit
}


def next_fit(lengths, S, R, S_row, E_max):
  """(lengths of the examples of every row, examples consumed)."""
  rows, used, consumed = [[]], 0, 0
  for n in list(lengths)[:E_max]:
    n = min(max(int(n), 1), S)
    if used + n > S_row:
      if len(rows) == R:
        break
      rows.append([])
      used = 0
    rows[-1].append(n)
    used += n
    consumed += 1
  return rows + [[] for _ in range(R - len(rows))], consumed


@functools.lru_cache(maxsize=None)
def case_data(name, tables=True):
  """Inputs and expected outputs of a case, computed once: dicts of CPU tensors."""
  from mmt_amd import input_utils
  c = CASES[name]
  S, S_row, R, E_max = c['S'], c['S_row'], c['R'], c['E_max']
  E = len(c['lengths'])
  g = torch.Generator().manual_seed(len(name) + E)
  ins = {'word_ids': torch.randint(1, 30000, (E, S), generator=g, dtype=torch.int32),
         'segment_ids': torch.randint(0, 3, (E, S), generator=g, dtype=torch.int32),
         'lengths': torch.tensor(c['lengths'], dtype=torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)}
  rows, consumed = next_fit(c['lengths'], S, R, S_row, E_max)
  flat = [n for row in rows for n in row]
  if tables:      # positions inside the example, as the masking stage gives them; unused entries are 0
    for k, n in (('mlm_positions', c['n_mlm']), ('mpp_positions', c['n_mpp'])):
      clamped = torch.tensor([min(max(int(x), 1), S) for x in c['lengths']])
      ins[k] = (torch.rand(E, n, generator=g) * clamped[:, None]).to(torch.int32)
  ids, starts, slots, first = input_utils.packed_example_layout(rows, [[True] * len(r) for r in rows], S_row)
  want = {'word_ids': torch.zeros(R, S_row, dtype=torch.int32), 'segment_ids': torch.zeros(R, S_row, dtype=torch.int32),
          'example_ids': ids, 'example_starts': starts, 'patch_slots': slots,
          'first_positions': torch.zeros(E_max, 2, dtype=torch.int64), 'example_weight': torch.zeros(E_max),
          'consumed': torch.tensor([consumed], dtype=torch.int32)}
  want['first_positions'][:consumed] = first
  want['example_weight'][:consumed] = 1
  for e, ((r, at), n) in enumerate(zip(first.tolist(), flat)):
    want['word_ids'][r, at:at + n] = ins['word_ids'][e, :n]
    want['segment_ids'][r, at:at + n] = ins['segment_ids'][e, :n]
  if tables:
    for k in ('mlm_positions', 'mpp_positions'):
      want[k] = torch.zeros(E_max, ins[k].shape[1], dtype=torch.int32)
      want[k][:consumed] = (first[:, :1] * S_row + first[:, 1:] + ins[k][:consumed]).to(torch.int32)
  return c, ins, want, consumed


def guarded(shape, dtype, device):
  """(interior view, whole buffer): the interior and 16 elements on both sides hold the sentinel."""
  n = int(np.prod(shape))
  whole = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=device)
  return whole[GUARD:GUARD + n].view(shape), whole


def call(ins, S, S_row, R, E_max, device, host=None):
  """The raw entry point on `device` with guarded outputs and a guarded workspace.  Returns (rc, outputs, buffers)."""
  from mmt_amd import _lib
  L = _lib.lib()
  ins = {k: v.to(device).contiguous() for k, v in ins.items()}
  E = ins['word_ids'].shape[0]
  d = _lib.PackDesc()
  d.E, d.S, d.R, d.S_row, d.E_max = E, S, R, S_row, E_max
  mlm, mpp = ins.get('mlm_positions'), ins.get('mpp_positions')
  d.n_mlm, d.n_mpp = (0 if mlm is None else mlm.shape[1]), (0 if mpp is None else mpp.shape[1])
  out, whole = {}, {}
  def add(name, shape, dtype=torch.int32):
    out[name], whole[name] = guarded(shape, dtype, device)
  for k in ('word_ids', 'segment_ids', 'example_ids', 'example_starts', 'patch_slots'):
    add(k, (R, S_row))
  add('first_positions', (E_max, 2), torch.int64)
  add('example_weight', (E_max,), torch.float32)
  if mlm is not None:
    add('mlm_positions', (E_max, d.n_mlm))
  if mpp is not None:
    add('mpp_positions', (E_max, d.n_mpp))
  add('consumed', (1,))
  nbytes = L.mmt_pack_rows_workspace_bytes(d)
  assert nbytes >= 4 * (R + 1 + 2 * E) and nbytes % 16 == 0
  ws, whole['workspace'] = guarded((nbytes // 4,), torch.int32, device)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
  args = [d, p(ins['word_ids']), p(ins['segment_ids']), p(ins['lengths']), p(mlm), p(mpp), p(out['word_ids']), p(out['segment_ids']),
          p(out['example_ids']), p(out['example_starts']), p(out['patch_slots']), p(out['first_positions']),
          p(out['example_weight']), p(out.get('mlm_positions')), p(out.get('mpp_positions')), p(out['consumed']), p(ws), nbytes]
  if torch.device(device).type == 'cuda':
    rc = L.mmt_pack_rows(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
  else:
    rc = L.mmt_pack_rows_host(*args)
  return rc, out, whole


def check_guards(out, whole):
  """Nothing outside the outputs was written; the workspace's own guards too."""
  for name, w in whole.items():
    s = SENTINEL[w.dtype]
    w = w.cpu()
    assert bool((w[:GUARD] == s).all()) and bool((w[-GUARD:] == s).all()), f'{name}: a guard element was written'


def check_case(name, tables, device):
  c, ins, want, consumed = case_data(name, tables)
  rc, out, whole = call(ins, c['S'], c['S_row'], c['R'], c['E_max'], device)
  from mmt_amd import _lib
  assert rc == 0, _lib.lib().mmt_last_error().decode()
  check_guards(out, whole)
  assert out.keys() == want.keys()
  for k, w in want.items():
    got = out[k].cpu()
    assert not bool((got == SENTINEL[got.dtype]).any()), f'{k}: an element was not written'
    assert torch.equal(got, w), (k, int((got != w).sum()))
  return consumed
