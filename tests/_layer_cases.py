"""Inputs shared by the edge tests of the loss, row and GEMM kernels (tests/test_gpu_layer_edges.py,
tests/test_gpu_gemm_layouts.py) and the host test of their oracle (tests/test_oracle_layer_ops.py)."""
import numpy as np

XENT_INF_ROWS, XENT_INF_C = 6, 1001
XENT_INF_LABEL_ROW = 4          # the row whose label sits on a -inf column: loss +inf, finite gradient


def xent_neg_inf_case(label_on_inf=True):
  """[6, 1001] fp32 logits with -inf entries, labels and per-row coefficients.  A workgroup of the loss kernel has 256
  threads and thread t starts at column t (fp32) or at columns 2t, 2t + 1 (bf16):
    row 0  columns 0..255 at -inf: the first element of EVERY thread (fp32), of half the threads (bf16);
    row 1  every even column at -inf: the first element of every bf16 thread, of every other fp32 thread;
    row 2  columns 300.. at -inf: a finite running maximum meets -inf, and so does the odd last element;
    row 3  a single -inf at column C - 1 (the odd tail of the paired bf16 path);
    row 4  a -inf at column 17 with the label on it (`label_on_inf`; else the label is on column 18);
    row 5  no -inf at all.
  All other labels lie on finite columns."""
  rows, C = XENT_INF_ROWS, XENT_INF_C
  rng = np.random.default_rng(20211)
  x = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
  x[0, :256] = -np.inf
  x[1, 0::2] = -np.inf
  x[2, 300:] = -np.inf
  x[3, C - 1] = -np.inf
  x[4, 17] = -np.inf
  labels = np.array([500, 501, 7, 10, 17 if label_on_inf else 18, 333], dtype=np.int64)
  coef = (rng.standard_normal(rows) + 2.0).astype(np.float32)
  return x, labels, coef


def first_argmax(x):
  """First index of the row maximum (tf.argmax's tie rule), built explicitly: numpy's argmax promises it too, but the
  metric tests spell it out and so does this."""
  mx = x.max(-1, keepdims=True)
  idx = np.where(x == mx, np.arange(x.shape[1])[None, :], x.shape[1])
  return idx.min(-1)
