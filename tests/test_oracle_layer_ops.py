"""The fp64 oracle of the loss kernels on -inf logits (host only): the GPU tests compare against it, so it has to be
finite itself -- checked with every numpy floating-point warning turned into an error."""
import numpy as np

from oracle import layer_ops as lo
from tests._layer_cases import XENT_INF_LABEL_ROW, first_argmax, xent_neg_inf_case


def test_softmax_xent_oracle_is_finite_on_neg_inf_logits():
  x, labels, _ = xent_neg_inf_case()
  with np.errstate(all='raise'):
    loss, d = lo.softmax_xent(x, labels)
  other = np.arange(x.shape[0]) != XENT_INF_LABEL_ROW
  assert np.isfinite(loss[other]).all()
  assert loss[XENT_INF_LABEL_ROW] == np.inf            # label on a -inf column: -log(0)
  assert np.isfinite(d).all()
  # softmax - onehot: rows sum to 0, masked classes get exactly 0 (exactly -1 where the label sits on one)
  assert np.abs(d.sum(-1)).max() < 1e-12
  masked = np.isneginf(x)
  masked[XENT_INF_LABEL_ROW, labels[XENT_INF_LABEL_ROW]] = False
  assert not d[masked].any()
  assert d[XENT_INF_LABEL_ROW, labels[XENT_INF_LABEL_ROW]] == -1.0
  # an independent restatement over the finite entries only
  for r in range(x.shape[0]):
    fin = x[r][np.isfinite(x[r])].astype(np.float64)
    lse = np.log(np.exp(fin - fin.max()).sum()) + fin.max()
    if r != XENT_INF_LABEL_ROW:
      assert abs(loss[r] - (lse - x[r, labels[r]])) < 1e-12


def test_first_argmax_takes_the_first_of_equal_maxima():
  x = np.array([[1.0, 3.0, 3.0, -np.inf], [-np.inf, -np.inf, 0.0, 0.0]])
  assert first_argmax(x).tolist() == [1, 2]
