"""NumPy restatement of gs_densify_apply_state (include/gs_abi.h), for the tests.

``classes`` is the decision of oracle/densify_ref.py per INPUT row, derived as tests/test_gpu_step_regimes.py derives it
(``oracle_classes``), with the thresholds as arguments: 0 deleted, 1 kept, 2 kept + cloned, 3 kept + split.  In float32, one
rounding per operation; exact for the abs activation (numpy's float32 exp and the device's expf may differ in the last bit).

``apply_state`` is the table of the header: with K, C, S the numbers of non-deleted, cloned and split rows and kept_rank(i) the
number of non-deleted rows before row i, for every array
    class 1 or 2 : dst[kept_rank(i)] = src[i]
    class 3      : dst[kept_rank(i)] = 0
    class 0      : nothing
    rows [K, K + C + S) : 0
and nothing else exists: the result has exactly K + C + S rows."""
import numpy as np

from oracle import densify_ref

DELETE, KEEP, CLONE, SPLIT = 0, 1, 2, 3


def classes(scale, opa, grad, activation="abs", aggregation="max", use_clone=True, use_split=True, taus=0.05,
            delete_thresh=0.17, grad_thresh=0.0002):
    f = np.float32
    scale, opa, grad = (np.asarray(a, f) for a in (scale, opa, grad))
    a = np.abs(scale) if activation == "abs" else np.exp(scale)
    norm = np.sqrt((a * a).sum(-1, dtype=f))
    keep = (opa > f(densify_ref.inverse_sigmoid(0.02))) & (norm < f(delete_thresh))
    g = np.abs(grad).max(-1) if aggregation == "max" else np.abs(grad).mean(-1, dtype=f)
    dens = keep & (g > f(grad_thresh))
    cls = keep.astype(np.int32)
    cls[dens & (norm <= f(taus)) & bool(use_clone)] = CLONE
    cls[dens & (norm > f(taus)) & bool(use_split)] = SPLIT
    return cls


def counts(cls):
    """(K, C, S): non-deleted, cloned, split."""
    cls = np.asarray(cls)
    return int((cls != DELETE).sum()), int((cls == CLONE).sum()), int((cls == SPLIT).sum())


def apply_state(cls, arrays):
    """-> every destination array, K + C + S rows each."""
    cls = np.asarray(cls)
    k, c, s = counts(cls)
    kept = cls != DELETE
    zero = cls[kept] == SPLIT
    out = []
    for a in arrays:
        a = np.asarray(a, np.float32)
        assert a.shape[0] == cls.shape[0]
        d = np.zeros((k + c + s,) + a.shape[1:], np.float32)
        rows = a[kept].copy()
        rows[zero] = 0
        d[:k] = rows
        out.append(d)
    return out
