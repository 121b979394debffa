"""NumPy restatement of the map edit (include/gs_abi.h, gs_prune_classify / gs_prune_apply), for the tests.

The DECISION is restated in float32, one rounding per operation, as the kernel is specified (csrc/map_edit.hip is compiled
without contraction): keep <=> opa > opa_logit_min and sqrt(a a + b b + c c) < scale_max with (a, b, c) = |s| or exp(s).  With
the abs activation every operation is correctly rounded on both sides and the restatement keeps exactly the kernel's rows;
numpy's float32 exp and the device's expf may differ in the last bit, so a test that uses the exp activation keeps its norms
away from scale_max (``norm``).  The MOVE is a stable compaction: the kept rows, in order."""
import math

import numpy as np


def opa_logit(p):
    """A probability as the float32 logit the kernel compares: computed in double, rounded once."""
    return np.float32(-math.log(1.0 / float(p) - 1.0))


def norm(scale, activation):
    """||act(scale)|| per row in float32, one rounding per operation, summed left to right."""
    s = np.asarray(scale, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.abs(s) if activation == "abs" else np.exp(s).astype(np.float32)
        sq = (a * a).astype(np.float32)
        return np.sqrt(((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32)).astype(np.float32)


def keep_mask(scale, opa, opa_logit_min, scale_max, activation):
    """boolean [N]: the rows that stay.  A NaN on either side of either comparison is not kept."""
    opa = np.asarray(opa, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (opa > np.float32(opa_logit_min)) & (norm(scale, activation) < np.float32(scale_max))


def compact(arrays, mask):
    """The kept rows of every array, in order."""
    return [np.asarray(a)[mask] for a in arrays]
