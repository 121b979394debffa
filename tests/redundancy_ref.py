"""NumPy restatement of the redundancy histogram (include/gs_abi.h, gs_view_redundancy; csrc/redundancy.hip), for the tests.

Built on the float32 decisions the overlap tests already hold against the kernel and the host compilation of
csrc/overlap_point.h: ``overlap_ref.seen_f32`` for centred cameras, ``pp_testutil.overlap_seen_f32`` where the source or a view
has a principal-point offset.  Nothing of either file is changed."""
import numpy as np

import overlap_ref as R

BINS = 8


def hist_from_seen(seen, self_index):
    """seen bool [n_views, points] -> hist [9] int64: per point c = the views other than ``self_index`` (-1: none left out) that
    see it; bins 0..6 count the points with c == b, bin 7 those with c >= 7, entry 8 the points."""
    seen = np.asarray(seen, bool)
    if self_index >= 0:
        seen = np.delete(seen, self_index, 0)
    c = seen.sum(0).astype(np.int64)
    hist = np.zeros(BINS + 1, np.int64)
    hist[:BINS] = np.bincount(np.minimum(c, BINS - 1), minlength=BINS)
    hist[BINS] = seen.shape[1]
    return hist


def hist_f32(z, cam, views, self_index, stride, near, border):
    """The contract in float32: the measured lattice pixels of ``z`` seen from ``cam``, counted against ``views``."""
    from gs_geometry import principal_point_offset

    if any(principal_point_offset(c) != (0.0, 0.0) for c in [cam] + list(views)):
        import pp_testutil as P

        seen = P.overlap_seen_f32(z, cam, views, stride, near, border)
    else:
        seen = R.seen_f32(z, cam, views, stride, near, border)
    return hist_from_seen(seen, self_index)
