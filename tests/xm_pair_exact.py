"""The pairwise relative-rotation filter (tests/xm_pair_numpy.py) in numpy.longdouble with a sort-based trimmed mean, percentile and median
of its own: the reference for the FLOAT outputs of xm_pair_filter (scale1, scale2, translation, median, p95).  The f64 restatement's
difference from it is e_ref of the project's bound e_gpu <= max(16 e_ref, 64 eps)."""
import numpy as np

import xm_pair_numpy as pn

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


class Exact:
    dtype = LD

    @staticmethod
    def tmean(a, trim):
        a = np.sort(np.asarray(a, dtype=LD), axis=-1)
        k = a.shape[-1]
        lo = int(trim * k)
        return a[..., lo:k - lo].sum(axis=-1) / LD(k - 2 * lo)

    @staticmethod
    def pct(a, q):
        a = np.sort(np.asarray(a, dtype=LD))
        pos = LD(a.size - 1) * LD(q) / LD(100)
        i0 = int(np.floor(pos)); i1 = min(i0 + 1, a.size - 1)
        return a[i0] + (a[i1] - a[i0]) * (pos - LD(i0))

    @staticmethod
    def median(a):
        a = np.sort(np.asarray(a, dtype=LD))
        k = a.size
        return a[k // 2] if k % 2 else (a[k // 2 - 1] + a[k // 2]) / LD(2)


def pair_filter_exact(*args, **kw):
    return pn.pair_filter_numpy(*args, ops=Exact, **kw)


def bound(e_ref):
    return max(16.0 * e_ref, 64.0 * EPS)


def float_errors(stats, exact):
    """per float quantity, the largest relative error over the used pairs of `stats` (a structured array) against `exact` (what
    pair_filter_exact returned).  The denominator is the exact value, but not less than the magnitude of the terms the quantity is formed
    from where those cancel: the largest |coordinate| of dst for the translation (a mean of dst - R src), that over scale1 for median and
    p95 (order statistics of |R src + t - dst| / scale1)."""
    used = exact["stats"]["status"] == pn.USED
    fl = exact["floats"]
    out = {}
    for f in pn.FLOATS:
        x = np.asarray(stats[f], dtype=LD)[used]; xe = fl[f][used]
        if f == "translation":
            den = np.maximum(np.abs(xe).max(axis=1), exact["dst_max"][used]); num = np.abs(x - xe).max(axis=1)
        elif f in ("median", "p95"):
            den = np.maximum(np.abs(xe), exact["dst_max"][used] / fl["scale1"][used]); num = np.abs(x - xe)
        else:
            den = np.abs(xe); num = np.abs(x - xe)
        out[f] = float((num / den).max()) if num.size else 0.0
    return out
