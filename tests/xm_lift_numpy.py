"""The depth lift (include/xm_amd.h: xm_lift_observations) restated in numpy, the case builders of the lift's tests, and the literal float32
variant of the reference's percentile that the margin check uses.

lift_numpy follows the header's nine steps in f64 where the header says f64; lift_numpy(..., f32_rule=True) hands np.percentile the float32
samples as the reference's script does (5_test_ceres.py:273).  Every case the GPU tests use has depths on a 2^-10 grid in [0.5, 8), where
the two rules keep the same rows (tests/test_lift_numpy.py checks that for each of them)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lift")
CASES = ("a", "b")
INFO_FIELDS = ("rows_duplicate", "rows_border", "rows_depth", "rows_no_map", "cams_no_map", "cams_empty", "cams_small", "cams_large",
               "cams_workspace", "max_rows")
EPS = 2.0 ** -53


def percentile_f64(d, pct):
    """numpy's default percentile of the float32 samples d, in f64 on the widened samples (the header's step 4)"""
    s = np.sort(d.astype(np.float64))
    if np.isnan(s).any():
        return np.nan
    k = s.size
    pos = (k - 1) * (pct / 100.0)
    fl = np.floor(pos); t = pos - fl
    i0 = int(fl); i1 = min(i0 + 1, k - 1)
    a, b = s[i0], s[i1]
    diff = b - a
    thr = b - diff * (1.0 - t) if t >= 0.5 else a + diff * t
    return np.nan if np.isnan(thr) else float(thr)


def lift_numpy(cam, lm, xy, depth, conf, K, n=None, m=None, margin=10, depth_pct=95.0, f32_rule=False, limits=None):
    """-> dict(cam, lm, p, w, row, threshold, info, p_bound): the header's definition.  depth / conf: per camera None or a 2-D float32 array
    (conf may be None altogether).  limits (xmamd.lift_limits()): fills the cams_small / cams_large / cams_workspace counters."""
    cam = np.asarray(cam, dtype=np.int64); lm = np.asarray(lm, dtype=np.int64); xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(depth) if n is None else n
    nr = cam.size
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float64)) if n else np.zeros((0, 3, 3))
    order = np.lexsort((np.arange(nr), lm, cam))                       # 1. by camera, track, input row: the first of a group stays
    sc, sl = cam[order], lm[order]
    first = np.ones(nr, dtype=bool)
    first[1:] = (sc[1:] != sc[:-1]) | (sl[1:] != sl[:-1])
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["rows_duplicate"] = int((~first).sum())
    rows_all = order[first]
    cam_of = cam[rows_all]
    per_cam = np.bincount(cam, minlength=n) if nr else np.zeros(n, dtype=np.int64)
    info["max_rows"] = int(per_cam.max()) if n else 0
    if limits is not None:
        info["cams_small"] = int(((per_cam > 0) & (per_cam <= limits["small_rows"])).sum())
        info["cams_large"] = int(((per_cam > limits["small_rows"]) & (per_cam <= limits["lds_rows"])).sum())
        info["cams_workspace"] = int((per_cam > limits["lds_rows"]).sum())
    uv = np.trunc(xy).astype(np.int64)                                 # 2. toward zero
    out = dict(cam=[], lm=[], p=[], w=[], row=[], p_bound=[])
    thr_all = np.full(n, np.nan)
    for c in range(n):
        lo, hi = np.searchsorted(cam_of, (c, c + 1))
        rows = rows_all[lo:hi]                                         # in track order
        if depth[c] is None:
            info["cams_no_map"] += 1; info["rows_no_map"] += rows.size
            continue
        D = depth[c]; h, w = D.shape
        u, v = uv[rows, 0], uv[rows, 1]
        ok = (u >= margin) & (u < w - margin) & (v >= margin) & (v < h - margin)
        info["rows_border"] += int((~ok).sum())
        rows, u, v = rows[ok], u[ok], v[ok]
        if rows.size == 0:
            info["cams_empty"] += 1
            continue
        d = D[v, u]                                                    # 3. float32
        if f32_rule:
            with np.errstate(invalid="ignore"):
                thr = np.percentile(d, depth_pct)
            keep = (d > 0) & (d < thr)
        else:
            thr = percentile_f64(d, depth_pct)                         # 4.
            keep = (d > 0) & (d.astype(np.float64) < thr)              # 5., 6.
        thr_all[c] = np.nan if np.isnan(thr) else float(thr)
        info["rows_depth"] += int((~keep).sum())
        rows, u, v, d = rows[keep], u[keep], v[keep], d[keep].astype(np.float64)
        if rows.size == 0:
            info["cams_empty"] += 1
            continue
        cf = np.ones(rows.size, dtype=np.float32) if conf is None or conf[c] is None else conf[c][v, u]
        ki = Kinv[c]
        uf, vf = u.astype(np.float64), v.astype(np.float64)
        ray = np.stack([(ki[a, 0] * uf + ki[a, 1] * vf) + ki[a, 2] for a in range(3)], axis=1)        # 8.
        mag = np.stack([np.abs(ki[a, 0]) * np.abs(uf) + np.abs(ki[a, 1]) * np.abs(vf) + np.abs(ki[a, 2]) for a in range(3)], axis=1)
        out["cam"].append(np.full(rows.size, c)); out["lm"].append(lm[rows]); out["row"].append(rows)
        out["p"].append(ray * d[:, None]); out["p_bound"].append(8.0 * EPS * mag * np.abs(d)[:, None])
        out["w"].append((cf * cf).astype(np.float64))                  # 7. the float32 product, widened
    cat = lambda k, shape, dt: np.concatenate(out[k]).astype(dt) if out[k] else np.zeros(shape, dtype=dt)
    return dict(cam=cat("cam", 0, np.int32), lm=cat("lm", 0, np.int32), row=cat("row", 0, np.int32), p=cat("p", (0, 3), np.float64),
                p_bound=cat("p_bound", (0, 3), np.float64), w=cat("w", 0, np.float64), threshold=thr_all, info=info)


# ------------------------------------------------------------------------------------------------ case builders
def grid_depth(rng, h, w):
    """depths on the 2^-10 grid in [0.5, 8)"""
    return (rng.integers(512, 8192, (h, w)) / 1024.0).astype(np.float32)


def intrinsics(n, hw):
    K = np.zeros((n, 3, 3))
    for c in range(n):
        f = 40.0 + 3.0 * c
        K[c] = [[f, 0.0, hw[c][1] / 2.0], [0.0, f * 1.0625, hw[c][0] / 2.0], [0.0, 0.0, 1.0]]
    return K


def scene(sizes, seed, hw=(48, 64), margin=10, outside=0.0, twins=0.0, shuffle=True, no_map=(), with_conf=True):
    """one camera per entry of sizes with that many rows of distinct tracks; `outside`: the share of a camera's rows put outside the border;
    `twins`: the share of a camera's rows that get a second row of the same track at another pixel (so the camera has more rows than its
    entry says).  Pixels are drawn inside the border with replacement, so several tracks may share one.  -> dict of lift arguments"""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    hws = [hw] * n if isinstance(hw[0], int) else list(hw)
    m = max(max(sizes), 1) + 7
    cam, lm, xy = [], [], []
    depth, conf = [], []
    for c, k in enumerate(sizes):
        h, w = hws[c]
        depth.append(None if c in no_map else grid_depth(rng, h, w))
        conf.append(None if c in no_map else rng.uniform(0.05, 1.0, (h, w)).astype(np.float32))
        tracks = rng.permutation(m)[:k]
        x = rng.integers(margin, w - margin, k) + rng.uniform(0.0, 0.99, k)
        y = rng.integers(margin, h - margin, k) + rng.uniform(0.0, 0.99, k)
        out = rng.random(k) < outside
        x[out] = rng.choice([margin - 1 + 0.9, w - margin + 0.1], int(out.sum()))
        cam.append(np.full(k, c)); lm.append(tracks); xy.append(np.stack([x, y], axis=1))
        tw = np.flatnonzero(rng.random(k) < twins)
        if tw.size:
            x2 = rng.integers(margin, w - margin, tw.size) + 0.5; y2 = rng.integers(margin, h - margin, tw.size) + 0.5
            cam.append(np.full(tw.size, c)); lm.append(tracks[tw]); xy.append(np.stack([x2, y2], axis=1))
    cam = np.concatenate(cam).astype(np.int32) if cam else np.zeros(0, np.int32)
    lm = np.concatenate(lm).astype(np.int32) if lm else np.zeros(0, np.int32)
    xy = np.concatenate(xy) if xy else np.zeros((0, 2))
    if shuffle:
        perm = rng.permutation(cam.size)
        cam, lm, xy = cam[perm], lm[perm], xy[perm]
    return dict(cam=cam, lm=lm, xy=xy, depth=depth, conf=conf if with_conf else None, K=intrinsics(n, hws), n=n, m=m, margin=margin, depth_pct=95.0)


def size_cases(limits):
    """camera sizes at which the code takes another path: the percentile position is integral at 21 and 41 rows, a wavefront has 64 lanes,
    and xm_lift_limits() names the workgroup size and the two limits"""
    T, S, L = limits["threads"], limits["small_rows"], limits["lds_rows"]
    small = sorted({0, 1, 2, 20, 21, 41, 63, 64, 65, T - 1, T, T + 1, S - 1, S, S + 1})
    return dict(small=scene(small, 11), tiers=scene([L - 1, L, L + 1, S + 1, 2 * L + 1, 3], 12))


def degenerate_case():
    """cameras 0 and 5 without a map, camera 1 with every row outside the border, camera 2 with one depth everywhere, camera 3 with zeros
    and negatives among its depths, camera 4 with one NaN, camera 6 with no row at all, camera 7 ordinary"""
    c = scene([30, 25, 40, 50, 35, 12, 0, 60], 21, no_map=(0, 5))
    in1 = c["cam"] == 1
    c["xy"][in1, 0] = np.where(np.arange(int(in1.sum())) % 2 == 0, 3.5, 60.25)
    c["depth"][2][:] = np.float32(2.5)
    rng = np.random.default_rng(5)
    d3 = c["depth"][3]
    d3[rng.random(d3.shape) < 0.2] = 0.0
    d3[rng.random(d3.shape) < 0.2] = -1.5
    r4 = int(np.flatnonzero(c["cam"] == 4)[7])
    c["depth"][4][int(c["xy"][r4, 1]), int(c["xy"][r4, 0])] = np.nan
    return c


def border_case(margin):
    """pixels exactly on both sides of each of the four borders (and, with margin 0, x = -0.5, which truncates to 0 and passes), in maps of
    different, non-square sizes; a handful of ordinary rows so that the percentile has something to work on"""
    hws = [(48, 64), (33, 47), (40, 29)]
    c = scene([24, 24, 24], 31 + margin, hw=hws, margin=margin)
    cam, lm, xy = [c["cam"]], [c["lm"]], [c["xy"]]
    for i, (h, w) in enumerate(hws):
        xs = [margin - 1, margin, w - margin - 1, w - margin]
        ys = [margin - 1, margin, h - margin - 1, h - margin]
        at = lambda q: q + 0.75 if q >= 0 else q - 0.25          # inside pixel q (truncation is toward zero: -0.25 would be pixel 0)
        pts = [(at(x), h / 2.0) for x in xs] + [(w / 2.0, at(y)) for y in ys] + [(margin - 0.5, h / 2.0), (w / 2.0, margin - 0.5)]
        cam.append(np.full(len(pts), i, dtype=np.int32)); lm.append(np.arange(len(pts), dtype=np.int32) + c["m"]); xy.append(np.array(pts))
    c.update(cam=np.concatenate(cam), lm=np.concatenate(lm), xy=np.concatenate(xy), m=c["m"] + 10)
    return c


def duplicate_case():
    """twins and triples; track 900 of camera 0: the first row is outside the border, the second inside (the first stays, and is then
    dropped); track 901 of camera 1: two rows at the two ends of the input"""
    c = scene([50, 70, 90], 41, twins=0.3, shuffle=True)
    rng = np.random.default_rng(42)
    t = np.flatnonzero(c["cam"] == 2)[:9]                                       # triples: a third row for nine tracks of camera 2
    extra_cam = [np.full(9, 2)]; extra_lm = [c["lm"][t]]; extra_xy = [np.stack([rng.integers(10, 54, 9) + 0.25, rng.integers(10, 38, 9) + 0.25], axis=1)]
    extra_cam.append(np.array([0, 0])); extra_lm.append(np.array([900, 900])); extra_xy.append(np.array([[2.5, 20.5], [30.5, 20.5]]))
    cam = np.concatenate([[1], c["cam"]] + extra_cam + [[1]]).astype(np.int32)
    lm = np.concatenate([[901], c["lm"]] + extra_lm + [[901]]).astype(np.int32)
    xy = np.concatenate([[[20.5, 15.5]], c["xy"]] + extra_xy + [[[40.5, 30.5]]])
    c.update(cam=cam, lm=lm, xy=xy, m=902)
    return c


def gpu_cases(limits):
    """every case the GPU tests compare with lift_numpy, by name"""
    out = size_cases(limits)
    out.update(degenerate=degenerate_case(), border10=border_case(10), border0=border_case(0), duplicates=duplicate_case(),
               no_conf=scene([33, 80], 51, with_conf=False), mixed=scene([120, 7, 300, 64], 52, outside=0.15, twins=0.1))
    return out


def call_args(c):
    return (c["cam"], c["lm"], c["xy"], c["depth"], c["conf"], c["K"]), dict(n=c["n"], m=c["m"], margin=c["margin"], depth_pct=c["depth_pct"])


def run_numpy(c, **kw):
    a, k = call_args(c)
    k.update(kw)
    return lift_numpy(*a, **k)


def load_case(name):
    """tests/golden/lift/<name>.npz -> (the lift arguments, the recorded outputs of the reference's own lines)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = int(z["n"])
    has = z["has_map"].astype(bool)
    hw = z["hw"]
    depth, conf, o = [], [], 0
    for c in range(n):
        if not has[c]:
            depth.append(None); conf.append(None)
            continue
        h, w = int(hw[c, 0]), int(hw[c, 1])
        depth.append(z["depth"][o:o + h * w].reshape(h, w).copy()); conf.append(z["conf"][o:o + h * w].reshape(h, w).copy())
        o += h * w
    c = dict(cam=z["cam"].astype(np.int32), lm=z["lm"].astype(np.int32), xy=z["xy"], depth=depth, conf=conf, K=z["K"], n=n, m=int(z["m"]), margin=10,
             depth_pct=95.0)
    ref = dict(cam=z["ref_cam"].astype(np.int32), lm=z["ref_lm"].astype(np.int32), row=z["ref_row"].astype(np.int32), p=z["ref_p"], w=z["ref_w"],
               rows_duplicate=int(z["ref_rows_duplicate"]))
    return c, ref
