"""Predicted boxes on the camera views and a top-down panel (toc3d_amd.BoxVis, include/toc3d_boxes.h): the cases and the restatements that the CPU and GPU tests
compare with -- corners, projection, near-plane and rectangle clipping in FLOAT64 (with the margin of every decision, so that a test can leave out what float32
may decide the other way, and the error bound of an untouched end); coverage and the winner rule in numpy integers; the base bytes through the restatement of
tests/token_vis_cases.py.  The corners are held to tests/golden/box_vis_cases.npz, which tools/gen_golden_box_vis.py makes with the reference's own
``LiDARInstance3DBoxes.corners`` (lidar_box3d.py:50-90) and ``rotation_3d_in_axis`` (structures/utils.py:79-106), and to a hand-computed box, by
tests/test_cpu_box_vis.py.  Importing this module needs no GPU."""
import os

import numpy as np

import token_vis_cases as TC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_vis_cases.npz")
U = 2.0 ** -24                               # float32 unit roundoff
EDGES = ((0, 1), (0, 3), (0, 4), (1, 2), (1, 5), (3, 2), (3, 7), (4, 5), (4, 7), (2, 6), (5, 6), (6, 7))             # image_vis.py:77
OFFSETS = np.array([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)], dtype=np.float64)   # lidar_box3d.py:50-90
BEV_EDGES = ((0, 3), (3, 7), (7, 4), (4, 0))
PALETTE = np.array([(255, 158, 0)] * 5 + [(112, 128, 144)] + [(255, 61, 99)] * 2 + [(0, 0, 230), (47, 79, 79)], dtype=np.uint8)
GUARD, NEAR, THR = 16, 0.1, 0.25
THICKNESSES = (1, 2, 3, 5, 15)


# ---- geometry in float64 ----------------------------------------------------------------------------------------------------------------------------------------
def corners64(boxes):
    """(n, >= 7) -> (n, 8, 3) float64: LiDARInstance3DBoxes.corners."""
    b = np.asarray(boxes, dtype=np.float64)
    local = (OFFSETS[None] - np.array([0.5, 0.5, 0.0])) * b[:, None, 3:6]
    sn, cs = np.sin(b[:, 6])[:, None], np.cos(b[:, 6])[:, None]
    x = local[..., 0] * cs - local[..., 1] * sn
    y = local[..., 0] * sn + local[..., 1] * cs
    return np.stack([x, y, local[..., 2]], axis=-1) + b[:, None, :3]


def corner_error(boxes, corners):
    """|float32 corner - float64 corner| <= this, per coordinate (n, 8, 3).  sincosf within 2 ulp of a value <= 1 (4 U each; HIP documents 1 ulp), the two
    products, the difference and the sum one rounding each: (4 + 4 + 1 + 1 + 1) U on terms bounded by r = (|dx| + |dy|) / 2, taken as 12 U r, plus U |corner| for
    the last sum; z_bottom + dz is one rounding."""
    b = np.abs(np.asarray(boxes, dtype=np.float64))
    r = 0.5 * (b[:, 3] + b[:, 4])[:, None]
    e = np.empty_like(corners)
    e[..., 0] = U * (12 * r + np.abs(corners[..., 0]))
    e[..., 1] = U * (12 * r + np.abs(corners[..., 1]))
    e[..., 2] = U * np.abs(corners[..., 2])
    return e


def _liang_barsky(x0, y0, x1, y1, lo_x, lo_y, hi_x, hi_y):
    """-> (kept, (x0, y0, x1, y1), touched, margin): margin is the smallest distance, in pixels, by which a comparison of the clip was decided."""
    dx, dy = x1 - x0, y1 - y0
    length = max(abs(dx), abs(dy), 1e-300)
    t0, t1, margin = 0.0, 1.0, np.inf
    for p, q in ((-dx, x0 - lo_x), (dx, hi_x - x0), (-dy, y0 - lo_y), (dy, hi_y - y0)):
        if p == 0:
            margin = min(margin, abs(q))
            if q < 0:
                return False, None, True, margin
        else:
            r = q / p
            if p < 0:
                margin = min(margin, abs(r - t1) * length, abs(r - t0) * length)
                if r > t1:
                    return False, None, True, margin
                t0 = max(t0, r)
            else:
                margin = min(margin, abs(r - t0) * length, abs(r - t1) * length)
                if r < t0:
                    return False, None, True, margin
                t1 = min(t1, r)
    ax, ay = (x0 + t0 * dx, y0 + t0 * dy) if t0 > 0 else (x0, y0)
    bx, by = (x0 + t1 * dx, y0 + t1 * dy) if t1 < 1 else (x1, y1)
    clamp = lambda v, lo, hi: min(max(v, lo), hi)
    return True, (clamp(ax, lo_x, hi_x), clamp(ay, lo_y, hi_y), clamp(bx, lo_x, hi_x), clamp(by, lo_y, hi_y)), (t0 > 0 or t1 < 1), margin


def _live(box, score, label, thr, ncol):
    return bool(np.isfinite(np.asarray(box[:7], dtype=np.float64)).all() and not (score < thr) and 0 <= label < ncol)


def camera_segments64(boxes, scores, labels, proj, H, W, thr=THR, ncol=10, near=NEAR, guard=GUARD):
    """The camera tables in float64.  -> dict(segf (V, n, 12, 4), cidx (V, n, 12), touched (V, n, 12) bool: a clip moved an end, or dropped the segment;
    margin (V, n, 12): the smallest decision margin over its own error bound (> 1: float32 decides alike; inf where nothing was decided);
    bound (V, n, 12, 4): the error bound of an end no clip touched, in pixels)."""
    boxes, proj = np.asarray(boxes, dtype=np.float64), np.asarray(proj, dtype=np.float64)
    scores64 = np.asarray(scores, dtype=np.float64)
    V, n = proj.shape[0], boxes.shape[0]
    segf, cidx = np.zeros((V, n, 12, 4)), np.full((V, n, 12), 255, dtype=np.uint8)
    touched, margin, bound = np.zeros((V, n, 12), dtype=bool), np.full((V, n, 12), np.inf), np.zeros((V, n, 12, 4))
    with np.errstate(all="ignore"):
        cor = corners64(boxes)
        cerr = corner_error(boxes, cor)
    lo, hi_x, hi_y = -float(guard), W - 1.0 + guard, H - 1.0 + guard
    for v in range(V):
        P = proj[v]
        for b in range(n):
            live = _live(boxes[b], scores64[b], int(labels[b]), thr, ncol) and bool(np.isfinite(P).all())
            if not live:
                # the score test is a decision too: its margin is exact (the threshold is compared in float32 with a float32 score)
                touched[v, b] = True
                continue
            c1 = np.concatenate([cor[b], np.ones((8, 1))], axis=1)
            h = c1 @ P.T                                                     # (8, 4)
            # |float32 h - float64 h|: the corner errors through |P|, and at most four roundings (a product and three sums) on every term of the row
            A = np.abs(c1) @ np.abs(P).T
            dh = cerr[b] @ np.abs(P[:, :3]).T + 4 * U * A
            for e, (ka, kb) in enumerate(EDGES):
                ha, hb, da, db = h[ka], h[kb], dh[ka], dh[kb]
                m = min(abs(ha[2] - near) / da[2], abs(hb[2] - near) / db[2])
                a_behind, b_behind = ha[2] < near, hb[2] < near
                if a_behind and b_behind:
                    touched[v, b, e], margin[v, b, e] = True, m
                    continue
                clipped = a_behind != b_behind
                if clipped:
                    t = (near - ha[2]) / (hb[2] - ha[2])
                    mid = ha + t * (hb - ha)
                    mid[2] = near
                    if a_behind:
                        ha = mid
                    else:
                        hb = mid
                pa, pb = ha[:2] / ha[2], hb[:2] / hb[2]
                # an end no clip touched: (dhx + |px| dhz) / hz, 5 % for the second order (dhz / hz below 0.04: asserted), one rounding of the quotient
                assert clipped or (da[2] < 0.04 * abs(ha[2]) and db[2] < 0.04 * abs(hb[2])), "a case for another bound: the depth error is no small part of the depth"
                ea = 1.05 * (da[:2] + np.abs(pa) * da[2]) / abs(ha[2]) + U * np.abs(pa)
                eb = 1.05 * (db[:2] + np.abs(pb) * db[2]) / abs(hb[2]) + U * np.abs(pb)
                if clipped:
                    # the interpolated end: about sixteen roundings on quantities bounded by M, t amplified by 1 / |zb - za|, all divided by near: taken as 64 U
                    M = np.abs(h[ka][:3]).sum() + np.abs(h[kb][:3]).sum()
                    amp = 64 * U * M / near * (1 + (abs(h[ka][2]) + abs(h[kb][2])) / abs(h[kb][2] - h[ka][2])) + 16 * (da[:3].sum() + db[:3].sum()) / near
                    ea, eb = (np.full(2, amp), eb) if a_behind else (ea, np.full(2, amp))
                kept, seg, rect_touched, rm = _liang_barsky(pa[0], pa[1], pb[0], pb[1], lo, lo, hi_x, hi_y)
                m = min(m, rm / max(ea.max(), eb.max()))
                margin[v, b, e], touched[v, b, e] = m, clipped or rect_touched or not kept
                bound[v, b, e] = np.concatenate([ea, eb])
                if kept and np.isfinite(seg).all():
                    segf[v, b, e], cidx[v, b, e] = seg, labels[b]
    return dict(segf=segf, cidx=cidx, touched=touched, margin=margin, bound=bound)


def bev_segments64(boxes, scores, labels, S, range_m=51.2, thr=THR, ncol=10, guard=GUARD):
    """The top-down tables in float64 -> dict(segf (n, 5, 4), cidx (n, 5), touched, margin, bound).  Error of an end: the corner's (or the centre's: none), times the
    scale, and three roundings (the scale itself, the product, the difference) on values bounded by S / 2 + |coordinate| scale."""
    boxes = np.asarray(boxes, dtype=np.float64)
    n = boxes.shape[0]
    segf, cidx = np.zeros((n, 5, 4)), np.full((n, 5), 255, dtype=np.uint8)
    touched, margin, bound = np.zeros((n, 5), dtype=bool), np.full((n, 5), np.inf), np.zeros((n, 5, 4))
    scale, half = S / (2.0 * range_m), S / 2.0
    with np.errstate(all="ignore"):
        cor = corners64(boxes)
        cerr = corner_error(boxes, cor)
    for b in range(n):
        if not _live(boxes[b], float(scores[b]), int(labels[b]), thr, ncol):
            touched[b] = True
            continue
        pts = {k: cor[b, k, :2] for k in (0, 3, 7, 4)}
        errs = {k: cerr[b, k, :2] for k in (0, 3, 7, 4)}
        pts["c"], errs["c"] = boxes[b, :2], np.zeros(2)
        pts["m"], errs["m"] = 0.5 * (cor[b, 4, :2] + cor[b, 7, :2]), 0.5 * (cerr[b, 4, :2] + cerr[b, 7, :2]) + U * np.abs(cor[b, 4, :2] + cor[b, 7, :2])
        pix = lambda k: np.array([half - pts[k][1] * scale, half - pts[k][0] * scale])
        perr = lambda k: (errs[k][::-1] * scale + 3 * U * (half + np.abs(pts[k][::-1]) * scale)) * 1.05
        for e, (ka, kb) in enumerate(BEV_EDGES + (("c", "m"),)):
            pa, pb, ea, eb = pix(ka), pix(kb), perr(ka), perr(kb)
            kept, seg, rect_touched, rm = _liang_barsky(pa[0], pa[1], pb[0], pb[1], -float(guard), -float(guard), S - 1.0 + guard, S - 1.0 + guard)
            margin[b, e], touched[b, e] = rm / max(ea.max(), eb.max()), rect_touched or not kept
            bound[b, e] = np.concatenate([ea, eb])
            if kept:
                segf[b, e], cidx[b, e] = seg, labels[b]
    return dict(segf=segf, cidx=cidx, touched=touched, margin=margin, bound=bound)


# ---- coverage and the winner, in integers ------------------------------------------------------------------------------------------------------------------------
def coverage(H, W, seg, t, window=None):
    """bool (H, W) (or the window (y0, y1, x0, x1) of it): the pixels segment (x0, y0, x1, y1) covers at thickness t, by the rule of include/toc3d_boxes.h in int64."""
    ya, yb, xa, xb = (0, H, 0, W) if window is None else window
    x0, y0, x1, y1 = (int(c) for c in seg)
    py, px = np.meshgrid(np.arange(ya, yb, dtype=np.int64), np.arange(xa, xb, dtype=np.int64), indexing="ij")
    dx, dy, qx, qy = x1 - x0, y1 - y0, px - x0, py - y0
    dd, u, tt = dx * dx + dy * dy, qx * dx + qy * dy, t * t
    cap0 = 4 * (qx * qx + qy * qy) <= tt
    rx, ry = qx - dx, qy - dy
    cap1 = 4 * (rx * rx + ry * ry) <= tt
    c = qx * dy - qy * dx
    body = 4 * c * c <= tt * dd
    return np.where((dd == 0) | (u <= 0), cap0, np.where(u >= dd, cap1, body))


def distance_coverage(H, W, seg, t):
    """Brute force in float64: (covered (H, W), the smallest |distance - t/2| over the pixels)."""
    x0, y0, x1, y1 = (float(c) for c in seg)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dx, dy = x1 - x0, y1 - y0
    dd = dx * dx + dy * dy
    s = np.zeros_like(px) if dd == 0 else np.clip(((px - x0) * dx + (py - y0) * dy) / dd, 0.0, 1.0)
    dist = np.hypot(px - (x0 + s * dx), py - (y0 + s * dy))
    return dist <= t / 2.0, float(np.abs(dist - t / 2.0).min())


def render_restated(base, segi, cidx, palette, t, guard=GUARD):
    """base uint8 (V, H, W, 3), red first; segi (V, S, 4) integers; cidx (V, S) -> uint8 (V, H, W, 3).  Painted from the last segment to the first, so the smallest
    covering index ends on top; cidx >= len(palette) and a segment with an end outside the guarded rectangle are not drawn."""
    out = np.array(base, dtype=np.uint8, copy=True)
    V, H, W, _ = out.shape
    segi, cidx = np.asarray(segi).reshape(V, -1, 4).astype(np.int64), np.asarray(cidx).reshape(V, -1)
    g = (t + 1) // 2
    for v in range(V):
        for s in range(segi.shape[1] - 1, -1, -1):
            if cidx[v, s] >= len(palette):
                continue
            x0, y0, x1, y1 = segi[v, s]
            if min(x0, x1) < -guard or max(x0, x1) > W - 1 + guard or min(y0, y1) < -guard or max(y0, y1) > H - 1 + guard:
                continue
            win = (max(0, min(y0, y1) - g), min(H, max(y0, y1) + g + 1), max(0, min(x0, x1) - g), min(W, max(x0, x1) + g + 1))
            if win[0] >= win[1] or win[2] >= win[3]:
                continue
            cov = coverage(H, W, segi[v, s], t, win)
            out[v, win[0]:win[1], win[2]:win[3]][cov] = palette[cidx[v, s]]
    return out


def coloured(out, base):
    """bool (V, H, W): pixels whose bytes are not the base's."""
    return (out != base).any(axis=-1)


def within_one_pixel(a, b):
    """Every pixel set in a and not in b has a pixel of b in its 3 x 3 neighbourhood, and the other way round -> the number of pixels that do not."""
    def grown(m):
        p = np.pad(m, [(0, 0), (1, 1), (1, 1)])
        return np.max([p[:, i:i + m.shape[1], j:j + m.shape[2]] for i in range(3) for j in range(3)], axis=0).astype(bool)
    return int((a & ~grown(b)).sum() + (b & ~grown(a)).sum())


# ---- the base bytes: TokenVis's image byte, red first -----------------------------------------------------------------------------------------------------------------
def base_f32(img, norm):
    """float32 (V, 3, H, W), img_norm_cfg or None -> uint8 (V, H, W, 3) red first: tests/token_vis_cases.py's denormalisation, reversed where to_rgb is false."""
    pics = []
    for v in range(img.shape[0]):
        pic = np.ascontiguousarray(img[v].transpose(1, 2, 0))
        if norm is not None:
            pic = TC.imdenormalize(pic, norm["mean"], norm["std"], to_bgr=False)
        with np.errstate(invalid="ignore"):
            pics.append(TC.to_bytes(np.nan_to_num(pic, nan=0.0, posinf=np.inf, neginf=-np.inf)))
    out = np.stack(pics)
    return out if (norm is not None and norm["to_rgb"]) else np.ascontiguousarray(out[..., ::-1])


def base_u8(raw):
    """uint8 (V, H, W, 3) raw frames (blue first, as cv2.imread gives them) -> red first."""
    return np.ascontiguousarray(raw[..., ::-1])


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------------------------
def pinhole(f, cx, cy, yaw_deg=0.0, pitch_deg=0.0, t=(0.0, 0.0, 0.0)):
    """lidar2img (4, 4) float32 of a camera at lidar position t that looks along +x turned by yaw about z (and pitched): camera axes (right, down, forward)."""
    a, p = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    fwd = np.array([np.cos(a) * np.cos(p), np.sin(a) * np.cos(p), np.sin(p)])
    right = np.array([np.sin(a), -np.cos(a), 0.0])
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ np.asarray(t, dtype=np.float64)
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = cx, cy
    return (K @ E).astype(np.float32)


GEOM_HW = (48, 80)
# name -> boxes (n, 9) float32, scores, labels; two views each: a pinhole along +x and a rotated, pitched, displaced one
_HAND = np.array([
    [12.0, 0.5, -1.0, 4.0, 1.8, 1.5, 0.3, 0, 0],          # fully in view 0
    [0.5, 0.3, -0.5, 4.0, 2.0, 1.5, 0.2, 0, 0],           # straddles view 0's near plane
    [-10.0, 0.0, -1.0, 4.0, 1.8, 1.5, 1.0, 0, 0],         # wholly behind view 0
    [6.0, 4.5, -1.0, 4.2, 1.9, 1.6, -0.4, 0, 0],          # partly outside view 0's rectangle
    [5.0, 20.0, -1.0, 4.0, 1.8, 1.5, 0.1, 0, 0],          # in front of view 0, wholly outside its rectangle
    [14.0, -1.0, -1.0, 0.8, 0.8, 1.8, 2.0, 0, 0],         # below the score threshold
    [15.0, 2.0, -1.0, 0.5, 0.5, 1.0, 0.0, 0, 0],          # a label out of range
    [13.0, 1.0, -1.0, np.nan, 1.8, 1.5, 0.3, 0, 0],       # a NaN box
    [9.0, -2.5, -1.2, 2.0, 0.9, 1.7, -2.6, 0, 0],         # fully in view 0, another class
], dtype=np.float32)


def geometry_case(name):
    """-> dict(boxes, scores, labels, proj (2, 4, 4), H, W)."""
    H, W = GEOM_HW
    proj = np.stack([pinhole(45.0, 40.0, 24.0), pinhole(38.0, 41.5, 20.0, yaw_deg=100.0, pitch_deg=-6.0, t=(0.6, 0.4, 0.3))])
    if name == "hand":
        boxes = _HAND.copy()
        scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.1, 0.45, 0.4, 0.3], dtype=np.float32)
        labels = np.array([0, 8, 3, 6, 5, 8, 10, 1, 9], dtype=np.int64)
    elif name == "empty":
        boxes, scores, labels = np.zeros((0, 9), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    else:
        rng = np.random.default_rng(dict(random_a=5101, random_b=5102)[name])
        n = 8
        boxes = np.zeros((n, 9), dtype=np.float32)
        boxes[:, 0:2] = rng.uniform(-18, 18, (n, 2))
        boxes[:, 2] = rng.uniform(-2.5, 0.0, n)
        boxes[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
        boxes[:, 6] = rng.uniform(-np.pi, np.pi, n)
        scores = np.sort(rng.uniform(0.2, 1.0, n).astype(np.float32))[::-1].copy()
        labels = rng.integers(-1, 11, n).astype(np.int64)
    return dict(boxes=boxes, scores=scores, labels=labels, proj=proj, H=H, W=W)


GEOMETRY_CASES = ("hand", "random_a", "random_b", "empty")
BEV_S, BEV_RANGE = 96, 20.0


def big_case(seed=5200, n=300, V=6, H=320, W=800):
    """300 boxes at the shipped pc_range, six views around the vehicle."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((n, 9), dtype=np.float32)
    boxes[:, 0:2] = rng.uniform(-51.2, 51.2, (n, 2))
    boxes[:, 2] = rng.uniform(-5.0, 1.0, n)
    boxes[:, 3:6] = rng.uniform(0.4, 8.0, (n, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, n)
    scores = np.sort(rng.uniform(0.05, 1.0, n).astype(np.float32))[::-1].copy()
    labels = rng.integers(0, 10, n).astype(np.int64)
    proj = np.stack([pinhole(500.0, W / 2.0, H / 2.0, yaw_deg=60.0 * v, pitch_deg=-2.0, t=(1.0 * np.cos(v), 0.5 * np.sin(v), 1.5)) for v in range(V)])
    img = rng.uniform(-2.2, 2.6, (V, 3, H, W)).astype(np.float32)
    return dict(boxes=boxes, scores=scores, labels=labels, proj=proj, img=img, H=H, W=W)


def render_case(name):
    """Hand-made and random segment tables for the exact render tests -> dict(H, W, segi (2, S, 4) int32, cidx (2, S) uint8)."""
    H, W = dict(odd=(40, 70), w4=(36, 72), empty=(40, 70), random=(40, 70))[name]
    if name == "empty":
        return dict(H=H, W=W, segi=np.zeros((2, 0, 4), np.int32), cidx=np.zeros((2, 0), np.uint8))
    if name == "random":
        rng = np.random.default_rng(5300)
        S = 40
        segi = np.stack([rng.integers(-GUARD, W + GUARD, (2, S)), rng.integers(-GUARD, H + GUARD, (2, S)),
                         rng.integers(-GUARD, W + GUARD, (2, S)), rng.integers(-GUARD, H + GUARD, (2, S))], axis=-1).astype(np.int32)
        cidx = rng.integers(0, 10, (2, S)).astype(np.uint8)
        cidx[:, ::5] = 255
        cidx[1, 3] = 200                                                    # beyond the palette, not 255: not drawn either
        return dict(H=H, W=W, segi=segi, cidx=cidx)
    X, Y = W - 1, H - 1
    hand = [
        (5, 5, 5, 5, 0), (20, 8, 20, 8, 8),                                 # zero length
        (2, 12, 60, 12, 5), (33, 2, 33, 37, 6),                             # horizontal, vertical (they cross: the smaller index on top)
        (4, 30, 50, 6, 8), (10, 3, 44, 35, 9),                              # diagonals
        (0, 0, X, 0, 0), (0, Y, X, Y, 5), (0, 0, 0, Y, 6), (X, 0, X, Y, 8),     # on every border
        (-GUARD, 20, 10, 20, 9), (W - 6, 25, X + GUARD, 25, 0), (50, -GUARD, 50, 6, 5), (12, Y - 5, 12, Y + GUARD, 6),     # beyond every border, up to the guard
        (-GUARD, -GUARD, 14, 14, 8), (X + GUARD, Y + GUARD, X - 12, Y - 12, 9),     # through the corners
        (-8, -3, -2, -1, 0), (X + 3, 10, X + 9, 30, 5),                     # wholly in the guard band: only a thick stroke reaches the image
        (24, 18, 40, 18, 255), (24, 20, 40, 20, 0), (24, 20, 40, 20, 8), (30, 14, 30, 26, 255), (30, 14, 30, 26, 6),      # 255 entries interleaved, overlaps
        (-GUARD - 1, 5, 20, 5, 0), (3, 3, X + GUARD + 1, 9, 5),             # an end beyond the guard: not drawn
        (60, 30, 66, 36, 8), (63, 14, 68, 17, 9),                           # across the tile boundary at x = 64 / y = 16, 32
    ]
    rev = [(x1, y1, x0, y0, c) for x0, y0, x1, y1, c in reversed(hand)]     # the other view: the same segments in the other index order, ends swapped
    a = np.array([hand, rev], dtype=np.int64)
    return dict(H=H, W=W, segi=a[..., :4].astype(np.int32), cidx=a[..., 4].astype(np.uint8))


RENDER_CASES = ("odd", "w4", "random", "empty")


def render_sources(H, W, seed):
    """The three source forms of a render case, V = 2: f32 with values beyond the byte range (and a NaN), raw u8 frames, none."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-3.5, 3.5, (2, 3, H, W)).astype(np.float32)
    img[0, :, 0, :4] = np.float32([-1e30, 1e30, np.nan, -0.0])[None]
    raw = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    return img, raw
