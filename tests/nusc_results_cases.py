"""Cases and the float64 restatement for toc3d_boxes_to_global / toc3d_amd.NuScenesResults (include/toc3d_results.h).  A plain module: importing it needs no GPU.

THE RESTATEMENT (:func:`restate`) is written from the reference's lines, not from the kernel: mmdet3d/datasets/nuscenes_dataset.py:576-619 (output_to_nusc_box:
gravity centre, dims [1, 0, 2], Quaternion(axis=[0, 0, 1], radians=yaw), velocity (vx, vy, 0)), :622-657 (lidar_nusc_box_to_global: rotate, translate, the range
test on the ego-frame radius, rotate, translate), :327-346 (the attribute branch on the global speed) and nuscenes' Box.rotate / Box.translate (centre and velocity
through the rotation matrix, orientation multiplied from the left).  It runs box by box on Python floats -- float64, every operation rounded once -- with math.sin
and math.cos.  THE REFERENCE'S OWN FUNCTIONS CANNOT MAKE THIS FIXTURE: they need pyquaternion and the nuScenes devkit, and neither is installed where the fixture
was generated (tools/gen_golden_nusc_results.py tries the import first and says which route it took).  So that the restatement is not its own judge it has a
second, independent rotation route: ``route="sandwich"`` turns every vector with q v q* (two Hamilton products) where ``route="matrix"`` uses the rotation matrix,
and tests/test_cpu_nusc_results.py holds the two together.

THE BOUND of a record element against the restatement, u = 2^-53 (:func:`restate` returns it as ``bound``; written down before the first run on a device):
* a rotation-matrix entry is at most five roundings of magnitudes <= 1 away from the true one on either side: 10 u between the two;
* R c + t: three products and three sums of terms |R_ij c_j| <= |c_j| and t_i, at most 4 u (S + |t_i|) a side with S = |c_0| + |c_1| + |c_2|, plus the entries'
  10 u S: e_i = 18 u S + 8 u |t_i|.  The second pose sees the first's error through |R_ij| <= 1: e'_i = (e_0 + e_1 + e_2) + 18 u S' + 8 u |t'_i|;
* the velocity likewise without a translation: 18 u V, then (sum of those) + 18 u V';
* the orientation: q0 = (cos, 0, 0, sin) is off by the device's sin/cos error E (against math.sin / math.cos on the same float64 half angle); the first product
  has two terms of magnitude <= 1 a component: 2 E from q0, and two products and a sum, 4 u a side, e = 2 E + 8 u.  The second has four terms a component: it sees
  e through the pose's components, whose magnitudes sum to at most 2 (the L1 norm of a unit quaternion), and adds four products and three sums on terms whose
  magnitudes sum to at most 1, 5 u a side: 2 e + 10 u = 4 E + 26 u.  E is not documented on the machines the tests run on, so the GPU test measures that one figure on the
  fixture's own angles with identity poses and says so;
* the size is the float32 value promoted: exact; so is the score.
Decisions (range, speed) are exact because every box of the fixture keeps |radius - range| and |speed - 0.2| above 1e-6, which the CPU test asserts.
"""
import math
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nusc_results_cases.npz")
U = 2.0 ** -53
SPEED_THR = 0.2
MARGIN = 1e-6

# the class order of the shipped configs, and the reference's tables (mmdet3d/datasets/nuscenes_dataset.py:72-103)
CLASS_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked", "truck": "vehicle.parked", "bus": "vehicle.moving",
                     "motorcycle": "cycle.without_rider", "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "", "traffic_cone": ""}
ATTR_REV = ["cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing", "pedestrian.sitting_lying_down", "vehicle.moving",
            "vehicle.parked", "vehicle.stopped"]
# detection_cvpr_2019.json: class_range
CVPR_2019_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40, "bicycle": 40,
                   "traffic_cone": 30, "barrier": 30}
IDENTITY_POSE = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
OUT_KEYS = ("rec", "score", "name", "attr", "src", "kept")


def reference_attribute(name, moving):
    """:327-346, as written there."""
    if moving:
        if name in ["car", "construction_vehicle", "bus", "truck", "trailer"]:
            return "vehicle.moving"
        elif name in ["bicycle", "motorcycle"]:
            return "cycle.with_rider"
        return DEFAULT_ATTRIBUTE[name]
    if name in ["pedestrian"]:
        return "pedestrian.standing"
    elif name in ["bus"]:
        return "vehicle.stopped"
    return DEFAULT_ATTRIBUTE[name]


def tables(class_names=CLASS_NAMES, max_depth=60, class_range=CVPR_2019_RANGE):
    """-> (class_range float64, attr_moving int32, attr_still int32), -1 the empty attribute."""
    idx = lambda a: ATTR_REV.index(a) if a else -1
    rng = np.array([min(class_range[n], max_depth) for n in class_names], dtype=np.float64)
    mov = np.array([idx(reference_attribute(n, True)) for n in class_names], dtype=np.int32)
    still = np.array([idx(reference_attribute(n, False)) for n in class_names], dtype=np.int32)
    return rng, mov, still


# ---- float64 on Python floats --------------------------------------------------------------------------------------------------------------------------------------
def qmul(a, b):
    """The Hamilton product a (x) b."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (((aw * bw - ax * bx) - ay * by) - az * bz, ((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by - ax * bz) + ay * bw) + az * bx,
            ((aw * bz + ax * by) - ay * bx) + az * bw)


def rotation_matrix(q):
    w, x, y, z = q
    return ((1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)),
            (2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)),
            (2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)))


def turn(q, v, route):
    """v turned by the unit quaternion q: through the rotation matrix, or as the sandwich q v q*."""
    if route == "matrix":
        R = rotation_matrix(q)
        return tuple((R[i][0] * v[0] + R[i][1] * v[1]) + R[i][2] * v[2] for i in range(3))
    w, x, y, z = q
    return qmul(qmul(q, (0.0, v[0], v[1], v[2])), (w, -x, -y, -z))[1:]


def restate(boxes, scores, labels, counts, poses, with_velocity=True, class_names=CLASS_NAMES, max_depth=60, speed_thr=SPEED_THR, route="matrix"):
    """``boxes`` float32 (B, K, >= 7 / 9), ``scores`` float32 (B, K), ``labels`` int64 (B, K), ``counts`` (B,), ``poses`` float64 (B, 2, 7), unit quaternions.
    -> dict(rec, score, name, attr, src, kept: what the entry point writes; bound (B, K, 12): the module docstring's, without the 4 E of the orientation;
    radius, limit, speed (B, K): of every valid input row, NaN elsewhere, for the margin checks; half (B, K): the float64 half angles of the kept rows)."""
    rng, mov, still = tables(class_names, max_depth)
    B, K = scores.shape
    out = dict(rec=np.zeros((B, K, 12)), score=np.zeros((B, K), dtype=np.float32), name=np.full((B, K), -1, dtype=np.int32), attr=np.full((B, K), -1, dtype=np.int32),
               src=np.full((B, K), -1, dtype=np.int32), kept=np.zeros(B, dtype=np.int64), bound=np.zeros((B, K, 12)), radius=np.full((B, K), np.nan),
               limit=np.full((B, K), np.nan), speed=np.full((B, K), np.nan), half=np.full((B, K), np.nan))
    used = 9 if with_velocity else 7
    for b in range(B):
        q1, t1, q2, t2 = tuple(map(float, poses[b, 0, :4])), tuple(map(float, poses[b, 0, 4:])), tuple(map(float, poses[b, 1, :4])), tuple(map(float, poses[b, 1, 4:]))
        n = min(max(int(counts[b]), 0), K)
        k = 0
        for i in range(n):
            row, lab = boxes[b, i], int(labels[b, i])
            if not (0 <= lab < len(class_names)) or not np.isfinite(row[:used]).all() or not np.isfinite(scores[b, i]):
                continue
            with np.errstate(over="ignore"):
                zg = np.float32(row[2]) + np.float32(row[5]) * np.float32(0.5)      # float32, as lidar_box3d.py:41-47
            if not np.isfinite(zg):
                continue
            c = (float(row[0]), float(row[1]), float(zg))
            v = (float(row[7]), float(row[8]), 0.0) if with_velocity else (0.0, 0.0, 0.0)
            half = float(row[6]) / 2                                                # np.float32 / 2.0 under NumPy 1.x: float64
            q = (math.cos(half), 0.0, 0.0, math.sin(half))
            s0, v0 = sum(map(abs, c)), sum(map(abs, v))
            # box.rotate(Quaternion(lidar2ego_rotation)); box.translate(lidar2ego_translation)
            c = tuple(r + t for r, t in zip(turn(q1, c, route), t1))
            q = qmul(q1, q)
            v = turn(q1, v, route)
            e1 = [18 * U * s0 + 8 * U * abs(t) for t in t1]
            s1, v1 = sum(map(abs, c)), sum(map(abs, v))
            radius = math.sqrt(c[0] * c[0] + c[1] * c[1])                           # np.linalg.norm(box.center[:2], 2)
            out["radius"][b, i], out["limit"][b, i] = radius, rng[lab]
            inside = not radius > rng[lab]
            c = tuple(r + t for r, t in zip(turn(q2, c, route), t2))
            q = qmul(q2, q)
            v = turn(q2, v, route)
            speed = math.sqrt(v[0] * v[0] + v[1] * v[1])                            # np.sqrt(box.velocity[0]**2 + box.velocity[1]**2)
            out["speed"][b, i] = speed
            if not inside:
                continue
            out["rec"][b, k] = (*c, float(row[4]), float(row[3]), float(row[5]), *q, v[0], v[1])
            out["score"][b, k], out["name"][b, k], out["src"][b, k] = scores[b, i], lab, i
            out["attr"][b, k] = mov[lab] if speed > speed_thr else still[lab]
            out["half"][b, k] = half
            out["bound"][b, k, 0:3] = [sum(e1) + 18 * U * s1 + 8 * U * abs(t) for t in t2]
            out["bound"][b, k, 6:10] = 26 * U
            out["bound"][b, k, 10:12] = 3 * 18 * U * v0 + 18 * U * v1
            k += 1
        out["kept"][b] = k
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
def random_unit_quaternion(rng):
    q = rng.normal(size=4)
    return q / math.sqrt(float((q * q).sum()))


def random_poses(rng, B):
    """lidar -> ego: any rotation, a translation of a metre or two; ego -> global: any rotation, a translation of up to about 2000 m."""
    poses = np.empty((B, 2, 7))
    for b in range(B):
        poses[b, 0, :4], poses[b, 0, 4:] = random_unit_quaternion(rng), rng.uniform(-2.0, 2.0, 3)
        poses[b, 1, :4], poses[b, 1, 4:] = random_unit_quaternion(rng), rng.uniform(-2000.0, 2000.0, 3) * (1.0, 1.0, 0.01)
    return poses


def random_sample(rng, n, K, pattern, pose, invalid=0):
    """n boxes in K rows.  ``pattern`` places each box's EGO-frame radius inside (<= 0.8 of its class range) or beyond (>= 1.2) it: 'all', 'none', 'alternating'
    (even rows inside), 'random' (anywhere up to twice the range: about half beyond); the centre is drawn in the ego frame and taken back through ``pose`` (lidar -> ego, any rotation) into the
    lidar frame, where it is rounded to float32.  ``invalid``: that many rows get a NaN or infinite column, an infinite score or a label outside the classes.
    Rows beyond n hold NaN boxes and label 99: they must not be read."""
    boxes = np.full((K, 9), np.nan, dtype=np.float32)
    scores, labels = np.full(K, np.nan, dtype=np.float32), np.full(K, 99, dtype=np.int64)
    limit = tables()[0]
    lab = rng.integers(0, len(CLASS_NAMES), n)
    inside = dict(all=np.ones(n, bool), none=np.zeros(n, bool), alternating=np.arange(n) % 2 == 0, random=rng.random(n) < 0.5)[pattern]
    frac = np.where(inside, rng.uniform(0.0, 0.8, n), rng.uniform(1.2, 2.0, n))
    if pattern == "random":
        frac = rng.uniform(0.0, 2.0, n)                                      # anywhere, the neighbourhood of the range included
    rad, ang = frac * limit[lab], rng.uniform(-math.pi, math.pi, n)
    ego = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3.0, 3.0, n)], axis=1)
    centre = (ego - pose[4:]) @ np.array(rotation_matrix(tuple(pose[:4])))                       # R^T (c - t), row by row
    speed = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.4, n), rng.uniform(0.4, 15.0, n))
    heading = rng.uniform(-math.pi, math.pi, n)
    dz = rng.uniform(0.3, 4.0, n)
    boxes[:n] = np.stack([centre[:, 0], centre[:, 1], centre[:, 2] - dz / 2, rng.uniform(0.3, 12.0, n), rng.uniform(0.3, 3.0, n), dz,
                          rng.uniform(-2 * math.pi, 2 * math.pi, n), speed * np.cos(heading), speed * np.sin(heading)], axis=1).astype(np.float32)
    scores[:n] = np.sort(rng.uniform(0.01, 0.99, n))[::-1].astype(np.float32)
    labels[:n] = lab
    for j, i in enumerate(rng.choice(n, size=min(invalid, n), replace=False)):
        if j % 3 == 0:
            boxes[i, int(rng.integers(0, 9))] = (np.nan, np.inf, -np.inf)[j // 3 % 3]
        elif j % 3 == 1:
            labels[i] = (-1, len(CLASS_NAMES), 1 << 40)[j // 3 % 3]
        else:
            scores[i] = np.inf
    return boxes, scores, labels


PATTERNS = ("all", "none", "alternating", "random")
# name -> (counts, K, pattern per sample or one for all, invalid rows a sample, with_velocity, seed)
RANDOM_CASES = {
    "n0": ((0,), 4, "all", 0, True, 11),
    "n1": ((1,), 1, "all", 0, True, 12),
    "n1_none": ((1,), 3, "none", 0, True, 13),
    "wave_all": ((63, 64, 65), 65, "all", 0, True, 14),
    "wave_none": ((63, 64, 65), 65, "none", 0, True, 15),
    "wave_alternating": ((63, 64, 65), 65, "alternating", 0, True, 16),
    "wave_random": ((63, 64, 65), 65, "random", 4, True, 17),
    "wave_mixed": ((63, 64, 65), 70, ("none", "random", "all"), 2, True, 18),
    "wave_novel": ((63, 64, 65), 65, "random", 4, False, 19),
    "chunk_all": ((256, 257), 257, "all", 0, True, 20),
    "chunk_alternating": ((256, 257), 257, "alternating", 0, True, 21),
    "chunk_random": ((256, 257), 300, "random", 6, True, 22),
    "full": ((2048,), 2048, "random", 9, True, 23),
}
EXACT_CASE = "exact"
CASES = tuple(RANDOM_CASES) + (EXACT_CASE,)
# the exact case: identity poses, zero translations.  (label by name, x, y, vx, what must come out: None = dropped, otherwise the attribute)
F32 = np.float32
EXACT_ROWS = (
    ("car", 30.0, 40.0, 0.0, "vehicle.parked"),                                                    # radius exactly 50 = the range: kept (not >)
    ("car", 30.0, float(np.nextafter(F32(40.0), F32(50.0))), 0.0, None),                           # the next float32: dropped
    ("car", 3.0, 4.0, float(F32(0.2)), "vehicle.moving"),                                          # float32(0.2) > 0.2
    ("car", 3.0, 4.0, float(np.nextafter(F32(0.2), F32(0.0))), "vehicle.parked"),                  # the float32 just below: still
    ("bus", 5.0, -6.0, 0.0, "vehicle.stopped"),
    ("pedestrian", -7.0, 2.0, 0.0, "pedestrian.standing"),
    ("barrier", 1.0, 1.0, 0.0, ""),
    ("traffic_cone", -1.0, 8.0, 0.0, ""),
    ("barrier", 0.0, 30.0, 5.0, ""),                                                               # radius exactly 30 = its range, moving: still ''
    ("pedestrian", 24.0, 32.0, 1.0, "pedestrian.moving"),                                          # radius exactly 40
)


def exact_case():
    n = len(EXACT_ROWS)
    boxes = np.zeros((1, n, 9), dtype=np.float32)
    labels = np.zeros((1, n), dtype=np.int64)
    for i, (name, x, y, vx, _) in enumerate(EXACT_ROWS):
        boxes[0, i] = (x, y, -1.0, 4.0, 2.0, 1.5, 0.0, vx, 0.0)
        labels[0, i] = CLASS_NAMES.index(name)
    scores = np.linspace(0.9, 0.1, n, dtype=np.float32)[None]
    poses = np.array([[IDENTITY_POSE, IDENTITY_POSE]], dtype=np.float64)
    return dict(boxes=boxes, scores=scores, labels=labels, counts=np.array([n], dtype=np.int64), poses=poses, with_velocity=True)


def build_case(name):
    """The seeded inputs of a case: dict(boxes (B, K, 9) f32, scores, labels, counts, poses, with_velocity)."""
    if name == EXACT_CASE:
        return exact_case()
    counts, K, pattern, invalid, vel, seed = RANDOM_CASES[name]
    rng = np.random.default_rng(seed)
    poses = random_poses(rng, len(counts))
    parts = [random_sample(rng, n, K, pattern if isinstance(pattern, str) else pattern[b], poses[b, 0], invalid) for b, n in enumerate(counts)]
    return dict(boxes=np.stack([p[0] for p in parts]), scores=np.stack([p[1] for p in parts]), labels=np.stack([p[2] for p in parts]),
                counts=np.array(counts, dtype=np.int64), poses=poses, with_velocity=vel)


INPUT_KEYS = ("boxes", "scores", "labels", "counts", "poses")
STORED = OUT_KEYS + ("bound", "radius", "limit", "speed", "half")
BOUND_COLUMNS = [0, 1, 2, 6, 10]


def fixture_arrays():
    """Everything tools/gen_golden_nusc_results.py stores: per case the inputs and the restated outputs."""
    arrays = {}
    for name in CASES:
        c = build_case(name)
        r = restate(c["boxes"], c["scores"], c["labels"], c["counts"], c["poses"], c["with_velocity"])
        arrays.update({f"{name}_{k}": c[k] for k in INPUT_KEYS})
        arrays.update({f"{name}_{k}": r[k] for k in STORED})
        arrays[f"{name}_bound"] = r["bound"][..., BOUND_COLUMNS]           # (the twelve bounds are five numbers: three translations, the orientation, the velocity)
        arrays[f"{name}_with_velocity"] = np.array(int(c["with_velocity"]))
    return arrays


_LOADED = {}


def load_case(name):
    """A case from the fixture: the inputs and the restated outputs, computed once and shared (do not modify)."""
    if "z" not in _LOADED:
        _LOADED["z"] = dict(np.load(FIXTURE))
    z = _LOADED["z"]
    c = {k: z[f"{name}_{k}"] for k in INPUT_KEYS + STORED}
    five = c["bound"]
    c["bound"] = np.zeros(five.shape[:2] + (12,))
    c["bound"][..., [0, 1, 2, 6, 7, 8, 9, 10, 11]] = five[..., [0, 1, 2, 3, 3, 3, 3, 4, 4]]
    c["with_velocity"] = bool(z[f"{name}_with_velocity"])
    return c


def pose_records(poses):
    """float64 (B, 2, 7) -> the pose records (dicts of lists) NuScenesResults takes."""
    return [dict(lidar2ego_rotation=p[0, :4].tolist(), lidar2ego_translation=p[0, 4:].tolist(), ego2global_rotation=p[1, :4].tolist(),
                 ego2global_translation=p[1, 4:].tolist()) for p in poses]
