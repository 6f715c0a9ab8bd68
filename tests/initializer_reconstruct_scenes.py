"""Synthetic two-view scenes for the reconstruction tests and the golden generator: float64 geometry,
float32 keypoints and models.  Frame 1 is K[I|0], frame 2 K[R|t]; the models are the exact F21 /
H21 of the motion (and plane), narrowed to float32."""
import numpy as np

f32 = np.float32
K4 = np.array([500.0, 500.0, 320.0, 240.0], f32)  # fx, fy, cx, cy
PLANE_SEED = 16  # of the plane scenes' points: one at which all three keep 5 % from their boundaries
SCENE_NAMES = ("f60", "f130", "f300", "h_accept", "h_ambiguous_t", "h_ambiguous_plane")


def K_of(K4=K4):
    return np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], np.float64)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * (S @ S)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


R_TRUE = rodrigues((0.2, 1.0, 0.1), 0.05)


def project(X, R, t, K):
    Y = X @ R.T + t
    return (Y[:, :2] / Y[:, 2:3]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])


def make_pair(X, R, t, noise=0.3, seed=0, extra1=0, extra2=0, shuffle=False):
    """Keypoints of both frames (n x 2 float32) and matches12 for 3-D points X.  `extra1` / `extra2`
    unmatched keypoints are mixed in and, with `shuffle`, frame 2 is permuted, so that match ordinal,
    frame-1 index and frame-2 index all differ."""
    rng = np.random.default_rng(seed)
    K = K_of()
    n = len(X)
    p1 = project(X, np.eye(3), np.zeros(3), K) + rng.normal(0, noise, (n, 2)) * (noise > 0)
    p2 = project(X, R, np.asarray(t, np.float64), K) + rng.normal(0, noise, (n, 2)) * (noise > 0)
    n1, n2 = n + extra1, n + extra2
    k1 = rng.uniform(0, 480, (n1, 2))
    k2 = rng.uniform(0, 480, (n2, 2))
    pos1 = np.sort(rng.permutation(n1)[:n]) if extra1 else np.arange(n)
    pos2 = rng.permutation(n2)[:n] if shuffle else np.arange(n)
    k1[pos1] = p1
    k2[pos2] = p2
    m12 = np.full(n1, -1, np.int32)
    m12[pos1] = pos2
    return k1.astype(f32), k2.astype(f32), m12


def F_of(R, t, K=None):
    K = K_of() if K is None else K
    Ki = np.linalg.inv(K)
    return (Ki.T @ skew(np.asarray(t, np.float64)) @ R @ Ki).astype(f32)


def H_of(R, t, normal, d, K=None):
    """The homography of the plane normal . X = d (frame-1 coordinates)."""
    K = K_of() if K is None else K
    return (K @ (R + np.outer(np.asarray(t, np.float64), normal) / d) @ np.linalg.inv(K)).astype(f32)


def volume_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 10, n)], 1)


def plane_points(n, seed, z0, ax, ay):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.2, 1.2, n)
    return np.stack([x, y, z0 + ax * x + ay * y], 1)


def scene(name, **kw):
    """dict(k1, k2, m12, M21, use_h, R, t, X) of a named scene; pts_seed reseeds the plane scenes'
    points, the rest of kw goes to make_pair."""
    pts_seed = kw.pop("pts_seed", PLANE_SEED)
    if name in ("f60", "f130", "f300"):
        n = int(name[1:])
        t = np.array([0.3, 0.02, 0.03])
        X = volume_points(n, 100 + n)
        M, use_h = F_of(R_TRUE, t), False
    else:
        z0, ax, ay, t = {"h_accept": (3.0, 0.8, 0.1, (0.6, 0.3, 0.0)),
                         "h_ambiguous_t": (3.0, 0.8, 0.1, (0.3, 0.02, 0.03)),
                         "h_ambiguous_plane": (5.0, 0.3, 0.1, (0.6, 0.3, 0.0))}[name]
        t = np.array(t)
        X = plane_points(130, pts_seed, z0, ax, ay)
        # z = z0 + ax x + ay y  <=>  (-ax, -ay, 1) . X = z0
        M, use_h = H_of(R_TRUE, t, np.array([-ax, -ay, 1.0]), z0), True
    kw.setdefault("seed", 1)
    k1, k2, m12 = make_pair(X, R_TRUE, t, **kw)
    return dict(k1=k1, k2=k2, m12=m12, M21=M, use_h=use_h, R=R_TRUE, t=t, X=X)


def mask_first(m12, k):
    """A mask over match ordinals with the first k set."""
    n = int((np.asarray(m12) >= 0).sum())
    m = np.zeros(n, np.uint8)
    m[:k] = 1
    return m


def keypoint_records(xy, dtype):
    """n x 2 floats as keypoint records of `dtype` (orbslam_jpminipc_amd.KEYPOINT_DTYPE)."""
    k = np.zeros(len(xy), dtype)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k
