"""What k_pose computes, restated from the formulas in numpy long double (64-bit significand) - independent of oracle/pnp.cpp
and of the kernel: Rodrigues, the pinhole + plumb-bob projection (k1, k2, p1, p2, k3), the reprojection cost of the 4 float
corners with its Jacobian by the complex step (clongdouble: exact to rounding, no step-size error), the rotation distance, the
observation of a marker (aruco_slam.cpp:325-374 with a camera mount) and CalculateCovariance (aruco_slam.cpp:437-471).
Every function takes a batch: leading axes are markers."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
PI = LD("3.14159265358979323846264338327950288")
STEP = LD("1e-30")                       # complex step (relative to parameters of size ~1)


def object_points(marker_length):
    """the marker's corners in its own frame: top-left, top-right, bottom-right, bottom-left (z = 0), half-length rounded to
    float as the reference's objectPoints_ holds it"""
    h = LD(float(np.float32(np.float32(marker_length) / np.float32(2))))
    return np.array([[-h, h], [h, h], [h, -h], [-h, -h]], dtype=LD)


def skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def rodrigues(r):
    """R = I + sin(th)/th [r]x + (1 - cos th)/th^2 [r]x^2, th^2 = r.r (no conjugate: analytic, so the complex step applies);
    |r| > 0 (a visible marker has |r| near pi)"""
    r = np.asarray(r)
    th2 = np.sum(r * r, axis=-1)[..., None, None]
    th = np.sqrt(th2)
    Kx = skew(r)
    eye = np.eye(3, dtype=LD)
    return eye + (np.sin(th) / th) * Kx + ((1 - np.cos(th)) / th2) * (Kx @ Kx)


def project(R, t, K, D, marker_length):
    """pixel coordinates (..., 4, 2) of the marker's corners for rotation R (..., 3, 3) and translation t (..., 3)"""
    obj = object_points(marker_length)
    d = np.zeros(5, dtype=LD)
    d[:len(D)] = np.asarray(D, dtype=LD)
    k1, k2, p1, p2, k3 = d
    P = np.einsum("...ij,qj->...qi", R[..., :, :2], obj) + t[..., None, :]
    x, y = P[..., 0] / P[..., 2], P[..., 1] / P[..., 2]
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    K = np.asarray(K, dtype=LD)
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], -1)


def residuals(rvec, tvec, corners, K, D, marker_length):
    """projection minus corners, (..., 8)"""
    rvec, tvec = np.asarray(rvec), np.asarray(tvec)
    p = project(rodrigues(rvec), tvec, K, D, marker_length)
    return (p - np.asarray(corners, dtype=LD).reshape(p.shape)).reshape(p.shape[:-2] + (8,))


def cost(rvec, tvec, corners, K, D, marker_length):
    """sum of squared reprojection errors over the 4 corners (px^2)"""
    e = residuals(np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD), corners, K, D, marker_length)
    return np.sum(e * e, axis=-1)


def cost_at(R, t, corners, K, D, marker_length):
    """the cost at a pose given by its rotation matrix (the truth of a generated case)"""
    p = project(np.asarray(R, dtype=LD), np.asarray(t, dtype=LD), K, D, marker_length)
    e = p - np.asarray(corners, dtype=LD).reshape(p.shape)
    return np.sum(e * e, axis=(-1, -2))


def jacobian(rvec, tvec, corners, K, D, marker_length):
    """d residuals / d (r, t), (..., 8, 6), by the complex step"""
    p = np.concatenate([np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)], -1).astype(CLD)
    cols = []
    for j in range(6):
        q = p.copy()
        q[..., j] += 1j * STEP
        cols.append(residuals(q[..., :3], q[..., 3:], corners, K, D, marker_length).imag / STEP)
    return np.stack(cols, -1)


def newton_step(rvec, tvec, corners, K, D, marker_length):
    """|dp| / |p| of the Gauss-Newton step dp = (J^T J)^-1 J^T e from p = (r, t): how far p is from a stationary point of the cost,
    in the units of solvePnP's own stopping rule (|dp| / |p| < FLT_EPSILON).  The gradient J^T e alone does not vanish at a
    converged pose: with float corners the residual e is rounding noise, and a step of FLT_EPSILON |p| moves e by about as much"""
    p = np.concatenate([np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)], -1)
    e = residuals(p[..., :3], p[..., 3:], corners, K, D, marker_length)
    J = jacobian(rvec, tvec, corners, K, D, marker_length)
    JtJ = np.einsum("...ri,...rj->...ij", J, J).astype(np.float64)
    g = np.einsum("...ri,...r->...i", J, e).astype(np.float64)
    dp = np.linalg.solve(JtJ, g[..., None])[..., 0]
    return np.sqrt(np.sum(dp * dp, axis=-1)) / np.sqrt(np.sum(np.asarray(p, np.float64) ** 2, axis=-1))


def rotation_distance(ra, rb):
    """max |R(ra) - R(rb)| over the 9 entries"""
    return np.max(np.abs(rodrigues(np.asarray(ra, dtype=LD)) - rodrigues(np.asarray(rb, dtype=LD))), axis=(-1, -2))


def norm_angle(a):
    """ArucoSlam::normAngle (aruco_slam.cpp:412-421): one wrap into [-pi, pi)"""
    a = np.where(a >= PI, a - 2 * PI, a)
    return np.where(a < -PI, a + 2 * PI, a)


def observation(rvec, tvec, mount=(0.0, 0.0, 0.0)):
    """(x, y, theta) of a marker at (rvec, tvec) seen by a camera mounted at (mx, my) with heading psi: the camera-frame
    (t_z, -t_x, normAngle(atan2(-R02, R22))) rotated by psi and moved by (mx, my), theta = normAngle(theta0 + psi)"""
    rvec, tvec = np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)
    R = rodrigues(rvec)
    mx, my, psi = (LD(float(v)) for v in mount)
    x0, y0 = tvec[..., 2], -tvec[..., 0]
    th0 = norm_angle(np.arctan2(-R[..., 0, 2], R[..., 2, 2]))
    c, s = np.cos(psi), np.sin(psi)
    return np.stack([c * x0 - s * y0 + mx, s * x0 + c * y0 + my, norm_angle(th0 + psi)], -1)


def range_gate(tvec, threshold=3.0):
    """(passes, margin): float(|t|) > float(threshold) drops the marker (aruco_slam.cpp:327-333); margin = relative distance of
    |t| from the threshold"""
    nt = np.sqrt(np.sum(np.asarray(tvec, dtype=LD) ** 2, axis=-1))
    thr = np.float32(threshold)
    passes = ~(np.asarray(nt, dtype=np.float64).astype(np.float32) > thr)
    return passes, np.abs(nt - LD(float(thr))) / LD(float(thr))


def covariance(rvec, tvec, corners, K, D, marker_length, R_xyt=(100.0, 100.0, 10.0)):
    """(diag R (..., 3), slack (..., 3)): CalculateCovariance with the projections rounded to float (projectedPoints is a
    vector<Point2f>): object_error = (sum_q |c_q - p_q|^2 / 4) / |c_0 - c_2| * |t| / L, R = object_error (R_x, R_y, R_theta) +
    (1e-2, 1e-2, 1e-3).  slack bounds what one float ulp of rounding of each projected coordinate can change in R (a double
    projection and this one may round to neighbouring floats)"""
    rvec, tvec = np.asarray(rvec, dtype=LD), np.asarray(tvec, dtype=LD)
    p = project(rodrigues(rvec), tvec, K, D, marker_length)
    pf = np.asarray(p, dtype=np.float64).astype(np.float32)
    c = np.asarray(corners, dtype=np.float32).reshape(pf.shape)
    e = c.astype(LD) - pf.astype(LD)
    rms = np.sum(e * e, axis=(-1, -2)) / 4
    ulp = np.spacing(np.abs(pf)).astype(LD)
    drms = np.sum(2 * np.abs(e) * ulp + ulp * ulp, axis=(-1, -2)) / 4
    diag = np.sqrt(np.sum((c[..., 0, :].astype(LD) - c[..., 2, :].astype(LD)) ** 2, axis=-1))
    nt = np.sqrt(np.sum(tvec * tvec, axis=-1))
    scale = nt / LD(float(marker_length)) / diag
    w = np.array(R_xyt, dtype=LD)
    R = (rms * scale)[..., None] * w + np.array([LD("1e-2"), LD("1e-2"), LD("1e-3")])
    return R, (drms * scale)[..., None] * w


def covariance_gate(R):
    """(passes, margin): |diag R| > 1 drops the marker (aruco_slam.cpp:367)"""
    n = np.sqrt(np.sum(np.asarray(R, dtype=LD) ** 2, axis=-1))
    return ~(n > 1), np.abs(n - 1)


def rot_x(a):
    a = LD(a)
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=LD)


def rot_y(a):
    a = LD(a)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=LD)


def rot_z(a):
    a = LD(a)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=LD)


def facing():
    """a marker facing the camera, upright in the image: rotation pi about the camera's x axis"""
    return rot_x(PI)
