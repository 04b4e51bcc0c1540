"""Plain numpy restatement of the map merge (include/aruco_slam_hip.h "map merge"): the yardstick of
tests/test_merge_maps.py.  Python loops and np.linalg.inv; shares no code with the library."""
import math

import numpy as np

ID_TABLE = 1024
MAP_DTYPE = np.dtype([("id", "<i4"), ("index", "<i4"), ("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("S", "<f8", (9,))])
PI = math.pi


def wrap(a):
    """the library's single angle wrap (ArucoSlam::normAngle)"""
    if a >= PI:
        a -= 2 * PI
    if a < -PI:
        a += 2 * PI
    return a


def rot(phi):
    c, s = math.cos(phi), math.sin(phi)
    return np.array([[c, -s], [s, c]])


def moved(rec, T):
    """a record's mean through T = (tx, ty, phi)"""
    xy = rot(T[2]) @ np.array([rec["x"], rec["y"]]) + T[:2]
    return np.array([xy[0], xy[1], wrap(float(rec["theta"]) + T[2])])


def usable(C):
    if not np.all(np.isfinite(C)):
        return False
    return C[0, 0] > 0 and np.linalg.det(C[:2, :2]) > 0 and np.linalg.det(C) > 0


def merge(records, n_maps, per_map, anchor=0, min_common=2):
    """records: n_maps x per_map MAP_DTYPE -> (ids, xyth, sigmas n x 3 x 3, n_seen, rounds, T n_maps x 3)"""
    records = np.asarray(records).view(MAP_DTYPE).reshape(n_maps, per_map)
    index = []                                          # per map: id -> first record with it
    for m in range(n_maps):
        d = {}
        for i in range(per_map):
            lid = int(records[m, i]["id"])
            if 0 <= lid < ID_TABLE and lid not in d:
                d[lid] = i
        index.append(d)
    table = {lid: np.array([records[anchor, i]["x"], records[anchor, i]["y"], records[anchor, i]["theta"]]) for lid, i in index[anchor].items()}
    rounds = np.full(n_maps, -1, np.int32)
    T = np.zeros((n_maps, 3))
    rounds[anchor] = 0
    k = 0
    while np.any(rounds < 0):
        k += 1
        new = []
        for m in range(n_maps):
            if rounds[m] >= 0:
                continue
            K = sorted(set(index[m]) & set(table))
            if len(K) < min_common:
                continue
            p = np.array([[records[m, index[m][lid]]["x"], records[m, index[m][lid]]["y"]] for lid in K])
            q = np.array([table[lid][:2] for lid in K])
            pm, qm = p.sum(0) / len(K), q.sum(0) / len(K)
            dp, dq = p - pm, q - qm
            a = float(np.sum(dp[:, 0] * dq[:, 1] - dp[:, 1] * dq[:, 0]))
            b = float(np.sum(dp[:, 0] * dq[:, 0] + dp[:, 1] * dq[:, 1]))
            if a == 0.0 and b == 0.0:
                continue
            phi = math.atan2(a, b)
            t = qm - rot(phi) @ pm
            new.append((m, np.array([t[0], t[1], phi])))
        if not new:
            break
        for m, Tm in new:
            rounds[m] = k
            T[m] = Tm
        for m, Tm in new:                                # ascending map order: the lowest map with a new id inserts it
            for lid, i in index[m].items():
                if lid not in table:
                    table[lid] = moved(records[m, i], Tm)
    ids = np.array(sorted(table), np.int32)
    n = ids.size
    xyth, sigmas, seen = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros(n, np.int32)
    for e, lid in enumerate(ids):
        m0 = table[int(lid)]
        Lam, eta = np.zeros((3, 3)), np.zeros(3)
        for m in range(n_maps):
            if rounds[m] < 0 or int(lid) not in index[m]:
                continue
            rec = records[m, index[m][int(lid)]]
            S = np.array(rec["S"]).reshape(3, 3)
            C = 0.5 * (S + S.T)
            J = np.eye(3)
            J[:2, :2] = rot(T[m, 2])
            Cp = J @ C @ J.T
            if not usable(Cp):
                continue
            d = moved(rec, T[m]) - m0
            d[2] = wrap(d[2])
            W = np.linalg.inv(Cp)
            Lam += W
            eta += W @ d
            seen[e] += 1
        xyth[e] = m0
        if seen[e]:
            P = np.linalg.inv(Lam)
            xyth[e] = m0 + P @ eta
            xyth[e, 2] = wrap(xyth[e, 2])
            sigmas[e] = P
    return ids, xyth, sigmas, seen, rounds, T
