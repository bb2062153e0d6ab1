"""
NumPy / Python restatements of three host rules the library implements once (csrc/amt_params.h, namespace amt_prm):
the pole test (amt_pole_in_view), the neighbour and steadiness tests and the box extrapolation behind the sequence
pipelines' box hints (amt_frames_close, amt_box_hint).  They are what the package itself ran before those became library
calls, unchanged; tests/test_host_rules_cpu.py compares the exported functions with them.
"""
import numpy as np


def pole_in_view(params, min_elevation=None, magnetic=False):
    """
    Host-side pole test for camera mappings: is the geographic (or, with magnetic=True, the SM) north
    or south pole of the mapping shell imaged by a valid pixel?  The pole point is projected through
    the inverse TAN model; it counts when it falls inside the frame, is the *first* hit of its ray
    and lies above the elevation threshold.  Returns +1 (north), -1 (south) or 0.
    """
    rot = np.array(params.rot[:]).reshape(3, 3)
    cd = np.array(params.cd[:]).reshape(2, 2)
    cam = np.array(params.cam[:])
    m = np.array(params.m_sm[:] if magnetic else params.m_geo[:]).reshape(3, 3)
    a, b = params.a, params.b
    scale = np.array([1 / a, 1 / a, 1 / b])
    for sign in (1, -1):
        u = m.T.dot([0.0, 0.0, float(sign)])                 # pole axis in J2000
        pole = u / np.sqrt(np.sum((u * scale) ** 2))          # point of the shell on that axis
        los = pole - cam
        dist = np.sqrt(los.dot(los))
        d = los / dist
        # first intersection of the ray with the shell (same quadratic as intersection.py:58-104)
        ds, os_ = d * scale, -cam * scale
        d_o, d_d, o_o = ds.dot(os_), ds.dot(ds), os_.dot(os_)
        disc = d_o * d_o - o_o * d_d + d_d
        if disc < 0:
            continue
        inside = np.sum((cam * scale) ** 2) < 1
        t = ((d_o + np.sqrt(disc)) if inside else (d_o - np.sqrt(disc))) / d_d
        if abs(t - dist) > 1e-6 * dist:
            continue                                           # the pole is on the far side
        v = rot.T.dot(d)                                       # native (projection) frame
        if v[2] <= 0:
            continue
        k = 180 / np.pi
        px, py = np.linalg.solve(cd, [k * v[1] / v[2], -k * v[0] / v[2]])
        x, y = px + params.crpix[0] - 1, py + params.crpix[1] - 1
        if not (-0.5 <= x <= params.width - 0.5 and -0.5 <= y <= params.height - 0.5):
            continue
        if min_elevation is not None:
            elev = np.rad2deg(np.arcsin(np.clip(-d.dot(pole) / np.sqrt(pole.dot(pole)), -1, 1)))
            if not elev >= min_elevation:
                continue
        return sign
    return 0


def close(a, b):
    """Are two amt_frame_params neighbours in a sequence: same frame size, camera model within 1 % in scale, camera
    within 100 km, boresight and Earth rotation within about half a degree, shell within 30 km?"""
    if (a.width, a.height, a.fast_center) != (b.width, b.height, b.fast_center):
        return False
    if abs(a.a - b.a) > 30.0 or abs(a.b - b.b) > 30.0:
        return False
    # (separately solved frames of one sequence differ in the sixth digit of their CD matrix: the plate scale within 1 %
    # and the reference pixel within 5 px move the box by far less than the superset's margin)
    cd_tol = 0.01 * max(abs(v) for v in a.cd)
    for x, y, tol in ((a.cam, b.cam, 100.0), (a.rot, b.rot, 0.01), (a.m_geo, b.m_geo, 0.01), (a.m_sm, b.m_sm, 0.01),
                      (a.cd, b.cd, cd_tol), (a.crpix, b.crpix, 5.0)):
        for u, v in zip(x, y):
            if abs(u - v) > tol:
                return False
    return True


def steady(a, b, c, n_ab, n_bc):
    """Frames a, b (n_ab frames apart) and c (n_bc frames after b): same frame size, shell and camera model as `close`
    asks, c within 400 km of b, and the camera has moved from b to c as it did from a to b (20 % + 5 km)?"""
    if n_ab <= 0 or n_bc <= 0 or n_bc > 16:
        return False
    if (b.width, b.height, b.fast_center) != (c.width, c.height, c.fast_center):
        return False
    if abs(b.a - c.a) > 30.0 or abs(b.b - c.b) > 30.0:
        return False
    for x, y, tol in ((b.cam, c.cam, 400.0), (b.rot, c.rot, 0.05), (b.m_geo, c.m_geo, 0.05), (b.m_sm, c.m_sm, 0.05),
                      (b.crpix, c.crpix, 5.0)):
        for u, v in zip(x, y):
            if abs(u - v) > tol:
                return False
    # the CD matrix turns with the camera's roll (5e-4 per element over 20 s of the real ISS029 sequence): same plate scale
    # within 1 %, and the elements where the pace of a -> b puts them
    scale_b = abs(b.cd[0] * b.cd[3] - b.cd[1] * b.cd[2]) ** 0.5
    scale_c = abs(c.cd[0] * c.cd[3] - c.cd[1] * c.cd[2]) ** 0.5
    if not (scale_b > 0 and abs(scale_c - scale_b) <= 0.01 * scale_b):
        return False
    for i in range(4):
        step = (b.cd[i] - a.cd[i]) / n_ab
        if abs((c.cd[i] - b.cd[i]) - step * n_bc) > 0.3 * abs(step * n_bc) + 0.01 * scale_b:
            return False
    for i in range(3):
        step = (b.cam[i] - a.cam[i]) / n_ab
        if abs((c.cam[i] - b.cam[i]) - step * n_bc) > 0.2 * abs(step * n_bc) + 5.0:
            return False
    for i in range(9):
        step = (b.rot[i] - a.rot[i]) / n_ab
        if abs((c.rot[i] - b.rot[i]) - step * n_bc) > 0.3 * abs(step * n_bc) + 2e-3:
            return False
    return True


def box_hint(last, prev, k, p):
    """
    Estimate of frame k's bounding-box reduction from frames that are already finished, or None.  `last`, `prev`: (exact
    bbox reduction, amt_frame_params, index) of the latest finished frame and of the one finished before it, or None.  The
    latest finished frame's exact box as it is when that frame is a neighbour of this one (`close`); else, in a steady
    sequence — the two latest finished frames are neighbours of each other and the camera has kept its pace — their boxes
    extrapolated linearly to this frame.
    """
    if last is None:
        return None
    if close(last[1], p):
        return last[0]
    if prev is None or not close(prev[1], last[1]) or not steady(prev[1], last[1], p, last[2] - prev[2], k - last[2]):
        return None
    if bool(prev[0][7]) != bool(last[0][7]) or (last[0][3] - last[0][2] > 180) != (prev[0][3] - prev[0][2] > 180):
        return None                     # a pole or the date line came into view between the two
    f = (k - last[2]) / float(last[2] - prev[2])
    est = [b + f * (b - a) for a, b in zip(prev[0][:6], last[0][:6])] + list(last[0][6:])
    est[0], est[1] = max(est[0], -90.0), min(est[1], 90.0)
    for i in (2, 3, 4, 5):
        est[i] = min(max(est[i], -180.0), 180.0)
    return est
