"""Poses for the projection tests and the restated query rows of SearchByProjection(CurrentFrame, LastFrame) on a frame slot's
fetched data.  Shared by tests/test_project_gpu.py and tests/test_stereo_gpu.py."""
import numpy as np

import oracle_lib


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def T4(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def moved(Tlw, d, R=np.eye(3)):
    """Tcw of a camera displaced by d (and turned by R) in the last camera's coordinates: tlc == d."""
    return T4(R, -R @ np.asarray(d, np.float64)) @ Tlw


def restated_last(slot_data, Tlw, Tcw, points, mpdesc, cam, scale, th, th_depth, mono, vo, bounds):
    """oracle/project_oracle.cpp on (mvKeysUn, mvDepth, mvuRight, descriptors) of a slot and 4x4 poses: (queries, qdesc, owner)."""
    import psl_slam_amd as P
    kun, dep, _, desc = slot_data
    pts = None if points is None else np.ascontiguousarray(points, P.LASTPOINT_DTYPE)
    md = None if mpdesc is None else np.ascontiguousarray(mpdesc, np.uint8)
    return oracle_lib.pr_project_last(kun, desc, dep, P.pose(Tlw).reshape(1), P.pose(Tcw).reshape(1), pts, md, np.ascontiguousarray(cam).reshape(1),
                                      scale, th, th_depth, mono, vo, bounds)
