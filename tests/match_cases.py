"""Projection queries around a frame's own keypoints.  Shared by tests/test_match_gpu.py and tests/test_prep_gpu.py."""
import numpy as np

import synth_frames as sf


def make_queries(kps, desc, rng, th=15.0, jitter=2.0, p_block=0.7, with_ur=False):
    import psl_slam_amd as P
    scale = sf.orb_scale_factors()
    q = np.zeros(len(kps), P.PROJQUERY_DTYPE)
    q["u"] = kps["x"] + rng.uniform(-jitter, jitter, len(kps)).astype(np.float32)
    q["v"] = kps["y"] + rng.uniform(-jitter, jitter, len(kps)).astype(np.float32)
    q["radius"] = np.float32(th) * scale[kps["octave"]]
    q["min_level"] = kps["octave"] - 1
    q["max_level"] = kps["octave"] + 1
    q["angle"] = kps["angle"]
    q["blocks"] = (rng.random(len(kps)) < p_block).astype(np.int32)
    q["ur"] = q["u"] - np.float32(40.0) / np.float32(2.0) if with_ur else 0
    return q, desc.copy()
