"""Writes tests/golden/relight_poses.npz: the camera poses of the REFERENCE's blender_backend/blender_utils.generate_relghting_poses for
a few (num, azimuth, elevation, dist).

Run once on a machine with the reference checkout, from its directory:

    cd <reference> && python <repo>/scripts/gen_relight_golden.py

blender_utils imports bpy at module level; Blender is not needed for the pose arithmetic, so an empty module stands in for it.  The
test suite needs neither this script nor the reference, only the .npz file: `cases` [n,4] = (num, azimuth, elevation, dist) and
`poses_<i>` [num,3,4] float64 per case.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(5, 0.0, 45.0, 3.0), (8, 30.0, 20.0, 2.5), (3, -120.0, 60.0, 4.0), (7, 200.0, -10.0, 1.5)]


def main():
    sys.modules.setdefault('bpy', types.ModuleType('bpy'))
    sys.path.insert(0, os.getcwd())
    from blender_backend.blender_utils import generate_relghting_poses
    out = {'cases': np.array(CASES, np.float64)}
    for i, (num, az, el, dist) in enumerate(CASES):
        out[f'poses_{i}'] = np.asarray(generate_relghting_poses(num, az, el, dist), np.float64)
    path = os.path.join(ROOT, 'tests', 'golden', 'relight_poses.npz')
    np.savez(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
