#!/usr/bin/env python3
"""COLMAP reconstruction -> scan folder for ``eval.py --dataset folder`` -- counterpart of the reference's ``colmap_input.py``
with the same flags (plus ``--device``):

    python colmap_input.py --input_folder <scene> [--output_folder <scan>] [--num_src_images N]
                           [--theta0 5 --sigma1 1 --sigma2 10] [--convert_format] [--device cuda]
                           [--undistort [--blank_pixels 0 --min_scale 0.2 --max_scale 2 --num_workers 4]]

``<scene>/sparse/{cameras,images,points3D}.bin`` (or ``.txt``) and ``<scene>/images/`` become ``<scan>/cams_1/%08d_cam.txt``,
``<scan>/images/%08d.jpg`` and ``<scan>/pair.txt``.  The view-selection scores and the depth ranges are computed by the HIP
kernels ``itermvs_view_scores`` / ``itermvs_depth_ranges`` (itermvs_amd/colmap.py).  ``--undistort`` resamples the images of
cameras with lens distortion (COLMAP's default SIMPLE_RADIAL, OPENCV, the fisheye models ...) to pinhole cameras with
``itermvs_undistort_rgb8`` and writes those cameras; without it the parameters' distortion terms are ignored, as in the reference.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from itermvs_amd.colmap import build_parser, main  # noqa: E402,F401

if __name__ == "__main__":
    main()
