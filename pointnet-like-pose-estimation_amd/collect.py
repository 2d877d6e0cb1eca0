"""Import shim: with this directory on sys.path, ``import collect`` (how the reference's capture
scripts import it, e.g. point_collect/test.py:2) resolves to the MI355X
implementation of clip_distance, delete_plane, delet_outlier_radius, delet_outlier_statistical
and cluster_point.  ``__all__`` stays pn2.collect's four names (tests/test_abi_collect.py pins
them); delet_outlier_statistical, knn_mean_distance, delete_plane and segment_plane are imported
by name after the star import, so ``collect.delete_plane`` resolves all the same."""
import os as _os
import sys as _sys

_here = _os.path.dirname(_os.path.abspath(__file__))
if _here not in _sys.path:
    _sys.path.insert(0, _here)

from pn2.collect import *  # noqa: E402,F401,F403
from pn2.collect import __all__  # noqa: E402,F401
from pn2.collect import delet_outlier_statistical, knn_mean_distance  # noqa: E402,F401
from pn2.collect import delete_plane, segment_plane  # noqa: E402,F401
