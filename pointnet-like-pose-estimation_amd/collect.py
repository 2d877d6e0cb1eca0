"""Import shim: with this directory on sys.path, ``import collect`` (how the reference's capture
scripts import it, e.g. point_collect/test.py:2) resolves to the MI355X
implementation of clip_distance, delet_outlier_radius and cluster_point."""
import os as _os
import sys as _sys

_here = _os.path.dirname(_os.path.abspath(__file__))
if _here not in _sys.path:
    _sys.path.insert(0, _here)

from pn2.collect import *  # noqa: E402,F401,F403
from pn2.collect import __all__  # noqa: E402,F401
