"""nr3d_lib_amd.maths -- the part of the reference's ``nr3d_lib.maths`` that stands on a native extension: ``knn_points`` /
``knn_gather`` (pytorch3d_knn.py) and ``chamfer_distance`` (chamfer_distance.py), on csrc/knn.hip."""
from .pytorch3d_knn import *
from .chamfer_distance import *
