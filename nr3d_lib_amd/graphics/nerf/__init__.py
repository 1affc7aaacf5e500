from .nerf_utils import *
from .nerf_ray_query import *
from .nerf_distant_ray_query import *
