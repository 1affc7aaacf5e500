from .neus_utils import *
from .neus_ray_query import *
from .neus_render import *
from .neus_forest_ray_query import *
