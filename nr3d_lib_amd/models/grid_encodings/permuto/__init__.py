from .permuto import *  # noqa: F401,F403
from .permuto_encoding import *  # noqa: F401,F403
