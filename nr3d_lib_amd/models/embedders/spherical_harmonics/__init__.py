from .sphere_harmonics import *  # noqa: F401,F403
