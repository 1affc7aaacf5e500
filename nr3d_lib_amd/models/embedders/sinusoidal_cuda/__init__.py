from .freq import *  # noqa: F401,F403
