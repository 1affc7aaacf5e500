from .renderer_mixin import *  # noqa: F401,F403
