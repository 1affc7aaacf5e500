from .single import *  # noqa: F401,F403
from .forest import *  # noqa: F401,F403
from .batched import *  # noqa: F401,F403
from .dynamic import *  # noqa: F401,F403
from .batched_dynamic import *  # noqa: F401,F403
