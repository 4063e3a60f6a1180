"""ops/ of the reference.  Its __init__ imports a module the snapshot does not have; the one module that exists is ccl."""
from . import ccl  # noqa: F401
