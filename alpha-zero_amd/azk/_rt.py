"""What the wrapper modules need at run time."""
import sys


def _torch():
    """torch, or AzkError without a GPU: the package's own _torch, looked up at call time (tests/test_fold_tables.py replaces
    azk._torch to build tables on the CPU)."""
    return sys.modules[__package__]._torch()
