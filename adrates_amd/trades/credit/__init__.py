"""Credit products: fixed-rate bonds and floating-rate notes (cavour/trades/credit/)."""
from .bond import Bond  # noqa: F401
from .frn import FRN  # noqa: F401
