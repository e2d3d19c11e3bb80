"""Credit products: fixed-rate bonds (cavour/trades/credit/bond.py)."""
from .bond import Bond  # noqa: F401
