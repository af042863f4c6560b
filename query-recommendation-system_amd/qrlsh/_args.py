"""Argument checks the modules share (no device, no library)."""
import numpy as np

INT_IN_TEXT = "%s must be an integer in %d..%d, got %r"


def _int_in(value, name, lo, hi):
    """value as an int when it is an integer (a bool is not) in lo..hi, ValueError otherwise"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(INT_IN_TEXT % (name, lo, hi, value))
    return int(value)
