"""The transmit side: framers (encoders.py), LUT modulators (modulators.py), the integer phase they share (phase.py), the
device handle (device.py) and the ``Modulator`` that ties them to a protocol and a radio (modulator.py)."""
from . import encoders, modulators, phase  # noqa: F401
from .encoders import DataLengthError  # noqa: F401
from .modulator import Modulator  # noqa: F401
