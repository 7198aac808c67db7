from .move import Move
from .device import DeviceMove
from .stretch import StretchMove
from .gaussian import GaussianMove, MHMove
from .distgen import DistributionGenerate
from .mtdistgen import MTDistGenMove
from .tempering import TemperatureControl, make_ladder

__all__ = ["Move", "DeviceMove", "StretchMove", "GaussianMove", "MHMove", "DistributionGenerate", "MTDistGenMove", "TemperatureControl",
           "make_ladder"]
