"""The barotropic vorticity model, the classical baseline of DLWP forecasts, stepped for many initial states at once."""
from .model import BarotropicModel

__all__ = ['BarotropicModel']
