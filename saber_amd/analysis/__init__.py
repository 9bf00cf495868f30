"""Post-segmentation analysis on the device: refinement of organelle labels against a membrane segmentation
(saber/analysis/refine_membranes.py).  Organelle statistics (saber/analysis/organelle_statistics.py) are not built."""
from .refine_membranes import FilteringConfig, OrganelleMembraneFilter

__all__ = ["FilteringConfig", "OrganelleMembraneFilter"]
