"""Post-segmentation analysis on the device: refinement of organelle labels against a membrane segmentation
(saber/analysis/refine_membranes.py) and organelle coordinates and size statistics (saber/analysis/organelle_statistics.py)."""
from .organelle_statistics import extract_organelle_statistics, organelle_table, save_coordinates_to_copick
from .refine_membranes import FilteringConfig, OrganelleMembraneFilter

__all__ = ["FilteringConfig", "OrganelleMembraneFilter", "extract_organelle_statistics", "organelle_table", "save_coordinates_to_copick"]
