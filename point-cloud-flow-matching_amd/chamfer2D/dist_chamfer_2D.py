"""Chamfer-2D distance (drop-in for
third_party/ChamferDistancePytorch/chamfer2D/dist_chamfer_2D.py): nearest
neighbours over 2-component points (planar clouds, image coordinates).
Built by pcfm/chamfer_dist.py, which says what each name is.
"""
from pcfm.chamfer_dist import make

__all__ = ["chamfer_2D", "chamfer_2DFunction", "chamfer_2DDist"]

chamfer_2D, _, chamfer_2DFunction, chamfer_2DDist = make(2)
