"""Chamfer-6D distance (drop-in for
third_party/ChamferDistancePytorch/chamfer6D/dist_chamfer_6D.py): nearest
neighbours over 6-component points, e.g. xyz + rgb clouds (callers scale the
colour channels themselves, as with the reference's module).
Built by pcfm/chamfer_dist.py, which says what each name is.
"""
from pcfm.chamfer_dist import make

__all__ = ["chamfer_6D", "chamfer_6DFunction", "chamfer_6DDist"]

chamfer_6D, _, chamfer_6DFunction, chamfer_6DDist = make(6)
