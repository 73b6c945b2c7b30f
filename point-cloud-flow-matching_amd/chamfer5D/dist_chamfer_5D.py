"""Chamfer-5D distance (drop-in for
third_party/ChamferDistancePytorch/chamfer5D/dist_chamfer_5D.py): nearest
neighbours over 5-component points (e.g. xyz plus two attribute channels; callers
scale the extra channels themselves, as with the reference's module).
Built by pcfm/chamfer_dist.py, which says what each name is.
"""
from pcfm.chamfer_dist import make

__all__ = ["chamfer_5D", "chamfer_5DFunction", "chamfer_5DDist"]

chamfer_5D, _, chamfer_5DFunction, chamfer_5DDist = make(5)
