"""F-score of two clouds from their Chamfer outputs (drop-in for
third_party/ChamferDistancePytorch/fscore.py)."""
import torch


def fscore(dist1, dist2, threshold=0.001):
    """dist1 (B, N), dist2 (B, M): the SQUARED nearest-neighbour distances a
    chamfer_{k}DDist returns, so `threshold` is a squared length too.
    -> (fscore, precision_1, precision_2), each (B,): the fractions of points
    closer than the threshold in either direction and their harmonic mean
    (0 where both fractions are 0)."""
    precision_1 = (dist1 < threshold).float().mean(dim=1)
    precision_2 = (dist2 < threshold).float().mean(dim=1)
    f = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    return torch.nan_to_num(f, nan=0.0), precision_1, precision_2
