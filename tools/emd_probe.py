"""EMD at the bench size (B=8, N=M=2048), default form: ms per call (events and
host clock) of the forward with match kept, the cost-only forward and forward
plus backward, one JSON line each:

    python tools/emd_probe.py [N [f32|f64]]

Run under rocprofv3 --kernel-trace --stats
for the per-kernel split; PCFM_LIB selects the library (A/B of two builds)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]

import torch  # noqa: E402


def main():
    from pcfm import _lib
    from PyTorchEMD.emd import earth_mover_distance
    _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    b, n = 8, int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    dt = sys.argv[2] if len(sys.argv) > 2 else "f32"
    dtype = {"f32": torch.float32, "f64": torch.float64}[dt]
    p1 = torch.rand(b, n, 3, device=dev, generator=g, dtype=dtype)
    p2 = torch.rand(b, n, 3, device=dev, generator=g, dtype=dtype)
    x = p1.detach().requires_grad_(True)  # the forward a backward follows: match kept

    def fwd_match():
        return earth_mover_distance(x, p2, transpose=False)

    def fwd_cost_only():
        return earth_mover_distance(p1, p2, transpose=False)

    def fwd_bwd():
        x.grad = None
        d = earth_mover_distance(x, p2, transpose=False)
        d.sum().backward()
        return d

    for what, fn in (("fwd_match", fwd_match), ("fwd_cost_only", fwd_cost_only),
                     ("fwd_bwd", fwd_bwd)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            d = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        host = (time.perf_counter() - t0) * 1e3 / reps
        print(json.dumps({"what": what, "b": b, "n": n, "dtype": dt, "ms_events": e0.elapsed_time(e1) / reps,
                          "ms_host": host, "cost0": float(d.detach()[0])}), flush=True)


if __name__ == "__main__":
    main()
