"""bench.py's options, without a GPU: a plain run keeps only the timed steps,
--full turns the other legs back on, --dump-outputs writes the last step's
results as bounded float32 arrays."""
import glob
import os
import sys

import numpy as np

import bench
from pcfm.train import TrainConfig, Trainer, synthetic_batch


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_drops_every_leg_but_the_timed_steps(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_chamfer and a.no_event_timing


def test_full_keeps_the_legs_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_cpu_baseline or a.no_chamfer or a.no_event_timing)
    a = _parse(monkeypatch, "--full", "--no-chamfer", "--dump-outputs", "d")
    assert a.no_chamfer and not a.no_cpu_baseline and a.dump_outputs == "d"


def test_dump_outputs_writes_the_steps_results(tmp_path, monkeypatch):
    cfg = TrainConfig(batch_size=2, num_points=512, ctx_stage_channels=[32, 64, 64],
                      ctx_stage_res=[8, 4, 4], pf_width=64, lf_width=64, enc_width=32,
                      latent_dim=16, steps_per_epoch=10, epochs=2)
    tr = Trainer(cfg, "cpu")
    tr.train_mode()
    last = tr.step(synthetic_batch(cfg, "cpu"), epoch=201)
    n_pf = sum(v.numel() for v in tr.pf.state_dict().values())
    cap = n_pf // 3  # state_pf and ema_pf are sampled, the smaller arrays are whole
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", cap)
    bench.dump_outputs(tr, last, str(tmp_path / "a"))
    bench.dump_outputs(tr, last, str(tmp_path / "b"))
    got = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))}
    assert set(got) == {"loss_point", "loss_latent", "grad_norm", "state_enc", "state_pf",
                        "state_lf", "ema_pf", "ema_lf"}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert got["loss_point"][0] == np.float32(last["loss_point"].item())
    assert got["grad_norm"][0] == np.float32(float(tr.last_grad_norm))
    enc = np.concatenate([v.detach().reshape(-1).float().numpy()
                          for v in tr.enc.state_dict().values()])
    assert np.array_equal(got["state_enc"], enc)
    pf = np.concatenate([v.detach().reshape(-1).float().numpy()
                         for v in tr.pf.state_dict().values()])
    idx = np.sort(np.random.default_rng(0).integers(0, n_pf, cap))
    assert got["state_pf"].shape == (cap,) and np.array_equal(got["state_pf"], pf[idx])
    for name, v in got.items():  # the sample is fixed: a second dump is identical
        assert np.array_equal(v, np.load(str(tmp_path / "b" / (name + ".npy"))))


def test_dump_stays_under_64_mb_at_any_model_size():
    # 3 scalars + 5 state arrays of at most DUMP_MAX_ELEMS float32 each
    assert 5 * bench.DUMP_MAX_ELEMS * 4 + 3 * 4 <= 64 * 10 ** 6
